// rope_math.hpp -- RoPE on one 8-element piece pair, and the bf16 <-> fp32 steps it is made of, shared by every kernel that rotates a head
// (rope_kernel / rope_append_kernel in decoder_ops.hip, attn_decode_one_kernel in attention_decode.hip, decode_attn_scores_kernel in decode.hip) so that the
// fused and the separate paths produce the same bits.
//   forward  (x1, x2) -> (x1 c - x2 s, x2 c + x1 s);  inverse (the backward pass): (g1 c + g2 s, g2 c - g1 s)
// with x1 = piece c of a head's first half, x2 = piece c of its second half, and cos / sin rounded to bf16 first: HF holds them in the activation dtype
// (modeling_llama.py:163-165).
#pragma once
#include <hip/hip_runtime.h>

namespace ecgb {

using bf16_row8 = __attribute__((ext_vector_type(8))) unsigned short;      // one 16-byte piece of a bf16 row

__device__ __forceinline__ float bf_value(unsigned short u) { return __uint_as_float((unsigned)u << 16); }
// round to nearest even (one v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned short bf_bits(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }

template <bool INVERSE>
__device__ __forceinline__ void rope_pair(bf16_row8 &a, bf16_row8 &b, const float *pc, const float *ps)
{
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float cc = bf_value(bf_bits(pc[j])), ss = bf_value(bf_bits(ps[j]));
        const float x1 = bf_value(a[j]), x2 = bf_value(b[j]);
        if (!INVERSE) { a[j] = bf_bits(x1 * cc - x2 * ss); b[j] = bf_bits(x2 * cc + x1 * ss); }
        else { a[j] = bf_bits(x1 * cc + x2 * ss); b[j] = bf_bits(x2 * cc - x1 * ss); }
    }
}

}  // namespace ecgb
