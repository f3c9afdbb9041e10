// attention_probs.hip -- the attention probabilities the fused forward never forms (HF's `output_attentions`), recomputed from q, k and the row log-sum-exps
// ecgb_attn_fwd leaves behind:  P[b,h,i,j] = exp2(scale * log2 e * q_i.k_j - lse[b,h,i]) on the visible keys, 0 elsewhere, 1/S across rows with no visible key.
//
// One workgroup of four waves per (batch, 64-query block, 64-key block) tile, the tiles above the diagonal included (they hold zeros, or 1/S in rows without
// a key).  The workgroup walks every query head of the batch row in ascending order, a KV group at a time: the group's K fragments stay in registers while its
// query heads pass; wave w computes the 32 x 32 quarter (query half w / 2, key half w % 2) with v_mfma_f32_32x32x16_bf16 (A = q rows, B = k rows: a lane holds
// one key and 16 query rows).  Quarters with every key after every query skip the products.
//   * full form (bf16 [B, Hq, S, S]): the quarter goes to a double-buffered 64 x 64 LDS tile, one barrier a head, and leaves as whole 128-byte row segments
//     (16-byte stores where S % 8 == 0; 4- or 2-byte stores where rows are not 16-byte aligned, e.g. S = 2050);
//   * sum form (fp32 [B, S, S]): the heads are added in fp32 registers in ascending order and stored once (32 lanes = 128 contiguous bytes a row), so every
//     launch gives the same bits, with or without the full form beside it.
// No device code is shared with the training kernels (attention.hip / attention_d256.hip); the launch helper is (attention_common.inc).
#include <cmath>

#include "attention_common.inc"
#include "../../include/ecgbyte_decoder.h"

namespace {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

constexpr int kTile = 64;
constexpr int kLdsRow = kTile + 8;     // bf16 elements a staged row: 144 bytes (16-byte aligned, the two wave halves' rows 4 apart land on different banks)

struct ProbsArgs {
    const unsigned short *q, *k;       // [B*S rows], row strides ldq / ldk; query head h at q + h*D, KV head g at k + g*D
    long long ldq, ldk;
    const float *mask;                 // [B, S]
    const float *lse;                  // [B, Hq, S]  (log2 domain, scale folded in; +inf: no visible key)
    unsigned short *p;                 // bf16 [B, Hq, S, S] or null
    float *psum;                       // fp32 [B, S, S] or null
    float weight;
    int accumulate;
    int B, S, Hq, Hkv, nblk;
    float sc;                          // scale * log2 e
    float inv_s;                       // 1 / S
};

__device__ __forceinline__ unsigned short f2bf_rne(float x)        // x finite and >= 0 here
{
    const unsigned u = __float_as_uint(x);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// STORE: 8 = 16-byte row pieces (S % 8 == 0), 2 = 4-byte pairs (S even), 1 = 2-byte elements
template <int D, int STORE>
__global__ __launch_bounds__(256) void attn_probs_kernel(ProbsArgs A)
{
    __shared__ __attribute__((aligned(16))) unsigned short lds[2][kTile * kLdsRow];
    const int S = A.S, nblk = A.nblk;
    const long long t = blockIdx.x;
    const int b = (int)(t / ((long long)nblk * nblk));
    const int rem = (int)(t % ((long long)nblk * nblk));
    const int qb = rem / nblk, kb = rem % nblk;                    // key block fastest: neighbouring workgroups share the q rows
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, hh = lane >> 5;
    const int wq = wave >> 1, wk = wave & 1;
    const int q0 = qb * kTile + wq * 32, k0 = kb * kTile + wk * 32;
    const bool products = k0 <= q0 + 31 && k0 < S && q0 < S;       // some key of the quarter is visible to some row of it
    const int G = A.Hq / A.Hkv;

    const int j = k0 + lr;                                           // the lane's key
    const bool key_vis = j < S && A.mask[(long long)b * S + min(j, S - 1)] != 0.f;
    int rows[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rows[r] = q0 + 8 * (r >> 2) + 4 * hh + (r & 3);

    const unsigned short *qrow = A.q + ((long long)b * S + min(q0 + lr, S - 1)) * A.ldq + hh * 8;
    const unsigned short *krow = A.k + ((long long)b * S + min(k0 + lr, S - 1)) * A.ldk + hh * 8;
    const bool want_p = A.p != nullptr, want_sum = A.psum != nullptr;

    f32x16 sum;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] = 0.f;

    for (int g = 0; g < A.Hkv; ++g) {
        bf16x8 kf[D / 16];
        if (products) {
#pragma unroll
            for (int ks = 0; ks < D / 16; ++ks) kf[ks] = *reinterpret_cast<const bf16x8 *>(krow + g * D + ks * 16);
        }
        for (int hq = g * G; hq < (g + 1) * G; ++hq) {
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
            if (products) {
#pragma unroll
                for (int ks = 0; ks < D / 16; ++ks) {
                    const bf16x8 qf = *reinterpret_cast<const bf16x8 *>(qrow + hq * D + ks * 16);
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kf[ks], s, 0, 0, 0);
                }
            }
            const float *lse_h = A.lse + ((long long)b * A.Hq + hq) * S;
            float p[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = rows[r];
                const float l = lse_h[min(i, S - 1)];
                float v = 0.f;
                if (l == INFINITY) v = A.inv_s;
                else if (j <= i && key_vis) v = __builtin_amdgcn_exp2f(s[r] * A.sc - l);
                p[r] = v;
            }
            if (want_sum) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sum[r] += p[r];
            }
            if (want_p) {
                unsigned short *buf = lds[hq & 1];
#pragma unroll
                for (int r = 0; r < 16; ++r) buf[(rows[r] - qb * kTile) * kLdsRow + wk * 32 + lr] = f2bf_rne(p[r]);
                __syncthreads();      // the other buffer was last read before the previous barrier: one barrier a head
                unsigned short *out = A.p + ((long long)b * A.Hq + hq) * S * S;
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) {
                    const int c = threadIdx.x + c2 * 256, row = c >> 3, col = (c & 7) * 8;
                    const int i = qb * kTile + row, j0 = kb * kTile + col;
                    if (i >= S || j0 >= S) continue;
                    const u32x4 v = *reinterpret_cast<const u32x4 *>(&buf[row * kLdsRow + col]);
                    unsigned short *dst = out + (long long)i * S + j0;
                    if constexpr (STORE == 8) {
                        *reinterpret_cast<u32x4 *>(dst) = v;
                    } else if constexpr (STORE == 2) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (j0 + 2 * e < S) reinterpret_cast<unsigned *>(dst)[e] = v[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (j0 + e < S) dst[e] = (unsigned short)(v[e >> 1] >> (16 * (e & 1)));
                    }
                }
            }
        }
    }
    if (want_sum && j < S) {
        float *out = A.psum + (long long)b * S * S + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = rows[r];
            if (i >= S) continue;
            const float add = A.weight * sum[r];
            float *dst = out + (long long)i * S;
            *dst = A.accumulate ? *dst + add : add;
        }
    }
}

template <int D>
int launch_probs(const ProbsArgs &A, unsigned grid, void *stream)
{
    void (*kern)(ProbsArgs) = attn_probs_kernel<D, 8>;
    if (A.S % 8) kern = A.S % 2 == 0 ? attn_probs_kernel<D, 2> : attn_probs_kernel<D, 1>;
    return launch_attn(kern, "attn_probs_kernel", grid, 256, 0, stream, A);
}

}  // namespace

extern "C" int ecgb_attn_probs(const void *q_dev, long long ldq, const void *k_dev, long long ldk, const float *attn_mask_dev,
                               const float *lse_dev, void *p_dev, float *psum_dev, float psum_weight, int psum_accumulate,
                               int batch, int seq, int n_q_heads, int n_kv_heads, int head_dim, float scale, void *stream)
{
    if (!q_dev || !k_dev || !attn_mask_dev || !lse_dev || (!p_dev && !psum_dev)) {
        ecgb::set_error("ecgb_attn_probs: null pointer (q, k, mask and lse are required, and at least one of p / psum)");
        return ECGB_ERR_INVALID;
    }
    if (batch <= 0 || seq <= 0 || n_q_heads <= 0 || n_kv_heads <= 0 || n_q_heads % n_kv_heads) {
        ecgb::set_error("ecgb_attn_probs: bad shape");
        return ECGB_ERR_INVALID;
    }
    if (head_dim != 64 && head_dim != 128 && head_dim != 256) {
        ecgb::set_error("ecgb_attn_probs: head_dim must be 64, 128 or 256");
        return ECGB_ERR_UNSUPPORTED;
    }
    if (ldq % 8 || ldk % 8 || ldq < (long long)n_q_heads * head_dim || ldk < (long long)n_kv_heads * head_dim ||
        (((uintptr_t)q_dev | (uintptr_t)k_dev) & 15)) {
        ecgb::set_error("ecgb_attn_probs: q / k need 16-byte aligned rows holding every head (strides multiples of 8 elements)");
        return ECGB_ERR_UNSUPPORTED;
    }
    const long long nblk = (seq + kTile - 1) / kTile;
    const long long grid = (long long)batch * nblk * nblk;
    if (grid > 0x7fffffffll) {
        ecgb::set_error("ecgb_attn_probs: too many tiles for one launch");
        return ECGB_ERR_UNSUPPORTED;
    }
    ProbsArgs A = {};
    A.q = (const unsigned short *)q_dev; A.k = (const unsigned short *)k_dev; A.ldq = ldq; A.ldk = ldk;
    A.mask = attn_mask_dev; A.lse = lse_dev; A.p = (unsigned short *)p_dev; A.psum = psum_dev;
    A.weight = psum_weight; A.accumulate = psum_accumulate ? 1 : 0;
    A.B = batch; A.S = seq; A.Hq = n_q_heads; A.Hkv = n_kv_heads; A.nblk = (int)nblk;
    A.sc = scale * kLog2e;
    A.inv_s = 1.0f / (float)seq;
    if (head_dim == 64) return launch_probs<64>(A, (unsigned)grid, stream);
    if (head_dim == 128) return launch_probs<128>(A, (unsigned)grid, stream);
    return launch_probs<256>(A, (unsigned)grid, stream);
}
