// attention_decode.hip -- a decode step's attention for MI355X (gfx950): one query per (batch, head) against the KV cache, head_dim 64 / 128 / 256.
//
// Reference: LlamaSdpaAttention.forward with a DynamicCache (modeling_llama.py:526-614, cache_utils.py:408-470): key j is visible iff mask[b, j] != 0; softmax in
// fp32, P cast to bf16 for P.V.  Rows without a visible key produce zeros.
//
// q [B, Hq*D]; k/v cache rows [B, cap] with row stride ld (elements), kv head g at + g*D; len = keys in the cache (incl. the new one), an argument or -- when the
// step is replayed from a captured graph -- in device memory.  Three forms of the same arithmetic (decode_attn.inc holds it, once):
//   attn_decode_kernel                             one workgroup of 16 waves a head: short caches
//   attn_decode_scores / values / combine_kernel   a head's keys split over workgroups (long caches, few heads: one CU sustains only ~64 GB/s at the memory
//                                                  latency, the chip has 256)
//   attn_decode_one_kernel                         RoPE + cache append + the three above in one launch
// decode.hip's grouped kernels (all query heads of a KV group a workgroup) are the fourth.  All read the cache once, every row as one coalesced D*2-byte piece.
#include "attention_common.inc"
#include "decode_attn.inc"

#include <algorithm>

namespace {

namespace da = ecgb_dattn;
using da::row8;

// ---- one workgroup a head.  grid (Hq, B), 16 waves: scores and probabilities in LDS (fp32)
constexpr int kDecodeThreads = 1024;
template <int D>
__global__ __launch_bounds__(kDecodeThreads) void attn_decode_kernel(const unsigned short *q, const unsigned short *kc, const unsigned short *vc,
                                                                     long long ld, long long cap, const float *mask, long long mask_ld,
                                                                     unsigned short *o, int len_arg, const int *len_dev, int Hq, int Hkv, float scale)
{
    constexpr int NW = kDecodeThreads / 64, EPL = D / 64, KU = 16, VU = 8;
    extern __shared__ float s_p[];                      // [len] scores / probabilities, later [kDecodeThreads * 8] partial outputs; [2 * NW] reductions
    const int len = len_dev ? *len_dev : len_arg;
    const int rows_lds = len_dev ? (((int)cap + 3) & ~3) : ((len + 3) & ~3);
    float *s_red = s_p + max(rows_lds, kDecodeThreads * 8);   // behind the scores / the P.V partial sums, whichever is longer
    const int hq = blockIdx.x, b = blockIdx.y, g = hq / (Hq / Hkv), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned short *qp = q + ((long long)b * Hq + hq) * D;
    float qf[EPL];
#pragma unroll
    for (int t = 0; t < EPL; ++t) qf[t] = da::bf_value(qp[lane * EPL + t]);
    const unsigned short *K = kc + (long long)b * cap * ld + (long long)g * D;
    const unsigned short *V = vc + (long long)b * cap * ld + (long long)g * D;
    const float *mrow = mask + (long long)b * mask_ld;

    float m = -INFINITY, l;
    for (int j0 = wave; j0 < len; j0 += KU * NW) {
        uint2 kr[KU];
        float mk[KU], part[KU];
        da::load_keys<D, NW, KU>(kr, mk, K, ld, mrow, j0, len, lane);
        da::dot_keys<D, NW, KU, false>(part, qf, kr, qf, j0, -1);
        da::finish_scores<NW, KU>(part, mk, j0, len, scale, lane, m, [&](int j, float s) { s_p[j] = s; });
    }
    da::workgroup_stats<kDecodeThreads, true>(m, s_p, len, s_red, tid, m, l);      // s_p: the exponentials now
    const float inv = da::inverse_or_zero(l);

    const int piece = tid % (D / 8), slice = tid / (D / 8);
    float acc[8];
    row8 vv[VU];
    da::pv_range<D, kDecodeThreads, VU, false>(acc, vv, slice, len,
        [&](int j) { return *reinterpret_cast<const row8 *>(V + (long long)j * ld + piece * 8); },
        [&](int j) { return s_p[j]; }, [&](float e) { return e * inv; });
    __syncthreads();                                            // s_p is dead: the slices' partial sums go there (the launch sizes the buffer for it)
    const float sum = da::slice_sum<D, kDecodeThreads>(acc, s_p, tid);
    if (tid < D) o[((long long)b * Hq + hq) * D + tid] = da::bf_bits(sum);
}

// ---- the keys of a head split over several workgroups.  Three small kernels:
//   scores   grid (splits, Hq, B): the scores of the split's keys to scratch (fp32) + the split's max and sum of exponentials;
//   values   grid (splits, Hq, B): global max / sum from the splits' statistics, p_j = bf16(exp(s_j - max) / sum), partial P.V of the split's keys to scratch (fp32);
//   combine  grid (Hq, B): the partial outputs added in split order, cast to bf16.
// scratch (floats): scores [B, Hq, cap] | stats [B, Hq, splits, 2] | partial outputs [B, Hq, splits, D].
constexpr int kSplitThreads = 256;
constexpr int kSplitMaxChunk = 2048;                     // keys per split the scores kernel can hold (the launcher raises n_splits to fit)
constexpr int kSplitKU = 16, kSplitVU = 8;               // key rows a wave / value rows a thread keeps in flight

// a split's keys [k0, k1).  chunk_arg: from the host for a length it knows; a device-resident length (a replayed graph) gives the same split of the keys
__device__ __forceinline__ void split_range(int len, int chunk_arg, bool dyn, int &k0, int &k1)
{
    const int chunk = dyn ? (len + (int)gridDim.x - 1) / (int)gridDim.x : chunk_arg;
    k0 = (int)blockIdx.x * chunk;
    k1 = min(len, k0 + chunk);
}

template <int D>
__global__ __launch_bounds__(kSplitThreads) void attn_decode_scores_kernel(const unsigned short *q, const unsigned short *kc, long long ld, long long cap,
                                                                           const float *mask, long long mask_ld, float *scores, float *stats,
                                                                           int len_arg, int chunk_arg, const int *len_dev, int Hq, int Hkv, float scale)
{
    constexpr int NW = kSplitThreads / 64, EPL = D / 64, KU = kSplitKU;
    __shared__ float s_red[2 * NW];
    __shared__ float s_sc[kSplitMaxChunk];                // the split's scores once more: the sum of exponentials reads them here
    const int sp = blockIdx.x, hq = blockIdx.y, b = blockIdx.z, g = hq / (Hq / Hkv), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int k0, k1;
    split_range(len_dev ? *len_dev : len_arg, chunk_arg, len_dev != nullptr, k0, k1);
    const unsigned short *qp = q + ((long long)b * Hq + hq) * D;
    float qf[EPL];
#pragma unroll
    for (int t = 0; t < EPL; ++t) qf[t] = da::bf_value(qp[lane * EPL + t]);
    const unsigned short *K = kc + (long long)b * cap * ld + (long long)g * D;
    const float *mrow = mask + (long long)b * mask_ld;
    float *srow = scores + ((long long)b * Hq + hq) * cap;
    float m = -INFINITY, l;
    for (int j0 = k0 + wave; j0 < k1; j0 += KU * NW) {
        uint2 kr[KU];
        float mk[KU], part[KU];
        da::load_keys<D, NW, KU>(kr, mk, K, ld, mrow, j0, k1, lane);
        da::dot_keys<D, NW, KU, false>(part, qf, kr, qf, j0, -1);
        da::finish_scores<NW, KU>(part, mk, j0, k1, scale, lane, m, [&](int j, float s) { srow[j] = s; s_sc[j - k0] = s; });
    }
    da::workgroup_stats<kSplitThreads, false>(m, s_sc, k1 - k0, s_red, tid, m, l);
    if (tid == 0) {
        float *st = stats + (((long long)b * Hq + hq) * gridDim.x + sp) * 2;
        st[0] = m;
        st[1] = l;
    }
}

template <int D>
__global__ __launch_bounds__(kSplitThreads) void attn_decode_values_kernel(const unsigned short *vc, long long ld, long long cap, const float *scores,
                                                                           const float *stats, float *partial, int len_arg, int chunk_arg, const int *len_dev,
                                                                           int Hq, int Hkv)
{
    constexpr int TPR = D / 8, NS = kSplitThreads / TPR, VU = kSplitVU;
    __shared__ float s_part[NS * D];
    const int sp = blockIdx.x, hq = blockIdx.y, b = blockIdx.z, g = hq / (Hq / Hkv), tid = threadIdx.x;
    const int n_splits = gridDim.x;
    int k0, k1;
    split_range(len_dev ? *len_dev : len_arg, chunk_arg, len_dev != nullptr, k0, k1);
    float m, inv;
    da::merge_splits(stats + ((long long)b * Hq + hq) * n_splits * 2, n_splits, m, inv);
    const unsigned short *V = vc + (long long)b * cap * ld + (long long)g * D;
    const float *srow = scores + ((long long)b * Hq + hq) * cap;
    const int piece = tid % TPR, slice = tid / TPR;
    float acc[8];
    row8 vv[VU];
    da::pv_range<D, kSplitThreads, VU, false>(acc, vv, k0 + slice, k1,
        [&](int j) { return *reinterpret_cast<const row8 *>(V + (long long)j * ld + piece * 8); },
        [&](int j) { return srow[j]; }, [&](float s) { return da::exp_or_zero(s, m) * inv; });
    const float sum = da::slice_sum<D, kSplitThreads>(acc, s_part, tid);
    if (tid < D) partial[(((long long)b * Hq + hq) * n_splits + sp) * D + tid] = sum;
}

template <int D>
__global__ __launch_bounds__(D) void attn_decode_combine_kernel(const float *partial, unsigned short *o, int n_splits, int Hq)
{
    const int hq = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float *p = partial + ((long long)b * Hq + hq) * n_splits * D + tid;
    o[((long long)b * Hq + hq) * D + tid] = da::bf_bits(da::combine_splits(n_splits, [&](int t) { return p[(long long)t * D]; }));
}

// ---- round 6: the four launches of a decode step's attention (rope_append, scores, values, combine: 4.8 + 11.2 + 5.3 + 4.8 us a layer in the replayed graph at the
// C5 shape, every one of them on the ~5 us floor of a dependent launch) as ONE.  grid (splits, Hq, B) as the split kernels; the workgroups of a (sequence, head) meet
// twice through counters in device memory:
//   0  RoPE of the head's q and of the KV head's new key in LDS (rope_append_kernel's arithmetic; the workgroup of split 0 of the group's first head writes the rotated
//      key and the value to cache row len - 1 -- nobody reads that row in this launch: the split that owns key len - 1 takes it from LDS / from qkv)
//   1  the split's scores into LDS, its maximum and sum of exponentials to `stats`;  wait until every split's pair is there (a pair holds kDecodeOneEmpty until stored)
//   2  softmax over the splits' statistics, P.V of the split's keys to `partial`;  counter B: the last to arrive adds the partial outputs in split order, puts the
//      empty marks back and clears the counter for the next launch (a replayed graph never does itself).
// The same routines in the same order: the same bits as the four launches (tests/test_gpu_decode_fused.py).  The wait in step 1 needs every workgroup of the
// launch resident at once: the host only takes this form for splits * Hq * B <= two workgroups a CU.
// "not stored yet" in the splits' statistics: a NaN with a payload no arithmetic produces (a sum or maximum that IS NaN -- garbage in -- is the canonical one and ends the wait like any value)
constexpr unsigned kDecodeOneEmpty = 0x7FC0DEADu;
struct DecodeOneArgs {
    const unsigned short *qkv;    // [B, (Hq + 2 Hkv) D]: the step's projection, not written (q and the new key are rotated into LDS)
    long long ld_qkv;
    const float *cs, *sn;         // RoPE tables of the step's positions [B, D / 2]
    unsigned short *cache;        // [B, cap, ld]: keys | values
    long long cap, ld;
    const float *mask;
    long long mask_ld;
    float *stats, *partial;       // [B, Hq, splits, 2] (kDecodeOneEmpty between launches), [B, Hq, splits, D]
    unsigned *cnt;                // [B, Hq, 2], zero between launches (word 1: the tickets of the second meeting)
    unsigned short *o;            // [B, Hq D]
    const int *len_dev;
    int len_arg, Hq, Hkv;
    float scale;
};

template <int D>
__global__ __launch_bounds__(kSplitThreads) void attn_decode_one_kernel(DecodeOneArgs A)
{
    constexpr int NW = kSplitThreads / 64, EPL = D / 64, KU = kSplitKU, half = D / 2;
    constexpr int TPR = D / 8, NS = kSplitThreads / TPR, VU = kSplitVU;
    __shared__ __attribute__((aligned(16))) unsigned short s_q[D], s_kn[D];
    __shared__ float s_red[2 * NW];
    __shared__ float s_sc[kSplitMaxChunk];
    __shared__ float s_part[NS * D];
    __shared__ float s_st[2 * 64];                         // the splits' (maximum, sum) pairs (splits <= 64)
    __shared__ unsigned s_last;
    const int sp = blockIdx.x, hq = blockIdx.y, b = blockIdx.z, G = A.Hq / A.Hkv, g = hq / G, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_splits = gridDim.x;
    const int len = A.len_dev ? *A.len_dev : A.len_arg;
    int k0, k1;
    split_range(len, 0, true, k0, k1);
    const unsigned short *row = A.qkv + (long long)b * A.ld_qkv;
    // Memory between the workgroups of a (sequence, head): everything they exchange (statistics, partial outputs, counters) is written and read with agent-scope
    // RELAXED atomics -- stores that go through to the level the XCDs share, loads that do not stop at this XCD's L2 -- ordered by hand: a wave's stores are
    // complete (s_waitcnt vmcnt(0)) before its workgroup's counter moves.  Release / acquire orderings on the counters cost a write-back of the whole L2 per
    // arrival and an invalidate per poll: the launch took 24 us that way, as long as the four it replaces.
    auto ld_f = [](const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto st_f = [](float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    const unsigned short *K = A.cache + (long long)b * A.cap * A.ld + (long long)g * D;
    const unsigned short *V = A.cache + (long long)b * A.cap * A.ld + (long long)A.Hkv * D + (long long)g * D;
    const unsigned short *vnew = row + (long long)(A.Hq + A.Hkv + g) * D;
    const float *mrow = A.mask + (long long)b * A.mask_ld;
    const int piece = tid % TPR, slice = tid / TPR;
    // ---- the first batch of keys and values is asked for before anything else (a split of the C5 step is one batch: 61 keys): the loads fly under the RoPE and
    // the values' under the scores and the first meeting
    uint2 kr[KU];
    float mk[KU];
    row8 vv[VU];
    auto v_row = [&](int j) { return *reinterpret_cast<const row8 *>((j == len - 1 ? vnew : V + (long long)j * A.ld) + piece * 8); };
    if (k0 + wave < k1) da::load_keys<D, NW, KU>(kr, mk, K, A.ld, mrow, k0 + wave, k1, lane);
    if (k0 + slice < k1) da::load_values<D, kSplitThreads, VU>(vv, k0 + slice, k1, v_row);
    // ---- 0: RoPE -- piece c (eight elements) of a head's first half with piece c of its second half
    if (tid < 2 * (half / 8)) {
        const int c = tid % (half / 8), h = tid / (half / 8);                  // h 0: the query head; 1: the new key of its KV head
        const unsigned short *p = row + (long long)(h == 0 ? hq : A.Hq + g) * D + c * 8;
        row8 a = *reinterpret_cast<const row8 *>(p), bb = *reinterpret_cast<const row8 *>(p + half);
        ecgb::rope_pair<false>(a, bb, A.cs + (size_t)b * half + c * 8, A.sn + (size_t)b * half + c * 8);
        unsigned short *dst = h == 0 ? s_q : s_kn;
        *reinterpret_cast<row8 *>(dst + c * 8) = a;
        *reinterpret_cast<row8 *>(dst + half + c * 8) = bb;
        if (h == 1 && sp == 0 && hq == g * G) {                                // the append: rotated key
            unsigned short *kc = A.cache + ((long long)b * A.cap + (len - 1)) * A.ld + (size_t)g * D + c * 8;
            *reinterpret_cast<row8 *>(kc) = a;
            *reinterpret_cast<row8 *>(kc + half) = bb;
        }
    }
    if (sp == 0 && hq == g * G && tid >= 128 && tid < 128 + D / 8)             // the append: the value as it is
        *reinterpret_cast<row8 *>(A.cache + ((long long)b * A.cap + (len - 1)) * A.ld + (size_t)A.Hkv * D + (size_t)g * D + (tid - 128) * 8) =
            *reinterpret_cast<const row8 *>(vnew + (tid - 128) * 8);
    __syncthreads();
    // ---- 1: scores
    float qf[EPL], kn[EPL];
#pragma unroll
    for (int t = 0; t < EPL; ++t) { qf[t] = da::bf_value(s_q[lane * EPL + t]); kn[t] = da::bf_value(s_kn[lane * EPL + t]); }
    float m = -INFINITY, l;
    for (int j0 = k0 + wave; j0 < k1; j0 += KU * NW) {
        if (j0 != k0 + wave) da::load_keys<D, NW, KU>(kr, mk, K, A.ld, mrow, j0, k1, lane);
        float part[KU];
        da::dot_keys<D, NW, KU, true>(part, qf, kr, kn, j0, len - 1);
        da::finish_scores<NW, KU>(part, mk, j0, k1, A.scale, lane, m, [&](int j, float s) { s_sc[j - k0] = s; });
    }
    da::workgroup_stats<kSplitThreads, false>(m, s_sc, k1 - k0, s_red, tid, m, l);
    float *st = A.stats + ((long long)b * A.Hq + hq) * n_splits * 2;
    unsigned *cnt = A.cnt + ((long long)b * A.Hq + hq) * 2;
    if (tid == 0) {
        st_f(&st[2 * sp], m);
        st_f(&st[2 * sp + 1], l);
    }
    // ---- the first meeting: no counter.  A split's (maximum, sum) pair is kDecodeOneEmpty -- a NaN no sum produces -- until its workgroup has stored it (the scratch starts so and the last workgroup of
    // the launch puts it back): lane t polls pair t itself -- one round trip from the store to the values, where a counter cost an atomic, a poll and a load
    if (tid < 2 * n_splits) {
        const unsigned *sb = reinterpret_cast<const unsigned *>(st) + tid;
        unsigned v = __hip_atomic_load(sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (v == kDecodeOneEmpty) { __builtin_amdgcn_s_sleep(1); v = __hip_atomic_load(sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        s_st[tid] = __uint_as_float(v);
    }
    __syncthreads();
    // ---- 2: values
    float inv;
    da::merge_splits(s_st, n_splits, m, inv);
    float acc[8];
    da::pv_range<D, kSplitThreads, VU, true>(acc, vv, k0 + slice, k1, v_row,
        [&](int j) { return s_sc[j - k0]; }, [&](float s) { return da::exp_or_zero(s, m) * inv; });
    const float sum = da::slice_sum<D, kSplitThreads>(acc, s_part, tid);
    float *part_out = A.partial + ((long long)b * A.Hq + hq) * n_splits * D;
    if (tid < D) {
        st_f(&part_out[(long long)sp * D + tid], sum);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // this wave's part of the partial output has arrived
    }
    __syncthreads();
    if (tid == 0) s_last = __hip_atomic_fetch_add(&cnt[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(n_splits - 1) ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
    // ---- the last workgroup of the (sequence, head): the splits' partial outputs in split order
    if (tid < D)
        A.o[((long long)b * A.Hq + hq) * D + tid] = da::bf_bits(da::combine_splits(n_splits, [&](int t) { return ld_f(&part_out[(long long)t * D + tid]); }));
    // ready for the next launch: every workgroup of the (sequence, head) has read the statistics (it took its ticket after that)
    if (tid < 2 * n_splits) st_f(&st[tid], __uint_as_float(kDecodeOneEmpty));
    if (tid == 0) __hip_atomic_store(&cnt[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// cache[b, *len - 1, :] = src[b, col_off : col_off + width]   (the new token's roped K | V, position from device memory)
__global__ __launch_bounds__(256) void kv_append_kernel(const unsigned short *src, long long src_ld, long long col_off, int width,
                                                        unsigned short *cache, long long cap, const int *len_dev, int batch)
{
    const long long row = *len_dev - 1;
    const int per_row = width / 8;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < batch * per_row; i += gridDim.x * blockDim.x) {
        const int b = i / per_row, c = i % per_row;
        *reinterpret_cast<row8 *>(cache + ((long long)b * cap + row) * width + c * 8) =
            *reinterpret_cast<const row8 *>(src + (long long)b * src_ld + col_off + c * 8);
    }
}

}  // namespace

extern "C" size_t ecgb_attn_decode_split_scratch_bytes(long long capacity, int batch, int n_q_heads, int head_dim, int n_splits)
{
    if (capacity <= 0 || batch <= 0 || n_q_heads <= 0 || n_splits <= 0) return 0;
    // a split never holds more than kSplitMaxChunk keys: size for the splits the longest cache (capacity keys) can need
    const long long need_splits = (capacity + kSplitMaxChunk - 1) / kSplitMaxChunk;
    if (need_splits > n_splits) n_splits = (int)need_splits;
    return (size_t)batch * n_q_heads * ((size_t)capacity + (size_t)n_splits * (2 + (size_t)head_dim)) * sizeof(float);
}

namespace {

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, D>) for the head_dim the kernels are built for (the caller has checked it)
template <class F>
void with_head_dim(int head_dim, F f)
{
    if (head_dim == 64) f(std::integral_constant<int, 64>{});
    else if (head_dim == 128) f(std::integral_constant<int, 128>{});
    else f(std::integral_constant<int, 256>{});
}

// what every entry point checks, as the set of what is wrong: each reports it in its own words
enum : unsigned { kBadHeadDim = 1, kBadHeads = 2, kBadStride = 4, kBadLength = 8 };
unsigned decode_faults(int head_dim, int n_q_heads, int n_kv_heads, long long ld, int kv_len, const int *kv_len_dev, long long capacity)
{
    unsigned f = 0;
    if (head_dim != 64 && head_dim != 128 && head_dim != 256) f |= kBadHeadDim;
    if (n_q_heads <= 0 || n_kv_heads <= 0 || n_q_heads % n_kv_heads) f |= kBadHeads;
    if (ld % 8) f |= kBadStride;
    if (!kv_len_dev && (kv_len <= 0 || kv_len > capacity)) f |= kBadLength;      // a length in device memory is the caller's word
    return f;
}

int launch_attn_decode(const void *q_dev, const void *k_cache_dev, const void *v_cache_dev, long long ld, long long capacity,
                       const float *attn_mask_dev, long long mask_ld, void *o_dev, int batch, int kv_len, const int *kv_len_dev,
                       int n_q_heads, int n_kv_heads, int head_dim, float scale, void *stream)
{
    const unsigned faults = decode_faults(head_dim, n_q_heads, n_kv_heads, ld, kv_len, kv_len_dev, capacity);
    if (faults & kBadHeadDim) { ecgb::set_error("ecgb_attn_decode: head_dim must be 64, 128 or 256"); return ECGB_ERR_UNSUPPORTED; }
    if (batch <= 0 || faults) { ecgb::set_error("ecgb_attn_decode: bad shape"); return ECGB_ERR_INVALID; }
    const long long rows = kv_len_dev ? capacity : (long long)kv_len;
    const size_t lds = (std::max<size_t>((size_t)((rows + 3) & ~3ll), (size_t)kDecodeThreads * 8) + 2 * (kDecodeThreads / 64)) * 4;
    if (lds > 64 * 1024) { ecgb::set_error("ecgb_attn_decode: cache longer than ~16000 keys"); return ECGB_ERR_UNSUPPORTED; }
    with_head_dim(head_dim, [&](auto d) {
        hipLaunchKernelGGL(attn_decode_kernel<d()>, dim3((unsigned)n_q_heads, (unsigned)batch), dim3(kDecodeThreads), lds, (hipStream_t)stream,
                           (const unsigned short *)q_dev, (const unsigned short *)k_cache_dev, (const unsigned short *)v_cache_dev, ld, capacity, attn_mask_dev, mask_ld,
                           (unsigned short *)o_dev, kv_len, kv_len_dev, n_q_heads, n_kv_heads, scale);
    });
    return launched("attn_decode_kernel");
}

int launch_attn_decode_split(const char *who, const void *q_dev, const void *k_cache_dev, const void *v_cache_dev, long long ld, long long capacity,
                             const float *attn_mask_dev, long long mask_ld, void *o_dev, int batch, int kv_len, const int *kv_len_dev, int n_q_heads,
                             int n_kv_heads, int head_dim, float scale, int n_splits, void *scratch_dev, size_t scratch_bytes, void *stream)
{
    const unsigned faults = decode_faults(head_dim, n_q_heads, n_kv_heads, ld, kv_len, kv_len_dev, capacity);
    if (faults & kBadHeadDim) { ecgb::set_error(std::string(who) + ": head_dim must be 64, 128 or 256"); return ECGB_ERR_UNSUPPORTED; }
    if (!q_dev || !k_cache_dev || !v_cache_dev || !attn_mask_dev || !o_dev || !scratch_dev || batch <= 0 || capacity <= 0 || faults || n_splits <= 0 || n_splits > 1024) {
        ecgb::set_error(std::string(who) + ": bad argument");
        return ECGB_ERR_INVALID;
    }
    if (scratch_bytes < ecgb_attn_decode_split_scratch_bytes(capacity, batch, n_q_heads, head_dim, n_splits)) {
        ecgb::set_error(std::string(who) + ": scratch too small (ecgb_attn_decode_split_scratch_bytes)");
        return ECGB_ERR_INVALID;
    }
    // the split count is final BEFORE the scratch is laid out: stats and partial are indexed by gridDim.x.  A length in device memory can grow to the capacity.
    const long long longest = kv_len_dev ? capacity : (long long)kv_len;
    if ((longest + n_splits - 1) / n_splits > kSplitMaxChunk) n_splits = (int)((longest + kSplitMaxChunk - 1) / kSplitMaxChunk);
    float *scores = (float *)scratch_dev;
    float *stats = scores + (size_t)batch * n_q_heads * (size_t)capacity;
    float *partial = stats + (size_t)batch * n_q_heads * (size_t)n_splits * 2;
    const int chunk = kv_len_dev ? 0 : (kv_len + n_splits - 1) / n_splits;
    const dim3 grid((unsigned)n_splits, (unsigned)n_q_heads, (unsigned)batch), gc((unsigned)n_q_heads, (unsigned)batch);
    with_head_dim(head_dim, [&](auto d) {
        hipLaunchKernelGGL(attn_decode_scores_kernel<d()>, grid, dim3(kSplitThreads), 0, (hipStream_t)stream, (const unsigned short *)q_dev,
                           (const unsigned short *)k_cache_dev, ld, capacity, attn_mask_dev, mask_ld, scores, stats, kv_len, chunk, kv_len_dev, n_q_heads, n_kv_heads, scale);
        hipLaunchKernelGGL(attn_decode_values_kernel<d()>, grid, dim3(kSplitThreads), 0, (hipStream_t)stream, (const unsigned short *)v_cache_dev,
                           ld, capacity, scores, stats, partial, kv_len, chunk, kv_len_dev, n_q_heads, n_kv_heads);
        hipLaunchKernelGGL(attn_decode_combine_kernel<d()>, gc, dim3(d()), 0, (hipStream_t)stream, partial, (unsigned short *)o_dev, n_splits, n_q_heads);
    });
    return launched("attn_decode_split kernels");
}

}  // namespace

extern "C" int ecgb_attn_decode(const void *q_dev, const void *k_cache_dev, const void *v_cache_dev, long long ld, long long capacity,
                                const float *attn_mask_dev, long long mask_ld, void *o_dev, int batch, int kv_len, int n_q_heads,
                                int n_kv_heads, int head_dim, float scale, void *stream)
{
    return launch_attn_decode(q_dev, k_cache_dev, v_cache_dev, ld, capacity, attn_mask_dev, mask_ld, o_dev, batch, kv_len, nullptr,
                              n_q_heads, n_kv_heads, head_dim, scale, stream);
}

extern "C" int ecgb_attn_decode_dyn(const void *q_dev, const void *k_cache_dev, const void *v_cache_dev, long long ld, long long capacity,
                                    const float *attn_mask_dev, long long mask_ld, void *o_dev, int batch, const int *kv_len_dev,
                                    int n_q_heads, int n_kv_heads, int head_dim, float scale, void *stream)
{
    if (!kv_len_dev) { ecgb::set_error("ecgb_attn_decode_dyn: NULL length pointer"); return ECGB_ERR_INVALID; }
    return launch_attn_decode(q_dev, k_cache_dev, v_cache_dev, ld, capacity, attn_mask_dev, mask_ld, o_dev, batch, 0, kv_len_dev,
                              n_q_heads, n_kv_heads, head_dim, scale, stream);
}

extern "C" int ecgb_attn_decode_split(const void *q_dev, const void *k_cache_dev, const void *v_cache_dev, long long ld, long long capacity,
                                      const float *attn_mask_dev, long long mask_ld, void *o_dev, int batch, int kv_len, int n_q_heads,
                                      int n_kv_heads, int head_dim, float scale, int n_splits, void *scratch_dev, size_t scratch_bytes,
                                      void *stream)
{
    return launch_attn_decode_split("ecgb_attn_decode_split", q_dev, k_cache_dev, v_cache_dev, ld, capacity, attn_mask_dev, mask_ld, o_dev, batch, kv_len, nullptr,
                                    n_q_heads, n_kv_heads, head_dim, scale, n_splits, scratch_dev, scratch_bytes, stream);
}

extern "C" int ecgb_attn_decode_split_dyn(const void *q_dev, const void *k_cache_dev, const void *v_cache_dev, long long ld, long long capacity,
                                          const float *attn_mask_dev, long long mask_ld, void *o_dev, int batch, const int *kv_len_dev, int n_q_heads,
                                          int n_kv_heads, int head_dim, float scale, int n_splits, void *scratch_dev, size_t scratch_bytes,
                                          void *stream)
{
    if (!kv_len_dev) { ecgb::set_error("ecgb_attn_decode_split_dyn: NULL length pointer"); return ECGB_ERR_INVALID; }
    return launch_attn_decode_split("ecgb_attn_decode_split_dyn", q_dev, k_cache_dev, v_cache_dev, ld, capacity, attn_mask_dev, mask_ld, o_dev, batch, 0, kv_len_dev,
                                    n_q_heads, n_kv_heads, head_dim, scale, n_splits, scratch_dev, scratch_bytes, stream);
}

// floats of scratch ecgb_attn_decode_one needs (statistics, partial outputs, counters): before the first call the FIRST batch * n_q_heads * n_splits * 2 floats (the
// statistics) must hold the bit pattern 0x7FC0DEAD and the LAST batch * n_q_heads * 2 words (the counters) zero; every launch leaves them so
extern "C" size_t ecgb_attn_decode_one_scratch_floats(int batch, int n_q_heads, int head_dim, int n_splits)
{
    if (batch <= 0 || n_q_heads <= 0 || head_dim <= 0 || n_splits <= 0) return 0;
    return (size_t)batch * n_q_heads * ((size_t)n_splits * (2 + (size_t)head_dim) + 2);
}

// A decode step's RoPE + cache append + attention in ONE launch, from the step's raw q|k|v projection (q and k NOT rotated in place): the bits of ecgb_rope_append
// followed by ecgb_attn_decode_split[_dyn] with the same n_splits.  ECGB_ERR_UNSUPPORTED outside head_dim 64 / 128 / 256, n_splits <= 64, at most 2048 keys a split and
// n_splits * n_q_heads * batch <= two workgroups a CU (they wait for each other inside the launch: all of them must be resident).
extern "C" int ecgb_attn_decode_one(const void *qkv_dev, long long ld_qkv, const float *cos_dev, const float *sin_dev, void *cache_dev, long long ld, long long capacity,
                                    const float *attn_mask_dev, long long mask_ld, void *o_dev, int batch, int kv_len, const int *kv_len_dev, int n_q_heads, int n_kv_heads,
                                    int head_dim, float scale, int n_splits, float *scratch_dev, size_t scratch_floats, void *stream)
{
    const unsigned faults = decode_faults(head_dim, n_q_heads, n_kv_heads, ld, kv_len, kv_len_dev, capacity);
    if (!qkv_dev || !cos_dev || !sin_dev || !cache_dev || !attn_mask_dev || !o_dev || !scratch_dev || batch <= 0 || n_splits <= 0 || capacity <= 0 ||
        (faults & (kBadHeads | kBadLength))) {
        ecgb::set_error("ecgb_attn_decode_one: bad argument");
        return ECGB_ERR_INVALID;
    }
    const long long longest = kv_len_dev ? capacity : (long long)kv_len;
    int dev = 0, n_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0) n_cu = 128;
    // (two workgroups of 256 threads and 20 KB of LDS a CU are resident whatever else the kernel needs: the launch's workgroups wait for each other)
    if ((faults & (kBadHeadDim | kBadStride)) || n_splits > 64 || (longest + n_splits - 1) / n_splits > kSplitMaxChunk ||
        (long long)n_splits * n_q_heads * batch > 2ll * n_cu || ld_qkv % 8 || ((uintptr_t)qkv_dev & 15) || ((uintptr_t)cache_dev & 15) ||
        scratch_floats < ecgb_attn_decode_one_scratch_floats(batch, n_q_heads, head_dim, n_splits)) {
        ecgb::set_error("ecgb_attn_decode_one: head_dim 64 / 128 / 256, at most 64 splits of at most 2048 keys, at most two workgroups a CU, scratch of ecgb_attn_decode_one_scratch_floats()");
        return ECGB_ERR_UNSUPPORTED;
    }
    DecodeOneArgs A;
    A.qkv = (const unsigned short *)qkv_dev; A.ld_qkv = ld_qkv; A.cs = cos_dev; A.sn = sin_dev; A.cache = (unsigned short *)cache_dev; A.cap = capacity; A.ld = ld;
    A.mask = attn_mask_dev; A.mask_ld = mask_ld;
    A.stats = scratch_dev;
    A.partial = A.stats + (size_t)batch * n_q_heads * n_splits * 2;
    A.cnt = reinterpret_cast<unsigned *>(A.partial + (size_t)batch * n_q_heads * n_splits * head_dim);
    A.o = (unsigned short *)o_dev; A.len_dev = kv_len_dev; A.len_arg = kv_len; A.Hq = n_q_heads; A.Hkv = n_kv_heads; A.scale = scale;
    const dim3 grid((unsigned)n_splits, (unsigned)n_q_heads, (unsigned)batch);
    with_head_dim(head_dim, [&](auto d) { hipLaunchKernelGGL(attn_decode_one_kernel<d()>, grid, dim3(kSplitThreads), 0, (hipStream_t)stream, A); });
    return launched("attn_decode_one_kernel");
}

extern "C" int ecgb_kv_append(const void *src_dev, long long src_ld, long long col_off, int width, void *cache_dev, long long capacity,
                              int batch, const int *kv_len_dev, void *stream)
{
    if (!src_dev || !cache_dev || !kv_len_dev || width <= 0 || width % 8 || src_ld % 8 || col_off % 8 || batch <= 0) {
        ecgb::set_error("ecgb_kv_append: bad argument");
        return ECGB_ERR_INVALID;
    }
    const int items = batch * (width / 8);
    hipLaunchKernelGGL(kv_append_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned short *)src_dev, src_ld, col_off, width, (unsigned short *)cache_dev, capacity, kv_len_dev, batch);
    return launched("kv_append_kernel");
}
