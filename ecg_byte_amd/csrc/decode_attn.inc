// decode_attn.inc -- the arithmetic of one decode step's attention (one query per head against the KV cache), written ONCE.  The kernels of attention_decode.hip
// (one workgroup a head; keys split over workgroups; RoPE + append + split in one launch) and the grouped kernels of decode.hip (all query heads of a KV group a
// workgroup) are compositions of these routines: the same sums in the same order, so the forms agree bit for bit (tests/test_gpu_decode_fused.py,
// tests/test_gpu_decode_attn_edges.py).  Where the forms differ in WHERE a value lives (cache row or register, scratch or LDS, plain or agent-scope load) the
// routine takes a functor; what workgroups exchange, and how, stays in the kernels.
//   scores   a wave takes keys w, w + NW, ...: its lanes read a key row together (EPL = D / 64 elements each), multiply with the query (registers) and add up
//            across the wave; KU key rows of a wave in flight (memory latency, not bandwidth, is the cost)
//   softmax  (maximum, sum of exponentials) of a key range over the workgroup; over the splits: global maximum, rescaled sum
//   P.V      thread t owns one 16-byte piece of the value rows of its key slice t / (D / 8) (interleaved keys), VU rows in flight; P is cast to bf16 first, as SDPA
//            does; the slices' partial sums meet in LDS, the splits' in split order
#pragma once
#include <hip/hip_runtime.h>

#include "rope_math.hpp"

namespace ecgb_dattn {

using ecgb::bf_bits;
using ecgb::bf_value;
using row8 = ecgb::bf16_row8;

// ---- scores ---------------------------------------------------------------------------------------------------------------------------------------------------
// the raw bits of KU key rows (keys j0, j0 + NW, ...; EPL elements a lane: 8, 4 or 2 bytes) and their mask values.  Past the end (k1): the last key once more
template <int D, int NW, int KU>
__device__ __forceinline__ void load_keys(uint2 (&kr)[KU], float (&mk)[KU], const unsigned short *K, long long ld, const float *mrow, int j0, int k1, int lane)
{
    constexpr int EPL = D / 64;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
        const int j = min(j0 + u * NW, k1 - 1);
        mk[u] = mrow[j];
        const unsigned short *p = K + (long long)j * ld + lane * EPL;
        if constexpr (EPL == 4) kr[u] = *reinterpret_cast<const uint2 *>(p);
        else if constexpr (EPL == 2) { kr[u].x = *reinterpret_cast<const unsigned *>(p); kr[u].y = 0u; }
        else { kr[u].x = p[0]; kr[u].y = 0u; }
    }
}

// this lane's part of q . k for the batch's keys; past the end: whatever the repeated row gives (finish_scores ignores it -- a test here cost attn_decode_one_kernel
// 100 registers).  NEW: key `newest` is taken from registers (kn) -- its cache row is being written by another workgroup
template <int D, int NW, int KU, bool NEW>
__device__ __forceinline__ void dot_keys(float (&part)[KU], const float (&qf)[D / 64], const uint2 (&kr)[KU], const float (&kn)[D / 64], int j0, int newest)
{
    constexpr int EPL = D / 64;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
        if (NEW && j0 + u * NW == newest) {
            part[u] = qf[0] * kn[0];
#pragma unroll
            for (int t = 1; t < EPL; ++t) part[u] += qf[t] * kn[t];
        } else if constexpr (EPL == 4) {
            part[u] = qf[0] * __uint_as_float(kr[u].x << 16) + qf[1] * __uint_as_float(kr[u].x & 0xFFFF0000u) +
                      qf[2] * __uint_as_float(kr[u].y << 16) + qf[3] * __uint_as_float(kr[u].y & 0xFFFF0000u);
        } else if constexpr (EPL == 2) {
            part[u] = qf[0] * __uint_as_float(kr[u].x << 16) + qf[1] * __uint_as_float(kr[u].x & 0xFFFF0000u);
        } else {
            part[u] = qf[0] * bf_value((unsigned short)kr[u].x);
        }
    }
}

// the lanes' parts added across the wave; a masked key scores -inf; store(j, score) by lane 0; the wave's running maximum
template <int NW, int KU, class Store>
__device__ __forceinline__ void finish_scores(float (&part)[KU], const float (&mk)[KU], int j0, int k1, float scale, int lane, float &m, Store store)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
#pragma unroll
        for (int u = 0; u < KU; ++u) part[u] += __shfl_xor(part[u], d, 64);
#pragma unroll
    for (int u = 0; u < KU; ++u) {
        const int j = j0 + u * NW;
        if (j < k1) {
            const float sdot = (mk[u] != 0.f) ? part[u] * scale : -INFINITY;
            if (lane == 0) store(j, sdot);
            m = fmaxf(m, sdot);
        }
    }
}

// ---- softmax statistics ---------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float exp_or_zero(float score, float m) { return (m == -INFINITY) ? 0.f : __expf(score - m); }
__device__ __forceinline__ float inverse_or_zero(float l) { return l > 0.f ? 1.f / l : 0.f; }

template <int NW>
__device__ __forceinline__ float max_of_waves(const float *s_red)
{
    float m = s_red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmaxf(m, s_red[w]);
    return m;
}
template <int NW>
__device__ __forceinline__ float sum_of_waves(const float *s_red)
{
    float l = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) l += s_red[w];
    return l;
}
// this wave's sum of exp(s[i] - m) over i = tid, tid + THREADS, ... < n.  KEEP: the exponentials replace the scores
template <int THREADS, bool KEEP>
__device__ __forceinline__ float exp_sum_wave(float *s, int n, float m, int tid)
{
    float l = 0.f;
    for (int i = tid; i < n; i += THREADS) {
        const float e = exp_or_zero(s[i], m);
        if constexpr (KEEP) s[i] = e;
        l += e;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) l += __shfl_xor(l, d, 64);
    return l;
}
// (maximum, sum of exponentials) of the n scores s[] (LDS) over the workgroup, from the waves' maxima m_wave.  s_red: 2 NW floats.  Two barriers
template <int THREADS, bool KEEP>
__device__ __forceinline__ void workgroup_stats(float m_wave, float *s, int n, float *s_red, int tid, float &m, float &l)
{
    constexpr int NW = THREADS / 64;
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) s_red[wave] = m_wave;
    __syncthreads();
    m = max_of_waves<NW>(s_red);
    l = exp_sum_wave<THREADS, KEEP>(s, n, m, tid);
    if (lane == 0) s_red[NW + wave] = l;
    __syncthreads();
    l = sum_of_waves<NW>(s_red + NW);
}

// the splits' (maximum, sum) pairs st[2 t], st[2 t + 1] -> the maximum over all keys and 1 / (sum of exponentials against it); 0 when no key is visible
__device__ __forceinline__ void merge_splits(const float *st, int n_splits, float &m, float &inv)
{
    m = -INFINITY;
    for (int t = 0; t < n_splits; ++t) m = fmaxf(m, st[2 * t]);
    float l = 0.f;
    for (int t = 0; t < n_splits; ++t) l += (st[2 * t] == -INFINITY) ? 0.f : st[2 * t + 1] * __expf(st[2 * t] - m);
    inv = inverse_or_zero(l);
}

// ---- P.V ------------------------------------------------------------------------------------------------------------------------------------------------------
// this thread's piece of VU value rows (keys j0, j0 + NS, ...; past the end the last key once more: it gets probability 0).  row(j): the piece of key j's row
template <int D, int THREADS, int VU, class Row>
__device__ __forceinline__ void load_values(row8 (&vv)[VU], int j0, int k1, Row row)
{
    constexpr int NS = THREADS / (D / 8);
#pragma unroll
    for (int u = 0; u < VU; ++u) vv[u] = row(min(j0 + u * NS, k1 - 1));
}
// acc += bf16(prob(score(j))) * v_j over the batch.  score(j): what is stored for key j (a load: all of a batch are asked for together); prob: score -> probability
template <int D, int THREADS, int VU, class Score, class Prob>
__device__ __forceinline__ void pv_batch(float (&acc)[8], const row8 (&vv)[VU], int j0, int k1, Score score, Prob prob)
{
    constexpr int NS = THREADS / (D / 8);
    float sc[VU];
#pragma unroll
    for (int u = 0; u < VU; ++u) sc[u] = score(min(j0 + u * NS, k1 - 1));
#pragma unroll
    for (int u = 0; u < VU; ++u) {
        const float pj = (j0 + u * NS < k1) ? bf_value(bf_bits(prob(sc[u]))) : 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] += pj * bf_value(vv[u][t]);
    }
}
// the keys first, first + VU NS, ... < k1 of this thread's slice.  PRELOADED: vv already holds the first batch
template <int D, int THREADS, int VU, bool PRELOADED, class Row, class Score, class Prob>
__device__ __forceinline__ void pv_range(float (&acc)[8], row8 (&vv)[VU], int first, int k1, Row row, Score score, Prob prob)
{
    constexpr int NS = THREADS / (D / 8);
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = 0.f;
    for (int j0 = first; j0 < k1; j0 += VU * NS) {
        if (!PRELOADED || j0 != first) load_values<D, THREADS, VU>(vv, j0, k1, row);
        pv_batch<D, THREADS, VU>(acc, vv, j0, k1, score, prob);
    }
}
// the slices' partial sums through LDS (s_part: NS x D floats, free to be written), added in slice order: output dimension tid (tid < D; 0 elsewhere).  One barrier
template <int D, int THREADS>
__device__ __forceinline__ float slice_sum(const float (&acc)[8], float *s_part, int tid)
{
    constexpr int TPR = D / 8, NS = THREADS / TPR, kUnroll = NS > 32 ? 8 : NS;
    const int piece = tid % TPR, slice = tid / TPR;
#pragma unroll
    for (int t = 0; t < 8; ++t) s_part[slice * D + piece * 8 + t] = acc[t];
    __syncthreads();
    float sum = 0.f;
    if (tid < D) {
#pragma unroll kUnroll
        for (int sl = 0; sl < NS; ++sl) sum += s_part[sl * D + tid];
    }
    return sum;
}
// the splits' partial outputs part(0), part(1), ... added in split order, sixteen loads in flight
template <class Part>
__device__ __forceinline__ float combine_splits(int n_splits, Part part)
{
    float sum = 0.f;
    for (int t0 = 0; t0 < n_splits; t0 += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = part(min(t0 + u, n_splits - 1));
#pragma unroll
        for (int u = 0; u < 16; ++u) if (t0 + u < n_splits) sum += v[u];
    }
    return sum;
}

}  // namespace ecgb_dattn
