// sample.hip -- the sampling token choice of generate() in one launch on MI355X (gfx950): temperature, top-k, top-p and the draw, from the bf16 logits as the head GEMM
// leaves them.  The greedy choice has ecgb_argmax_bf16; this is its do_sample counterpart, so that a sampling decode step can be captured once and replayed.
//
// Reference behaviour (vendored transformers 4.46.0.dev0): GenerationMixin._sample (generation/utils.py:3131-3250) with TemperatureLogitsWarper, TopKLogitsWarper,
// TopPLogitsWarper (generation/logits_process.py) in front of `torch.multinomial(softmax(scores), 1)`.  The rule this file implements is written out in
// include/ecgbyte_decoder.h (ecgb_sample_bf16) and restated per token in float64 in tests/sample_ref.py.
//
// Form.  bf16 has 65 536 bit patterns and equal values have equal weights, so nothing is sorted: a row is summarised by an integer count per monotone 16-bit key, and the
// cuts and the draw are found by scans over the keys in descending order (64 keys a "chunk", 1 024 chunks, one per thread):
//   1. one pass over the row counts the drawable entries per key (integer LDS atomics) and finds the largest key;
//   2. an integer scan of the chunk counts gives the top-k cut key -- ties fall out for free, a key is kept or dropped whole;
//   3. count * exp((value - max) / T) per key in float64, summed per chunk by a fixed butterfly and scanned over the chunks in a fixed order, gives Z, the chunk that
//      holds the top-p cut and the chunk that holds the draw; inside such a chunk a wave scans its 64 keys and one lane solves for "how many of this key's entries";
//   4. a second pass over the row finds the j-th entry of the drawn key in id order (ballots over consecutive ids: no prefix sums).
// One workgroup of 1 024 threads per row.  No float atomics anywhere: every float64 sum is formed in a fixed order, so the same inputs give the same token on every launch.
//
// Storage of the counts: LDS.  64 Ki keys x 32 bits is 256 KiB and does not fit the CU's 160 KiB; a table in device memory would cost a zero fill, n atomics that meet in
// L2 and a 256 KiB read per row and launch, and would have to be left clean for the next replay.  So two keys share one LDS word as two 15-bit counts, each with a guard
// bit above it (128 KiB): an add that fills the 15 bits sets the guard instead of carrying into the neighbour; the thread that saw the count at 32 767 takes the guard
// back out and logs the key in a small list ("this key holds 32 768 more").  A key holds count + 32 768 x its entries in the list -- exact for a constant row or a masked
// vocabulary, whose one key holds every entry.  The list has room for 1 024 entries, which covers n <= 2^25.  The scratch in device memory is the flag word alone
// ("a row had nothing to draw"): it is raised and never cleared by the kernel -- the caller reads and clears it -- so a replayed graph needs nothing re-armed.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "tokenizer.hpp"

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) unsigned short;

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kHistWords = 32768;                 // 65 536 keys, two to a word
constexpr int kChunks = 1024;                     // 64 keys each; chunk 0 holds the greatest keys
constexpr int kMaxEvents = 1024;                  // "32 768 more of this key"
constexpr long long kMaxN = (long long)kMaxEvents * 32768;
constexpr size_t kLdsHist = (size_t)kHistWords * 4, kLdsE = (size_t)kChunks * 8, kLdsC = (size_t)kChunks * 4, kLdsEv = (size_t)kMaxEvents * 2;
constexpr size_t kLdsBytes = kLdsHist + kLdsE + kLdsC + kLdsEv;        // 142 KiB: one workgroup per CU
constexpr size_t kScratchBytes = 256;             // word 0: the flag

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's philox.h)
__host__ __device__ inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// monotone in the bf16 value; -1: never drawn (NaN, -inf); -0 is +0.  Drawable keys: 0x0080 (the most negative finite value) .. 0xFF80 (+inf); 0x7FFF stays empty.
__device__ __forceinline__ int sample_key(unsigned short b)
{
    const unsigned u = b, mag = u & 0x7FFFu;
    if (mag > 0x7F80u || u == 0xFF80u) return -1;
    if (mag == 0u) return 0x8000;
    return (u & 0x8000u) ? (int)(0x7FFFu - mag) : (int)(0x8000u | u);
}
__device__ __forceinline__ double key_value(int key)
{
    const unsigned u = key >= 0x8000 ? ((unsigned)key & 0x7FFFu) : (0x8000u | (0x7FFFu - (unsigned)key));
    return (double)__uint_as_float(u << 16);
}

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
// exclusive prefix of v over the workgroup's threads in thread order, and the total: the waves' totals are added in wave order by every thread (a fixed order)
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T *s_tot, T &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_incl_scan(v, lane);
    if (lane == 63) s_tot[wave] = incl;
    __syncthreads();
    T pre = 0, tot = 0;
    for (int w = 0; w < kWaves; ++w) {
        if (w == wave) pre = tot;
        tot += s_tot[w];
    }
    total = tot;
    T ex = __shfl_up(incl, 1, 64);
    if (lane == 0) ex = 0;
    return pre + ex;
}
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

struct SampleArgs {
    const unsigned short *x;
    long long ld;
    int n;
    float temperature;
    int top_k;
    float top_p;
    const unsigned long long *seed;   // [2]: seed, nonce
    const int *step_dev;
    int step;
    const double *u;
    int *flag;
    long long *out;
};

__global__ __launch_bounds__(kThreads) void sample_rows_kernel(SampleArgs A)
{
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned *hist = reinterpret_cast<unsigned *>(smem);
    double *s_E = reinterpret_cast<double *>(smem + kLdsHist);                       // per chunk: its kept weight, then the weight in front of it
    unsigned *s_C = reinterpret_cast<unsigned *>(smem + kLdsHist + kLdsE);           // per chunk: its entries
    unsigned short *s_ev = reinterpret_cast<unsigned short *>(smem + kLdsHist + kLdsE + kLdsC);
    __shared__ unsigned s_nev, s_wcnt[kWaves];
    __shared__ int s_maxkey, s_kchunk, s_kex, s_pchunk, s_dchunk, s_itot[kWaves];
    __shared__ double s_dtot[kWaves];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x, n = A.n;
    const unsigned short *row = A.x + (long long)r * A.ld;

    for (int i = tid; i < kHistWords / 4; i += kThreads) reinterpret_cast<uint4 *>(hist)[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) { s_nev = 0u; s_maxkey = -1; s_kchunk = -1; s_kex = 0; s_pchunk = -1; s_dchunk = -1; }
    __syncthreads();

    // ---- 1. entries per key ------------------------------------------------------------------------
    int kmax = -1;
    auto take = [&](unsigned short b) {
        const int k = sample_key(b);
        if (k < 0) return;
        const unsigned sh = (unsigned)(k & 1) * 16u;
        const unsigned old = atomicAdd(&hist[k >> 1], 1u << sh);
        if (((old >> sh) & 0x7FFFu) == 0x7FFFu) {                 // this add filled the 15 bits and set the guard bit: take it out, log 32 768 of the key
            atomicSub(&hist[k >> 1], 0x8000u << sh);
            const unsigned e = atomicAdd(&s_nev, 1u);
            if (e < (unsigned)kMaxEvents) s_ev[e] = (unsigned short)k;
        }
        kmax = k > kmax ? k : kmax;
    };
    {
        const int head = min(n, (int)(((16 - ((uintptr_t)row & 15)) & 15) / 2));      // elements before the first 16-byte boundary
        for (int i = tid; i < head; i += kThreads) take(row[i]);
        const int body = (n - head) / 8;
        constexpr int U = 8;                                      // 16-byte pieces in flight per thread
        for (int c0 = tid; c0 < body; c0 += kThreads * U) {
            bf16x8 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const bf16x8 *>(row + head + (long long)min(c0 + kThreads * u, body - 1) * 8);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (c0 + kThreads * u < body) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) take((unsigned short)v[u][j]);
                }
            }
        }
        for (int i = head + body * 8 + tid; i < n; i += kThreads) take(row[i]);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) kmax = max(kmax, __shfl_xor(kmax, d, 64));
    if (lane == 0 && kmax >= 0) atomicMax(&s_maxkey, kmax);
    __syncthreads();

    const int maxkey = s_maxkey;
    if (maxkey < 0) {                                             // nothing drawable: token 0 and the flag
        if (tid == 0) { A.out[r] = 0; *A.flag = 1; }
        return;
    }
    const unsigned nev = min(s_nev, (unsigned)kMaxEvents);
    auto key_count = [&](int key) -> unsigned {
        unsigned c = (hist[key >> 1] >> ((unsigned)(key & 1) * 16u)) & 0x7FFFu;
        for (unsigned e = 0; e < nev; ++e) c += (int)s_ev[e] == key ? 32768u : 0u;
        return c;
    };
    // chunk `tid`: keys 65535 - 64 tid - (0 .. 63), the words 32736 - 32 tid + (0 .. 31), read rotated by the thread so that a wave's reads spread over the banks
    unsigned ct = 0;
    {
        const unsigned base = 32736u - 32u * (unsigned)tid;
#pragma unroll 8
        for (int i = 0; i < 32; ++i) {
            const unsigned w = hist[base + ((unsigned)(i + tid) & 31u)];
            ct += (w & 0x7FFFu) + ((w >> 16) & 0x7FFFu);
        }
        for (unsigned e = 0; e < nev; ++e) ct += ((65535u - (unsigned)s_ev[e]) >> 6) == (unsigned)tid ? 32768u : 0u;
    }
    s_C[tid] = ct;

    // ---- 2. top-k: every key >= the key of the k-th entry ---------------------------------------------
    const bool k_on = A.top_k > 0 && A.top_k < n;
    int total;
    const int cex = block_excl_scan<int>((int)ct, s_itot, total);
    if (k_on && cex < A.top_k && A.top_k <= cex + (int)ct) { s_kchunk = tid; s_kex = cex; }      // one thread at most (fewer than k drawable entries: none, all kept)
    __syncthreads();
    int cutkey = 0;
    if (s_kchunk >= 0) {                                          // every wave for itself: the key inside the chunk
        const int key = 65535 - 64 * s_kchunk - lane;
        const int c = (int)key_count(key);
        const int incl = s_kex + wave_incl_scan(c, lane);
        const unsigned long long hit = __ballot(c > 0 && incl - c < A.top_k && A.top_k <= incl);
        if (hit) cutkey = 65535 - 64 * s_kchunk - (__ffsll((long long)hit) - 1);
    }
    const int cutchunk = (65535 - cutkey) >> 6;

    // ---- 3. weights: per chunk, a wave with a key per lane ---------------------------------------------
    const double vmax = key_value(maxkey), T = (double)A.temperature;
    auto weight = [&](int key) -> double { return key == maxkey ? 1.0 : exp((key_value(key) - vmax) / T); };      // (+inf as the maximum: 1, and exp(-inf) = 0 for the rest)
    for (int i = 0; i < kChunks / kWaves; ++i) {
        const int ch = wave + kWaves * i;                         // dealt round the waves: occupied chunks lie next to each other
        double s = 0.0;
        if (s_C[ch] != 0u && ch <= cutchunk) {
            const int key = 65535 - 64 * ch - lane;
            const unsigned c = key_count(key);
            double cw = 0.0;
            if (c != 0u && key >= cutkey) cw = (double)c * weight(key);
            s = wave_sum_f64(cw);
        }
        if (lane == 0) s_E[ch] = s;
    }
    __syncthreads();
    double Z;
    const double E = block_excl_scan<double>(s_E[tid], s_dtot, Z);       // the kept weight ordered before chunk `tid`
    s_E[tid] = E;
    const double pZ = (double)A.top_p * Z;
    const bool has = ct != 0u && tid <= cutchunk;                 // the chunk holds kept entries
    if (has && E < pZ) atomicMax(&s_pchunk, tid);                 // top-p: the last chunk whose first entry is kept holds the cut (the first occupied chunk: E = 0 < pZ)
    __syncthreads();

    // every wave for itself: in that chunk, the last key whose first entry is kept, and how many of its entries (lowest ids) are
    int pkey;
    unsigned pm;
    double Zp;
    {
        const int ch = s_pchunk, key = 65535 - 64 * ch - lane;
        const unsigned c = key_count(key);
        const bool kept = c != 0u && key >= cutkey;
        const double w = kept ? weight(key) : 0.0, cw = kept ? (double)c * w : 0.0;
        const double incl = wave_incl_scan(cw, lane);
        double ex = __shfl_up(incl, 1, 64);
        if (lane == 0) ex = 0.0;
        const double Pb = s_E[ch] + ex;                           // weight ordered before this key's first entry
        const unsigned long long f = __ballot(kept && Pb < pZ);
        const int L = f ? 63 - __clzll((long long)f) : 0;
        unsigned m = c;                                           // entry j of the key is kept iff Pb + j w < pZ
        if (kept && w > 0.0) {
            const double q = (pZ - Pb) / w;
            m = q >= (double)c ? c : (unsigned)ceil(q);
            m = m < 1u ? 1u : m;
            for (int it = 0; it < 4 && m < c && Pb + (double)m * w < pZ; ++it) ++m;
            for (int it = 0; it < 4 && m > 1u && !(Pb + (double)(m - 1u) * w < pZ); ++it) --m;
        }
        pkey = __shfl(key, L, 64);
        pm = __shfl(m, L, 64);
        Zp = __shfl(Pb + (double)m * w, L, 64);                   // the kept weight
    }

    // ---- 4. the draw -------------------------------------------------------------------------------------
    double u;
    if (A.u) {
        u = A.u[r];
    } else {
        const unsigned long long seed = A.seed[0], nonce = A.seed[1];
        const uint32_t ctr[4] = {(uint32_t)r, (uint32_t)(A.step_dev ? *A.step_dev : A.step), (uint32_t)nonce, (uint32_t)(nonce >> 32)};
        const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
        uint32_t o[4];
        philox4x32_10(ctr, key, o);
        u = (double)((((unsigned long long)o[0] << 32) | o[1]) >> 11) * 0x1.0p-53;
    }
    const double target = u * Zp;                                 // the drawn entry: the first kept one whose inclusive weight is > target
    if (has && tid <= s_pchunk && E <= target) atomicMax(&s_dchunk, tid);
    __syncthreads();
    int dkey;
    unsigned dj;
    {
        const int ch = s_dchunk, key = 65535 - 64 * ch - lane;
        unsigned c = key_count(key);
        c = key > pkey ? c : (key == pkey ? pm : 0u);             // kept entries of the key
        const double w = c != 0u ? weight(key) : 0.0, cw = (double)c * w;
        const double incl = wave_incl_scan(cw, lane);
        double ex = __shfl_up(incl, 1, 64);
        if (lane == 0) ex = 0.0;
        const double Pb = s_E[ch] + ex;
        const unsigned long long g = __ballot(c != 0u && Pb <= target);
        const int L = g ? 63 - __clzll((long long)g) : 0;
        unsigned j = c != 0u ? c - 1u : 0u;                       // entry j is drawn iff Pb + j w <= target < Pb + (j + 1) w; past the last one: the last one
        if (c != 0u && w > 0.0) {
            const double q = (target - Pb) / w;
            j = q >= (double)(c - 1u) ? c - 1u : (q > 0.0 ? (unsigned)floor(q) : 0u);
            for (int it = 0; it < 4 && j + 1u < c && Pb + (double)(j + 1u) * w <= target; ++it) ++j;
            for (int it = 0; it < 4 && j > 0u && Pb + (double)j * w > target; ++it) --j;
        }
        dkey = __shfl(key, L, 64);
        dj = __shfl(j, L, 64);
    }

    // ---- 5. entry dj, in id order, of the entries with key dkey: consecutive ids over the lanes, a sixteenth of the row per wave -------------------------------
    const int per = (((n + kWaves - 1) / kWaves) + 63) & ~63;
    const int lo = min(n, wave * per), hi = min(n, lo + per);
    unsigned cnt = 0;
    for (int i0 = lo; i0 < hi; i0 += 64 * 8) {
        unsigned short b[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) b[q] = row[min(i0 + 64 * q + lane, hi - 1)];
#pragma unroll
        for (int q = 0; q < 8; ++q) cnt += (unsigned)__popcll(__ballot(i0 + 64 * q + lane < hi && sample_key(b[q]) == dkey));
    }
    if (lane == 0) s_wcnt[wave] = cnt;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int w = 0; w < kWaves; ++w) {
        if (w == wave) before = all;
        all += s_wcnt[w];
    }
    if (dj >= all) {                                              // (cannot happen: the key holds more than dj entries)
        if (tid == 0) { A.out[r] = 0; *A.flag = 2; }
        return;
    }
    if (before <= dj && dj < before + cnt) {                      // this wave's part holds it
        unsigned seen = before;
        for (int i0 = lo; i0 < hi; i0 += 64) {
            const int i = i0 + lane;
            const unsigned long long mt = __ballot(i < hi && sample_key(row[min(i, hi - 1)]) == dkey);
            const unsigned pc = (unsigned)__popcll(mt);
            if (seen + pc > dj) {
                const unsigned rank = (unsigned)__popcll(mt & ((1ull << lane) - 1ull));
                if (((mt >> lane) & 1ull) && seen + rank == dj) A.out[r] = (long long)i;
                break;
            }
            seen += pc;
        }
    }
}

}  // namespace

extern "C" int ecgb_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    if (!ctr || !key || !out) { ecgb::set_error("ecgb_philox4x32_10: bad argument"); return ECGB_ERR_INVALID; }
    philox4x32_10(ctr, key, out);
    return ECGB_OK;
}

extern "C" size_t ecgb_sample_scratch_bytes(int rows) { return rows > 0 ? kScratchBytes : 0; }

extern "C" int ecgb_sample_bf16(const void *x_dev, long long ld, int rows, int n, float temperature, int top_k, float top_p, const uint64_t *seed_dev,
                                const int *step_dev, int step, const double *u_dev, void *scratch_dev, size_t scratch_bytes, int64_t *out_dev, void *stream)
{
    if (!x_dev || !out_dev || !scratch_dev || (!seed_dev && !u_dev) || rows <= 0 || n <= 0 || ld < n || !(temperature > 0.0f) || std::isinf(temperature) || top_k < 0 ||
        !(top_p > 0.0f && top_p <= 1.0f) || scratch_bytes < ecgb_sample_scratch_bytes(rows)) {
        ecgb::set_error("ecgb_sample_bf16: bad argument");
        return ECGB_ERR_INVALID;
    }
    if ((long long)n > kMaxN) { ecgb::set_error("ecgb_sample_bf16: rows of more than 2^25 entries are not supported"); return ECGB_ERR_UNSUPPORTED; }
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(sample_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e != hipSuccess) { ecgb::set_error(std::string("ecgb_sample_bf16: hipFuncSetAttribute: ") + hipGetErrorString(e)); return ECGB_ERR_HIP; }
    SampleArgs A;
    A.x = (const unsigned short *)x_dev; A.ld = ld; A.n = n; A.temperature = temperature; A.top_k = top_k; A.top_p = top_p;
    A.seed = (const unsigned long long *)seed_dev; A.step_dev = step_dev; A.step = step; A.u = u_dev; A.flag = (int *)scratch_dev; A.out = (long long *)out_dev;
    hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)rows), dim3(kThreads), kLdsBytes, (hipStream_t)stream, A);
    e = hipGetLastError();
    if (e != hipSuccess) { ecgb::set_error(std::string("sample_rows: ") + hipGetErrorString(e)); return ECGB_ERR_HIP; }
    return ECGB_OK;
}
