// detokenize.hip -- the inverse of the codec on the device: token ids -> symbols / per-symbol values / dequantised signal, and the token histogram.
//
// Reference: tokenizer_utils.py:75-77 decode_text (a Python join over vocab[id]), :22-28 reverse_normalize_all (numpy), the expand_attention loop of the
// interpret run, and analyze_token_distribution's Counter.  Input is what ecgb_encode_hip / ecgb_quantize_encode_hip write: rows of ids, a count per row.
//
// Shape of detokenize_kernel (one template, three payloads; DESIGN.md section 3 has the roofline):
//   * one workgroup of 256 lanes per record; the record's running output offset is the only serial quantity, and it lives in a register.
//   * tokens are taken in CHUNKS of kTokChunk = 1 024 (four consecutive tokens a lane): lengths from the expansion table (8 bytes per id, cache resident), a
//     wave scan plus a carry over the four waves, and the chunk's start offsets and table offsets go to LDS (8 KB).
//   * the output is taken in TILES of kTile = 4 096 positions, laid over the row so that a tile starts on a 16-byte boundary of memory whatever `out_stride` is
//     (position + shift, shift = the row start's misalignment in elements).  Every lane owns kRun = 16 consecutive positions: one binary search in the LDS
//     offsets (10 steps) finds the token of the first, then it walks forward -- a lane never depends on how long the tokens are, so a 300-byte flat-line token
//     and sixteen 1-byte tokens cost the same.  The bytes come out of the expansion table by gather (<= a few hundred KB: L1 / L2).
//   * bytes payload: the lane's 16 bytes ARE one aligned 16-byte store.  float / double payloads: the lane's 16 codes (the byte, or the token's index in the chunk)
//     go to LDS and the workgroup streams the tile out with one aligned 16-byte store per lane (4 floats / 2 doubles), 1 KiB per wave instruction.
//     Only a group cut by the row start, the row end or a chunk boundary is stored element by element.
// No float atomics anywhere: a record has one workgroup, so max |original - rebuilt| and the mismatch count are reduced inside it (shuffles, then four LDS slots).
// The histogram uses integer atomics only (LDS counters per workgroup, flushed once with 64-bit adds).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <string>

#include "tokenizer.hpp"

namespace {

#include "quantizer.inc"

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTokPerLane = 4;
constexpr uint32_t kTokChunk = kThreads * kTokPerLane;   // 1 024 tokens per chunk
constexpr uint32_t kRun = 16;                            // consecutive output positions a lane decodes
constexpr uint32_t kTile = kThreads * kRun;              // 4 096 output positions per tile
constexpr uint32_t kMaxExpansionLen = 1u << 20;          // kTokChunk of them still fit the chunk's 32-bit offsets
constexpr uint32_t kHistLds = 8192;                      // histogram bins a workgroup counts in LDS (32 KB); bins beyond go straight to memory

constexpr int PAYLOAD_BYTES = 0, PAYLOAD_VALUES = 1, PAYLOAD_SIGNAL = 2;
constexpr uint32_t kFlagUnknown = 1u, kFlagCut = 2u, kFlagNotSymbol = 4u;

template <int PAYLOAD> struct Payload;
template <> struct Payload<PAYLOAD_BYTES> { using Out = uint8_t; using Code = uint8_t; };
template <> struct Payload<PAYLOAD_VALUES> { using Out = uint32_t; using Code = uint16_t; };   // fp32 moved as bits: NaN payloads and -0 pass untouched
template <> struct Payload<PAYLOAD_SIGNAL> { using Out = double; using Code = uint8_t; };

struct DetokArgs {
    const uint32_t *ids; size_t ids_stride; const uint32_t *counts;
    const uint32_t *tab; uint32_t n_ids; const uint8_t *bytes;     // expansion table of the handle
    void *out; size_t out_stride;                                 // in elements of the payload
    uint32_t *n_sym; uint32_t *flags;
    const uint32_t *values;                                       // PAYLOAD_VALUES: rows of ids_stride
    double lo, range;                                             // PAYLOAD_SIGNAL: p1 - 0.5, (p99 + 0.5) - (p1 - 0.5)
    const double *original; size_t original_stride;               // PAYLOAD_SIGNAL, may be null
    double *max_abs_diff; uint32_t *n_mismatch;
    QuantParams qp;
};

// the literal operation sequence of normalize_all, for parameters the threshold staircase does not cover (quantize_exact_kernel in encode.hip)
__device__ __forceinline__ uint32_t level_exact(double x, double a, double d)
{
    double c = (x - a) / d;
    if (c < 0.0) c = 0.0;
    if (c > 1.0) c = 1.0;
    double s = floor(c * 26.0);
    if (s > 25.0) s = 25.0;
    return (s == s) ? (uint32_t)s : 0u;
}

template <int PAYLOAD>
__global__ __launch_bounds__(kThreads) void detokenize_kernel(DetokArgs A)
{
    using Out = typename Payload<PAYLOAD>::Out;
    using Code = typename Payload<PAYLOAD>::Code;
    constexpr uint32_t VEC = 16 / sizeof(Out);                    // elements of one 16-byte store
    constexpr uint32_t kCodeWords = kRun * sizeof(Code) / 4;      // 4 or 8
    constexpr bool kStaged = PAYLOAD != PAYLOAD_BYTES;

    __shared__ uint32_t s_start[kTokChunk + 1];                   // chunk-relative start offset of every token; [kTokChunk] = the chunk's length
    __shared__ uint32_t s_src[kTokChunk];                         // offset of the token's expansion in the byte table
    __shared__ __attribute__((aligned(16))) uint32_t s_code[kStaged ? kTile * sizeof(Code) / 4 : 4];
    __shared__ uint32_t s_wsum[kThreads / 64];
    __shared__ uint32_t s_flags;
    __shared__ double s_thr[28];
    __shared__ double s_rmax[kThreads / 64];
    __shared__ uint32_t s_rnan[kThreads / 64], s_rmis[kThreads / 64];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const uint32_t count = A.counts[b];
    const uint32_t n_tok = (uint32_t)((size_t)count < A.ids_stride ? (size_t)count : A.ids_stride);   // tokens past the row were never written
    const uint32_t *ids = A.ids + b * A.ids_stride;
    Out *row = reinterpret_cast<Out *>(A.out) + b * A.out_stride;
    const uint32_t shift = (uint32_t)((reinterpret_cast<uintptr_t>(row) / sizeof(Out)) % VEC);
    const uint64_t cap = A.out_stride;
    const uint2 *tab = reinterpret_cast<const uint2 *>(A.tab);

    if (tid == 0) s_flags = 0;
    if (PAYLOAD == PAYLOAD_SIGNAL && tid < 28) s_thr[tid] = A.qp.thr[tid];
    uint32_t myflags = 0, mism = 0;
    double mx = 0.0;
    bool has_nan = false;
    uint64_t running = 0;                                         // symbols of the tokens before this chunk (not clamped)

    for (uint32_t cb = 0; cb < n_tok; cb += kTokChunk) {
        __syncthreads();                                          // the previous chunk's readers of s_start / s_src are done
        uint32_t len[kTokPerLane], src[kTokPerLane], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kTokPerLane; ++k) {
            const uint32_t t = cb + kTokPerLane * tid + k;
            len[k] = 0; src[k] = 0;
            if (t < n_tok) {
                const uint32_t id = ids[t];
                if (id < A.n_ids) { const uint2 e = tab[id]; src[k] = e.x; len[k] = e.y; }
                if (len[k] == 0) myflags |= kFlagUnknown;
            }
            sum += len[k];
        }
        uint32_t inc = sum;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t v = __shfl_up(inc, d, 64);
            if (lane >= d) inc += v;
        }
        if (lane == 63) s_wsum[wave] = inc;
        __syncthreads();
        uint32_t base = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kThreads / 64; ++w) {
            const uint32_t v = s_wsum[w];
            if (w < wave) base += v;
            total += v;
        }
        uint32_t ex = base + inc - sum;
#pragma unroll
        for (uint32_t k = 0; k < kTokPerLane; ++k) {
            s_start[kTokPerLane * tid + k] = ex;
            s_src[kTokPerLane * tid + k] = src[k];
            ex += len[k];
        }
        if (tid == kThreads - 1) s_start[kTokChunk] = total;
        __syncthreads();

        const uint64_t c_lo = running, c_end = running + total;
        running = c_end;
        if (c_end > cap) myflags |= kFlagCut;
        const uint64_t c_hi = c_end < cap ? c_end : cap;
        if (c_lo >= c_hi) continue;                               // empty chunk, or the row is full: only the flags of the rest are still wanted

        // tile coordinates: q = position + shift, so that q % 16-byte-group == 0 is an aligned address
        const uint64_t lo_q = c_lo + shift, hi_q = c_hi + shift;
        for (uint64_t tq = lo_q / kTile * kTile; tq < hi_q; tq += kTile) {
            const uint64_t g0 = tq + (uint64_t)kRun * tid;
            const uint64_t qa = g0 > lo_q ? g0 : lo_q, qe = g0 + kRun < hi_q ? g0 + kRun : hi_q;
            uint32_t w[kCodeWords];
#pragma unroll
            for (uint32_t k = 0; k < kCodeWords; ++k) w[k] = 0;
            if (qa < qe) {
                uint32_t r = (uint32_t)(qa - lo_q);               // chunk-relative position; < total
                uint32_t lo_i = 1, hi_i = kTokChunk;              // smallest i with s_start[i] > r (s_start[kTokChunk] = total > r); the token is i - 1
                while (lo_i < hi_i) {
                    const uint32_t mid = (lo_i + hi_i) >> 1;
                    if (s_start[mid] > r) hi_i = mid; else lo_i = mid + 1;
                }
                uint32_t t = lo_i - 1;
                uint32_t t_start = s_start[t], t_end = s_start[t + 1];
                const uint8_t *t_bytes = A.bytes + s_src[t];
#pragma unroll
                for (uint32_t j = 0; j < kRun; ++j) {
                    const uint64_t q = g0 + j;
                    if (q >= qa && q < qe) {
                        if (r >= t_end) {
                            do { ++t; t_start = t_end; t_end = s_start[t + 1]; } while (r >= t_end);   // zero-length tokens are stepped over; r < total ends it
                            t_bytes = A.bytes + s_src[t];
                        }
                        const uint32_t code = (PAYLOAD == PAYLOAD_VALUES) ? t : (uint32_t)t_bytes[r - t_start];
                        ++r;
                        if constexpr (sizeof(Code) == 1) w[j / 4] |= code << (8 * (j % 4));
                        else w[j / 2] |= code << (16 * (j % 2));
                    }
                }
                if constexpr (!kStaged) {
                    if (qa == g0 && qe == g0 + kRun) {                                    // the whole run is in range: g0 - shift is a multiple of 16 past an aligned address
                        *reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(row) + (g0 - shift)) = make_uint4(w[0], w[1], w[2], w[3]);
                    } else {
#pragma unroll
                        for (uint32_t j = 0; j < kRun; ++j) {
                            const uint64_t q = g0 + j;
                            if (q >= qa && q < qe) reinterpret_cast<uint8_t *>(row)[q - shift] = (uint8_t)(w[j / 4] >> (8 * (j % 4)));
                        }
                    }
                } else {
                    uint4 *dst = reinterpret_cast<uint4 *>(s_code) + (size_t)tid * (kCodeWords / 4);
                    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
                    if constexpr (kCodeWords == 8) dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
                }
            }
            if constexpr (kStaged) {
                __syncthreads();
                const Code *code = reinterpret_cast<const Code *>(s_code);
                const uint32_t v_lo = (uint32_t)((tq > lo_q ? tq : lo_q) - tq), v_hi = (uint32_t)((tq + kTile < hi_q ? tq + kTile : hi_q) - tq);
                for (uint32_t g = v_lo / VEC + tid; g * VEC < v_hi; g += kThreads) {
                    Out vals[VEC];
                    bool full = true;
#pragma unroll
                    for (uint32_t e = 0; e < VEC; ++e) {
                        const uint32_t off = g * VEC + e;
                        const bool valid = off >= v_lo && off < v_hi;
                        full = full && valid;
                        vals[e] = Out();
                        if (!valid) continue;
                        const uint32_t c = code[off];
                        if constexpr (PAYLOAD == PAYLOAD_VALUES) {
                            vals[e] = A.values[b * A.ids_stride + cb + c];
                        } else {
                            const uint32_t idx = c - (uint32_t)'a';
                            double v;
                            if (idx < ECGB_ALPHABET) {
                                const double nrm = (double)idx / 25.0;                    // reverse_normalize_all, one IEEE operation at a time (-ffp-contract=off)
                                const double scaled = nrm * A.range;
                                v = scaled + A.lo;
                            } else {
                                v = __longlong_as_double(0x7FF8000000000000ll);
                                myflags |= kFlagNotSymbol;
                            }
                            vals[e] = v;
                            const uint64_t pos = tq + off - shift;
                            if (A.original && pos < A.original_stride) {
                                const double o = A.original[b * A.original_stride + pos];
                                const double d = fabs(o - v);
                                if (d != d) has_nan = true;                               // np.max: any NaN makes the maximum NaN -- kept as a flag, so the order cannot matter
                                else if (d > mx) mx = d;
                                const uint32_t lvl = A.qp.use_thresholds ? level_from_thresholds(o, A.qp.a, A.qp.scale, s_thr) : level_exact(o, A.qp.a, A.qp.d);
                                if (lvl != idx) ++mism;
                            }
                        }
                    }
                    if (full) {                                                           // an aligned 16-byte group, all of it in range
                        uint4 pack;
                        memcpy(&pack, vals, 16);
                        *reinterpret_cast<uint4 *>(row + (tq + (uint64_t)g * VEC - shift)) = pack;
                    } else {
#pragma unroll
                        for (uint32_t e = 0; e < VEC; ++e) {
                            const uint32_t off = g * VEC + e;
                            if (off >= v_lo && off < v_hi) row[tq + off - shift] = vals[e];
                        }
                    }
                }
                __syncthreads();                                                          // s_code is rewritten by the next tile
            }
        }
    }

    if (myflags) atomicOr(&s_flags, myflags);
    if (PAYLOAD == PAYLOAD_SIGNAL && A.original) {
#pragma unroll
        for (uint32_t d = 32; d >= 1; d >>= 1) {
            const double o = __shfl_xor(mx, d, 64);
            if (o > mx) mx = o;
            mism += __shfl_xor(mism, d, 64);
        }
        const bool any_nan = __any(has_nan);
        if (lane == 0) { s_rmax[wave] = mx; s_rnan[wave] = any_nan ? 1u : 0u; s_rmis[wave] = mism; }
    }
    __syncthreads();
    if (tid == 0) {
        A.n_sym[b] = (uint32_t)(running < cap ? running : cap);
        A.flags[b] = s_flags;
        if (PAYLOAD == PAYLOAD_SIGNAL && A.original) {
            double m = 0.0;
            uint32_t nan = 0, mis = 0;
            for (uint32_t w = 0; w < kThreads / 64; ++w) {
                if (s_rmax[w] > m) m = s_rmax[w];
                nan |= s_rnan[w];
                mis += s_rmis[w];
            }
            A.max_abs_diff[b] = nan ? __longlong_as_double(0x7FF8000000000000ll) : m;
            A.n_mismatch[b] = mis;
        }
    }
}

// Count of every id over the valid tokens of all records.  A workgroup counts ids below kHistLds in LDS (32-bit counters, flushed with 64-bit adds before they could
// wrap) and adds the rest to memory directly; ids >= n_bins are counted in a register and added to *overflow once per wave.  Integer adds only: the same bits every run.
__global__ __launch_bounds__(kThreads) void token_histogram_kernel(const uint32_t *__restrict__ ids, size_t ids_stride, const uint32_t *__restrict__ counts,
                                                                   size_t batch, unsigned long long *hist, uint32_t n_bins, unsigned long long *overflow)
{
    __shared__ uint32_t s_h[kHistLds];
    const uint32_t tid = threadIdx.x;
    const uint32_t n_lds = n_bins < kHistLds ? n_bins : kHistLds;
    for (uint32_t i = tid; i < n_lds; i += kThreads) s_h[i] = 0;
    __syncthreads();
    unsigned long long over = 0, held = 0;      // held: tokens counted since the last flush (uniform)
    for (size_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const uint32_t count = counts[b];
        const uint32_t n = (uint32_t)((size_t)count < ids_stride ? (size_t)count : ids_stride);
        if (held + n > 0xFFFFFFFFull) {
            __syncthreads();
            for (uint32_t i = tid; i < n_lds; i += kThreads) {
                const uint32_t v = s_h[i];
                if (v) atomicAdd(&hist[i], (unsigned long long)v);
                s_h[i] = 0;
            }
            __syncthreads();
            held = 0;
        }
        held += n;
        const uint32_t *row = ids + b * ids_stride;
        for (uint32_t t = tid; t < n; t += kThreads) {
            const uint32_t id = row[t];
            if (id < n_lds) atomicAdd(&s_h[id], 1u);
            else if (id < n_bins) atomicAdd(&hist[id], 1ull);
            else ++over;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < n_lds; i += kThreads) {
        const uint32_t v = s_h[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) over += __shfl_xor(over, d, 64);
    if ((tid & 63u) == 0 && over) atomicAdd(overflow, over);
}

int check_hip(hipError_t e, const char *what)
{
    if (e == hipSuccess) return ECGB_OK;
    ecgb::set_error(std::string(what) + ": " + hipGetErrorString(e));
    return ECGB_ERR_HIP;
}

int check_detok(const ecgb_tokenizer *tok, const void *ids, size_t ids_stride, const void *counts, size_t batch, const void *out, size_t out_stride,
                size_t elem, const void *n_sym, const void *flags, const char *who)
{
    if (!tok || !ids || !counts || !out || !n_sym || !flags || ids_stride == 0 || out_stride == 0) {
        ecgb::set_error(std::string(who) + ": NULL or zero-sized argument");
        return ECGB_ERR_INVALID;
    }
    if (!tok->exp_built) {
        ecgb::set_error(std::string(who) + ": the handle has no expansion table (a token id of 2^22 or more)");
        return ECGB_ERR_UNSUPPORTED;
    }
    if (!tok->exp_tab_dev) {
        ecgb::set_error(std::string(who) + ": tokenizer handle has no device copy (no GPU at creation)");
        return ECGB_ERR_NODEVICE;
    }
    if (tok->exp_max_len > kMaxExpansionLen || ids_stride >= 0x7FFF0000ull || out_stride > 0xFFFFFFFFull || batch >= 0x7FFFFFFFull) {
        ecgb::set_error(std::string(who) + ": an expansion longer than 2^20 bytes, a row of 2^31 or more ids or 2^32 or more outputs, or a batch too large");
        return ECGB_ERR_UNSUPPORTED;
    }
    if (reinterpret_cast<uintptr_t>(out) % elem) {
        ecgb::set_error(std::string(who) + ": output pointer not aligned to its element size");
        return ECGB_ERR_INVALID;
    }
    return ECGB_OK;
}

DetokArgs base_args(const ecgb_tokenizer *tok, const uint32_t *ids, size_t ids_stride, const uint32_t *counts, void *out, size_t out_stride, uint32_t *n_sym,
                    uint32_t *flags)
{
    DetokArgs A;
    std::memset(&A, 0, sizeof(A));
    A.ids = ids; A.ids_stride = ids_stride; A.counts = counts;
    A.tab = tok->exp_tab_dev; A.n_ids = (uint32_t)(tok->exp_tab.size() / 2); A.bytes = tok->exp_bytes_dev;
    A.out = out; A.out_stride = out_stride; A.n_sym = n_sym; A.flags = flags;
    return A;
}

template <int PAYLOAD>
int launch_detok(const DetokArgs &A, size_t batch, void *stream, const char *what)
{
    hipLaunchKernelGGL(detokenize_kernel<PAYLOAD>, dim3((unsigned)batch), dim3(kThreads), 0, (hipStream_t)stream, A);
    return check_hip(hipGetLastError(), what);
}

}  // namespace

extern "C" void ecgb_detokenize_tile(uint32_t *tokens_per_chunk, uint32_t *symbols_per_tile)
{
    if (tokens_per_chunk) *tokens_per_chunk = kTokChunk;
    if (symbols_per_tile) *symbols_per_tile = kTile;
}

extern "C" int ecgb_detokenize_hip(const ecgb_tokenizer *tok, const uint32_t *ids_dev, size_t ids_stride, const uint32_t *counts_dev, size_t batch,
                                   uint8_t *out_dev, size_t out_stride, uint32_t *n_sym_dev, uint32_t *flags_dev, void *stream)
{
    if (batch == 0) return ECGB_OK;
    const int rc = check_detok(tok, ids_dev, ids_stride, counts_dev, batch, out_dev, out_stride, 1, n_sym_dev, flags_dev, "ecgb_detokenize_hip");
    if (rc) return rc;
    return launch_detok<PAYLOAD_BYTES>(base_args(tok, ids_dev, ids_stride, counts_dev, out_dev, out_stride, n_sym_dev, flags_dev), batch, stream,
                                       "detokenize_kernel<bytes> launch");
}

extern "C" int ecgb_detokenize_values_f32_hip(const ecgb_tokenizer *tok, const uint32_t *ids_dev, size_t ids_stride, const uint32_t *counts_dev, size_t batch,
                                              const float *values_dev, float *out_dev, size_t out_stride, uint32_t *n_sym_dev, uint32_t *flags_dev,
                                              void *stream)
{
    if (batch == 0) return ECGB_OK;
    const int rc = check_detok(tok, ids_dev, ids_stride, counts_dev, batch, out_dev, out_stride, 4, n_sym_dev, flags_dev, "ecgb_detokenize_values_f32_hip");
    if (rc) return rc;
    if (!values_dev) { ecgb::set_error("ecgb_detokenize_values_f32_hip: NULL values"); return ECGB_ERR_INVALID; }
    DetokArgs A = base_args(tok, ids_dev, ids_stride, counts_dev, out_dev, out_stride, n_sym_dev, flags_dev);
    A.values = reinterpret_cast<const uint32_t *>(values_dev);
    return launch_detok<PAYLOAD_VALUES>(A, batch, stream, "detokenize_kernel<values> launch");
}

extern "C" int ecgb_detokenize_signal_f64_hip(const ecgb_tokenizer *tok, const uint32_t *ids_dev, size_t ids_stride, const uint32_t *counts_dev, size_t batch,
                                              double percentile_1, double percentile_99, double *out_dev, size_t out_stride, uint32_t *n_sym_dev,
                                              uint32_t *flags_dev, const double *original_dev, size_t original_stride, double *max_abs_diff_dev,
                                              uint32_t *n_mismatch_dev, void *stream)
{
    if (batch == 0) return ECGB_OK;
    const int rc = check_detok(tok, ids_dev, ids_stride, counts_dev, batch, out_dev, out_stride, 8, n_sym_dev, flags_dev, "ecgb_detokenize_signal_f64_hip");
    if (rc) return rc;
    if (original_dev && (!max_abs_diff_dev || !n_mismatch_dev || original_stride == 0)) {
        ecgb::set_error("ecgb_detokenize_signal_f64_hip: `original` given without max_abs_diff / n_mismatch / its row stride");
        return ECGB_ERR_INVALID;
    }
    DetokArgs A = base_args(tok, ids_dev, ids_stride, counts_dev, out_dev, out_stride, n_sym_dev, flags_dev);
    const double lo = percentile_1 - 0.5, hi = percentile_99 + 0.5;     // tokenizer_utils.py:23-24
    A.lo = lo;
    A.range = hi - lo;
    A.original = original_dev; A.original_stride = original_stride;
    A.max_abs_diff = max_abs_diff_dev; A.n_mismatch = n_mismatch_dev;
    if (original_dev) A.qp = make_quant_params(percentile_1, percentile_99);
    return launch_detok<PAYLOAD_SIGNAL>(A, batch, stream, "detokenize_kernel<signal> launch");
}

extern "C" int ecgb_token_histogram_hip(const uint32_t *ids_dev, size_t ids_stride, const uint32_t *counts_dev, size_t batch, uint64_t *hist_dev,
                                        size_t n_bins, uint64_t *overflow_dev, void *stream)
{
    if (!hist_dev || !overflow_dev || n_bins == 0 || (batch && (!ids_dev || !counts_dev || ids_stride == 0))) {
        ecgb::set_error("ecgb_token_histogram_hip: NULL or zero-sized argument");
        return ECGB_ERR_INVALID;
    }
    if (n_bins > 0xFFFFFFFFull || ids_stride >= 0x7FFF0000ull) {
        ecgb::set_error("ecgb_token_histogram_hip: 2^32 or more bins, or rows of 2^31 or more ids");
        return ECGB_ERR_UNSUPPORTED;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        ecgb::set_error("ecgb_token_histogram_hip: no GPU");
        return ECGB_ERR_NODEVICE;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc = check_hip(hipMemsetAsync(hist_dev, 0, n_bins * sizeof(uint64_t), st), "hipMemsetAsync(hist)");
    if (rc == ECGB_OK) rc = check_hip(hipMemsetAsync(overflow_dev, 0, sizeof(uint64_t), st), "hipMemsetAsync(overflow)");
    if (rc || batch == 0) return rc;
    const unsigned grid = (unsigned)(batch < 1024 ? batch : 1024);
    hipLaunchKernelGGL(token_histogram_kernel, dim3(grid), dim3(kThreads), 0, st, ids_dev, ids_stride, counts_dev, batch,
                       reinterpret_cast<unsigned long long *>(hist_dev), (uint32_t)n_bins, reinterpret_cast<unsigned long long *>(overflow_dev));
    return check_hip(hipGetLastError(), "token_histogram_kernel launch");
}
