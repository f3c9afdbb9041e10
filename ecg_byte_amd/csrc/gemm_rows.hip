// gemm_rows.hip -- the weight-streaming MFMA GEMM of a batched decode step: 9 to 64 activation rows against a whole weight matrix.
//
//   C[M,N] = alpha * (A[M,K] . B[N,K]^T + A2[M,K2] . B2[N,K2]^T)          8 < M <= 64, K and K2 multiples of 64
//
// The product is bound by the one pass over B, so the kernel is built around that stream:
//   * a wave owns 16 output columns (16 rows of B) and every row of A.  Its B fragments go global -> VGPRs with 16-byte non-temporal loads and are used once:
//     no LDS round trip.  With B as the MFMA's A operand (v_mfma_f32_16x16x32_bf16, D[n][m]) a lane ends up with four consecutive columns of one output row,
//     which leave as one 8-byte store.
//   * the small A is re-read by every column block: it goes through LDS, a chunk of 256 k at a time, fetched as whole 512-byte row pieces and read back as
//     fragments with ds_read_b128 (rows padded by 16 bytes so that the 16 rows of a fragment start on different banks).
//   * a workgroup is four waves = 64 columns over one K slice.  Wide matrices (256 column blocks or more) take K whole and store bf16 (or act(gate) * up) directly.
//     Narrower ones cut K into S slices of whole chunks so that about 512 workgroups stream at once; slice s leaves its fp32 partial in slab s of the caller's
//     scratch and a second launch adds the slabs in slice order (no atomics, no waiting between workgroups): the same inputs give the same bits on every launch.
//   * S depends on (N, K) alone and the second pair always rides behind the last slice, so the GLU form (gate and up rows of the SAME columns in one workgroup:
//     waves 0-1 gate, waves 2-3 up) sums in the order of the plain form on [gate; up] and gives the bits of that followed by ecgb_glu_fwd.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "glu_math.hpp"
#include "tokenizer.hpp"

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u16x4 = __attribute__((ext_vector_type(4))) unsigned short;

constexpr int KC = 256;                 // k per LDS chunk of A
constexpr int ROWB = KC * 2 + 16;       // bytes per LDS row: 512 of data and one 16-byte slot of padding
constexpr int COLS_WG = 64;             // rows of B per workgroup (GLU: 32 gate + the 32 up rows of the same columns)
constexpr int TARGET_WGS = 512;         // workgroups a narrow matrix is cut into (two per CU)

struct RowsArgs {
    const unsigned short *A, *B, *A2, *B2;
    long long lda, ldb, lda2, ldb2;
    int M, N, K, K2;                    // N: rows of B (GLU: 2 * inter)
    float alpha;
    unsigned short *C;                  // [M, N], or H [M, inter] in the GLU form
    long long ldc;
    float *slabs;                       // S > 1: slab s = [M, slab_cols] fp32 at slabs + s * M * slab_cols
    int slab_cols;                      // plain: columns as in C; GLU: gate column j at j, up column j at slab_cols / 2 + j
    int S;
    int inter;                          // GLU form: columns of H, else 0
    int gelu;
};

__device__ __forceinline__ unsigned short f2bf_rn(float f)
{
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float bf2f(unsigned short u) { return __uint_as_float((unsigned)u << 16); }

// act(gate) * up on values already rounded to bf16: the arithmetic of ecgb_glu_fwd
__device__ __forceinline__ unsigned short glu_bits(unsigned short g16, unsigned short u16, int gelu)
{
    const float g = bf2f(g16);
    const float a = bf2f(f2bf_rn(gelu ? ecgb::glu_act<true>(g) : ecgb::glu_act<false>(g)));
    return f2bf_rn(a * bf2f(u16));
}

// Four consecutive columns of one output row: one 8-byte store where the row allows it.
__device__ __forceinline__ void store_quad(unsigned short *row, long long ld, int col, int ncols, u16x4 v)
{
    if (col + 3 < ncols && (ld & 3) == 0 && ((uintptr_t)row & 7) == 0) {
        *reinterpret_cast<u16x4 *>(row + col) = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (col + j < ncols) row[col + j] = v[j];
}

// STEPS * 64 k of one operand pair: X [M, ..] through LDS, the wave's 16 rows of W straight to registers.  wp = the lane's row of W + 8 * (lane >> 4).
template <int MT, int STEPS>
__device__ __forceinline__ void rows_chunk(const unsigned short *X, long long ldx, int M, const unsigned short *wp, int k0, unsigned char *lds, f32x4 (&acc)[MT])
{
    constexpr int PIECES = MT * 16 * STEPS * 8;           // 16-byte pieces of the X chunk, STEPS * 8 a row
    constexpr int NI = (PIECES + 255) / 256;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
    bf16x8 xr[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int p = i * 256 + tid;
        if (PIECES % 256 == 0 || p < PIECES) {
            const int row = p / (STEPS * 8), c = p % (STEPS * 8);
            const int src = row < M ? row : M - 1;        // rows past M feed output rows that are never stored
            xr[i] = *reinterpret_cast<const bf16x8 *>(X + (long long)src * ldx + k0 + c * 8);
        }
    }
    bf16x8 w[STEPS][2];
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
        for (int h = 0; h < 2; ++h) w[s][h] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8 *>(wp + k0 + s * 64 + h * 32));
    __syncthreads();                                      // the previous chunk's fragments have been read
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int p = i * 256 + tid;
        if (PIECES % 256 == 0 || p < PIECES) {
            const int row = p / (STEPS * 8), c = p % (STEPS * 8);
            *reinterpret_cast<bf16x8 *>(lds + row * ROWB + c * 16) = xr[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const bf16x8 xf = *reinterpret_cast<const bf16x8 *>(lds + (mt * 16 + r) * ROWB + (s * 64 + h * 32 + q * 8) * 2);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[s][h], xf, acc[mt], 0, 0, 0);      // D[n = 4 q + reg][m = r]
            }
}

template <int MT, bool GLU>
__global__ __launch_bounds__(256) void gemm_rows_kernel(RowsArgs G)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[MT * 16 * ROWB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int part = GLU ? wave >> 1 : 0;                                        // GLU: 0 gate, 1 up
    const int ncols = GLU ? G.inter : G.N;                                       // columns of a part
    const int col0 = GLU ? blockIdx.x * (COLS_WG / 2) + (wave & 1) * 16 : blockIdx.x * COLS_WG + wave * 16;
    const int wr = col0 + r < ncols ? col0 + r : ncols - 1;                      // rows of B past the end feed columns that are never stored
    const long long brow = (long long)part * ncols + wr;

    // the slice's 64-k steps: whole chunks of four, S slices over the chunks
    const int steps = G.K / 64, chunks = (steps + 3) / 4, s = blockIdx.y;
    const int c_begin = (int)((long long)s * chunks / G.S), c_end = (int)((long long)(s + 1) * chunks / G.S);
    const int st_begin = c_begin * 4, st_end = min(c_end * 4, steps);

    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const unsigned short *wp = G.B + brow * G.ldb + q * 8;
    int st = st_begin;
    for (; st + 4 <= st_end; st += 4) rows_chunk<MT, 4>(G.A, G.lda, G.M, wp, st * 64, lds, acc);
    for (; st < st_end; ++st) rows_chunk<MT, 1>(G.A, G.lda, G.M, wp, st * 64, lds, acc);
    if (G.K2 > 0 && s == G.S - 1) {
        const unsigned short *wp2 = G.B2 + brow * G.ldb2 + q * 8;
        for (int k = 0; k < G.K2; k += 64) rows_chunk<MT, 1>(G.A2, G.lda2, G.M, wp2, k, lds, acc);
    }

    const int col = col0 + q * 4;                         // the lane's four columns inside its part
    if (G.S > 1) {                                        // fp32 partials; ecgb's reduce launch finishes them
        float *slab = G.slabs + (long long)s * G.M * G.slab_cols + (GLU ? part * (G.slab_cols / 2) : 0);
        if (col < ncols) {                                // slab rows are padded to whole quads
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int m = mt * 16 + r;
                if (m < G.M) *reinterpret_cast<f32x4 *>(slab + (long long)m * G.slab_cols + col) = acc[mt];
            }
        }
        return;
    }
    u16x4 v[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[mt][j] = f2bf_rn(G.alpha * acc[mt][j]);
    if constexpr (!GLU) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = mt * 16 + r;
            if (m < G.M && col < ncols) store_quad(G.C + (long long)m * G.ldc, G.ldc, col, ncols, v[mt]);
        }
    } else {
        // the up waves hand their quads to the gate waves of the same columns through LDS
        __syncthreads();                                  // the last chunk's fragments have been read
        u16x4 *xch = reinterpret_cast<u16x4 *>(lds);      // [wave & 1][mt][lane]
        if (part == 1) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) xch[((wave & 1) * MT + mt) * 64 + lane] = v[mt];
        }
        __syncthreads();
        if (part == 0) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const u16x4 u = xch[((wave & 1) * MT + mt) * 64 + lane];
                u16x4 h;
#pragma unroll
                for (int j = 0; j < 4; ++j) h[j] = glu_bits(v[mt][j], u[j], G.gelu);
                const int m = mt * 16 + r;
                if (m < G.M && col < ncols) store_quad(G.C + (long long)m * G.ldc, G.ldc, col, ncols, h);
            }
        }
    }
}

// The slabs of a sliced product, added in slice order: one thread per output quad.
template <bool GLU>
__global__ __launch_bounds__(256) void gemm_rows_reduce_kernel(RowsArgs G)
{
    const int ncols = GLU ? G.inter : G.N;
    const int quads = (ncols + 3) / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)G.M * quads) return;
    const int m = (int)(i / quads), col = (int)(i % quads) * 4;
    const long long slab_stride = (long long)G.M * G.slab_cols;
    const float *p = G.slabs + (long long)m * G.slab_cols + col;
    f32x4 a = *reinterpret_cast<const f32x4 *>(p), b = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (GLU) b = *reinterpret_cast<const f32x4 *>(p + G.slab_cols / 2);
    for (int s = 1; s < G.S; ++s) {
        a += *reinterpret_cast<const f32x4 *>(p + s * slab_stride);
        if (GLU) b += *reinterpret_cast<const f32x4 *>(p + s * slab_stride + G.slab_cols / 2);
    }
    u16x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned short g = f2bf_rn(G.alpha * a[j]);
        v[j] = GLU ? glu_bits(g, f2bf_rn(G.alpha * b[j]), G.gelu) : g;
    }
    store_quad(G.C + (long long)m * G.ldc, G.ldc, col, ncols, v);
}

// K slices of a product with N rows of B: a function of (N, K) alone (see the head of the file)
int rows_slices(int N, int K)
{
    const int blocks = (N + COLS_WG - 1) / COLS_WG, chunks = (K / 64 + 3) / 4;
    if (blocks >= TARGET_WGS / 2) return 1;
    const int S = (TARGET_WGS + blocks - 1) / blocks;
    return S < chunks ? S : chunks;
}
int rows_slab_cols(int N) { return (N + 7) / 8 * 8 + 8; }      // GLU: two halves, each holding inter rounded up to a quad

bool rows_domain(int M, int K, int K2) { return M > 8 && M <= 64 && K % 64 == 0 && K2 % 64 == 0; }

template <bool GLU>
int rows_launch(RowsArgs &G, void *scratch_dev, size_t scratch_bytes, void *stream, const char *who)
{
    G.S = rows_slices(G.N, G.K);
    G.slab_cols = rows_slab_cols(G.N);
    G.slabs = (float *)scratch_dev;
    if (G.S > 1) {
        const size_t need = (size_t)G.S * G.M * G.slab_cols * sizeof(float);
        if (!scratch_dev || scratch_bytes < need || ((uintptr_t)scratch_dev & 15)) {
            ecgb::set_error(std::string(who) + ": scratch of " + std::to_string(need) + " bytes (16-byte aligned) needed, see ecgb_gemm_nt_rows_scratch_bytes");
            return ECGB_ERR_INVALID;
        }
    }
    const dim3 grid((G.N + COLS_WG - 1) / COLS_WG, G.S);
    const int MT = (G.M + 15) / 16;
    switch (MT) {
    case 1: hipLaunchKernelGGL((gemm_rows_kernel<1, GLU>), grid, dim3(256), 0, (hipStream_t)stream, G); break;
    case 2: hipLaunchKernelGGL((gemm_rows_kernel<2, GLU>), grid, dim3(256), 0, (hipStream_t)stream, G); break;
    case 3: hipLaunchKernelGGL((gemm_rows_kernel<3, GLU>), grid, dim3(256), 0, (hipStream_t)stream, G); break;
    default: hipLaunchKernelGGL((gemm_rows_kernel<4, GLU>), grid, dim3(256), 0, (hipStream_t)stream, G); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && G.S > 1) {
        const int ncols = GLU ? G.inter : G.N;
        const long long threads = (long long)G.M * ((ncols + 3) / 4);
        hipLaunchKernelGGL(gemm_rows_reduce_kernel<GLU>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G);
        e = hipGetLastError();
    }
    if (e == hipSuccess) return ECGB_OK;
    ecgb::set_error(std::string(who) + ": " + hipGetErrorString(e));
    return ECGB_ERR_HIP;
}

// the checks both entry points share; 0 = go on
int rows_check(const char *who, const void *a, long long lda, const void *b, long long ldb, const void *a2, long long lda2, const void *b2, long long ldb2, int K2,
               const void *out, int M, int N, int K)
{
    if (!a || !b || !out || M <= 0 || N <= 0 || K <= 0 || K2 < 0 || (K2 > 0 && (!a2 || !b2))) {
        ecgb::set_error(std::string(who) + ": bad argument");
        return ECGB_ERR_INVALID;
    }
    bool ok = rows_domain(M, K, K2) && lda % 8 == 0 && ldb % 8 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
    if (K2 > 0) ok = ok && lda2 % 8 == 0 && ldb2 % 8 == 0 && (((uintptr_t)a2 | (uintptr_t)b2) & 15) == 0;
    if (!ok) {
        ecgb::set_error(std::string(who) + ": 8 < M <= 64, K and K2 multiples of 64, operands 16-byte aligned with strides % 8 == 0");
        return ECGB_ERR_UNSUPPORTED;
    }
    return ECGB_OK;
}

}  // namespace

extern "C" size_t ecgb_gemm_nt_rows_scratch_bytes(int M, int N, int K)
{
    if (M <= 0 || N <= 0 || K < 64) return 0;
    const int S = rows_slices(N, K);
    return S > 1 ? (size_t)S * M * rows_slab_cols(N) * sizeof(float) : 0;
}

extern "C" int ecgb_gemm_nt_rows_bf16(const void *a_dev, long long lda, const void *b_dev, long long ldb, const void *a2_dev, long long lda2, const void *b2_dev,
                                      long long ldb2, int K2, void *c_dev, long long ldc, int M, int N, int K, float alpha, void *scratch_dev, size_t scratch_bytes,
                                      void *stream)
{
    const char *who = "ecgb_gemm_nt_rows_bf16";
    if (const int rc = rows_check(who, a_dev, lda, b_dev, ldb, a2_dev, lda2, b2_dev, ldb2, K2, c_dev, M, N, K)) return rc;
    if (ldc < N) { ecgb::set_error(std::string(who) + ": ldc < N"); return ECGB_ERR_INVALID; }
    RowsArgs G{};
    G.A = (const unsigned short *)a_dev; G.B = (const unsigned short *)b_dev; G.A2 = (const unsigned short *)a2_dev; G.B2 = (const unsigned short *)b2_dev;
    G.lda = lda; G.ldb = ldb; G.lda2 = lda2; G.ldb2 = ldb2;
    G.M = M; G.N = N; G.K = K; G.K2 = K2; G.alpha = alpha;
    G.C = (unsigned short *)c_dev; G.ldc = ldc;
    return rows_launch<false>(G, scratch_dev, scratch_bytes, stream, who);
}

extern "C" int ecgb_gemm_nt_rows_glu_bf16(const void *a_dev, long long lda, const void *b_dev, long long ldb, const void *a2_dev, long long lda2, const void *b2_dev,
                                          long long ldb2, int K2, void *h_dev, long long ldh, int M, int inter, int K, float alpha, int gelu_tanh,
                                          void *scratch_dev, size_t scratch_bytes, void *stream)
{
    const char *who = "ecgb_gemm_nt_rows_glu_bf16";
    if (inter > (1 << 29)) { ecgb::set_error(std::string(who) + ": bad argument"); return ECGB_ERR_INVALID; }
    if (const int rc = rows_check(who, a_dev, lda, b_dev, ldb, a2_dev, lda2, b2_dev, ldb2, K2, h_dev, M, inter, K)) return rc;
    if (ldh < inter) { ecgb::set_error(std::string(who) + ": ldh < inter"); return ECGB_ERR_INVALID; }
    RowsArgs G{};
    G.A = (const unsigned short *)a_dev; G.B = (const unsigned short *)b_dev; G.A2 = (const unsigned short *)a2_dev; G.B2 = (const unsigned short *)b2_dev;
    G.lda = lda; G.ldb = ldb; G.lda2 = lda2; G.ldb2 = ldb2;
    G.M = M; G.N = 2 * inter; G.K = K; G.K2 = K2; G.alpha = alpha;
    G.C = (unsigned short *)h_dev; G.ldc = ldh;
    G.inter = inter; G.gelu = gelu_tanh;
    return rows_launch<true>(G, scratch_dev, scratch_bytes, stream, who);
}
