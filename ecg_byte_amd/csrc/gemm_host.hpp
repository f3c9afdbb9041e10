// Host side shared by gemm.hip and gemm_w4.hip: the CU count of the current device, the one kernel-launch sequence, and the four-wave kernel's interface towards
// gemm.hip's dispatch.  No device code.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "tokenizer.hpp"

namespace ecgb {

// CUs of the current device: looked up per device, cached per device (one value for the process would be wrong on a second GPU)
inline int device_cus()
{
    static int cached[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!cached[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}

// One kernel launch: the dynamic-LDS attribute (per device, so set on every launch -- a cached flag would be wrong on a second GPU; kernels without dynamic LDS
// have none to set), then the launch; either failure is reported with `what`.
template <typename Kern, typename... Args>
int launch_kernel(Kern kern, dim3 grid, dim3 block, int lds, void *stream, const char *what, const Args &...args)
{
    if (lds > 0) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) {
            set_error(std::string(what) + ": hipFuncSetAttribute(" + std::to_string(lds) + " bytes of dynamic LDS): " + hipGetErrorString(e));
            return ECGB_ERR_HIP;
        }
    }
    hipLaunchKernelGGL(kern, grid, block, lds, (hipStream_t)stream, args...);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return ECGB_OK;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return ECGB_ERR_HIP;
}

// csrc/gemm_w4.hip: the four-wave kernel (128x128 wave tiles, one wave per SIMD) for products of whole 256x256 tiles
enum W4Layout { W4_NT = 0, W4_NN = 1, W4_TN = 2 };      // B [N, K] / B [K, N] / A [K, M] and B [K, N], all row-major
enum W4Epilogue {
    W4_PLAIN = 0,               // C [M, N]
    W4_GLU_SILU = 1,            // NT, N = 2 * inter, B = [gate rows; up rows]: H [M, inter] = act(gate) * up, C (gate|up) may be null
    W4_GLU_GELU = 2,
    W4_ROPE = 3,                // NT: heads of 64 columns below rope_cols leave rotated
    W4_GLU_BWD_SILU = 4,        // NN: the product is d(act(gate) * up), C [M, 2 N] = d gate | d up from GU = the forward's gate|up
    W4_GLU_BWD_GELU = 5,
    W4_GLU_BWD_LORA_SILU = 6,   // NN: the LoRA adapter's share (dt, at, lscale, lthr, lseed) joins the product before the GLU backward
    W4_GLU_BWD_LORA_GELU = 7,
    W4_LORA = 8,                // NN: the adapter's share and a plain store
};
struct W4Launch {
    const void *a; long long lda;
    const void *b; long long ldb;
    void *c; long long ldc;
    int M, N, K;
    float alpha;
    void *stream;
    int layout = W4_NT;
    int epilogue = W4_PLAIN;
    void *h = nullptr; long long ldh = 0;                                                       // GLU forward
    const void *a2 = nullptr; long long lda2 = 0; const void *b2 = nullptr; long long ldb2 = 0; int K2 = 0;      // NT: a second operand pair contracted behind the first
    const float *rope_cos = nullptr, *rope_sin = nullptr; int rope_cols = 0;                    // W4_ROPE
    const void *gu = nullptr; long long ldgu = 0;                                               // GLU backward
    const void *dt = nullptr, *at = nullptr; float lscale = 0.f; unsigned lthr = 0, lseed = 0;  // the LoRA epilogues
};
bool gemm_w4_applies(const void *a_dev, long long lda, const void *b_dev, long long ldb, const void *c_dev, long long ldc, int M, int N, int K);
bool gemm_w4_span_ok(int lay, long long lda, long long ldb, long long K, long long extra_rows_b);      // 32-bit DMA offsets over the whole contraction
int gemm_w4_launch(const W4Launch &L);

}  // namespace ecgb
