// dropout_math.hpp -- the counter-based dropout mask shared by ecgb_dropout_bf16 (decoder_ops.hip) and the attention kernels with dropout on the
// probabilities (attention.hip): element `idx` of a tensor is kept iff mix32(seed, idx) >= drop_threshold(p).  Nothing is stored: whoever knows
// (p, seed) and the element's flat index evaluates the same bit again (the backward of either, tests/dropout_ref.py in numpy).
#pragma once
#include <hip/hip_runtime.h>

// the hash is splitmix64's finaliser over seed + idx * kMixStep, upper 32 bits.  The sum is linear in idx (mod 2^64), so a kernel whose elements sit at
// base + constant offsets forms it as (seed + base * kMixStep) + offset * kMixStep with the first part hoisted, and pays mix32_finish alone per element
// (two 64-bit multiplies)
constexpr unsigned long long kMixStep = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ unsigned mix32_finish(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)((z ^ (z >> 31)) >> 32);
}
__device__ __forceinline__ unsigned mix32(unsigned long long seed, unsigned long long idx)
{
    return mix32_finish(seed + idx * kMixStep);
}
// kept iff hash >= threshold: p = 0 keeps everything, p < 1 (a float: at most 1 - 2^-24) stays below 2^32
__host__ __device__ __forceinline__ unsigned drop_threshold(float p) { return (unsigned)(p * 4294967296.0); }
