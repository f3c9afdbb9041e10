"""numpy restatement of the counter-based dropout mask (ecg_byte_amd/csrc/dropout_math.hpp): element `idx` of a tensor is kept iff
mix32(seed, idx) >= (unsigned)(p * 2^32), p a float32.  uint64 arithmetic wraps as the kernels' does."""
import numpy as np

_STEP = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def mix32(seed, idx):
    """Upper 32 bits of splitmix64's finaliser over seed + idx * step (idx: any integer array; returned as uint32)."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & (2 ** 64 - 1)) + np.asarray(idx).astype(np.uint64) * _STEP
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)


def threshold(p):
    """(unsigned)(p * 4294967296.0) with p rounded to float32 first, as the C ABI takes it (0.1f is not 0.1)."""
    return np.uint32(int(float(np.float32(p)) * 4294967296.0))


def keep_flat(p, seed, n, start=0):
    """Keep pattern (bool [n]) of the elements start .. start + n - 1 of a contiguous tensor."""
    return mix32(seed, np.arange(start, start + n, dtype=np.uint64)) >= threshold(p)


def attn_keep(p, seed, B, Hq, S):
    """Keep pattern (bool [B, Hq, S, S]) of attention with dropout on the probabilities: element (b, hq, query i, key j) has the flat index
    ((b Hq + hq) S + i) S + j of a contiguous [B Hq, S, S] tensor."""
    return keep_flat(p, seed, B * Hq * S * S).reshape(B, Hq, S, S)
