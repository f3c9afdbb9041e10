// quantizer.inc -- the quantiser's parameters, its exact threshold staircase (host) and the device function that reads it: shared by the
// translation units that quantise (encode.hip: ecgb_quantize_hip and the fused encode; detokenize.hip: the round-trip count), so one set of
// bin edges serves them all.  Include inside the unit's anonymous namespace, after <hip/hip_runtime.h>, <cmath>, <cstring>, <limits>.
#pragma once

// ------------------------------------------------------------------------------------------
// Reference arithmetic of normalize_all, one operation per line (compiled with
// -ffp-contract=off so nothing is fused).  Returns the alphabet index; NaN -> 0.
inline int quantize_ref(double x, double a, double d)
{
    double nrm = (x - a) / d;
    double c = nrm;
    if (c < 0.0) c = 0.0;
    if (c > 1.0) c = 1.0;
    double s = std::floor(c * 26.0);
    if (s > 25.0) s = 25.0;
    return (s == s) ? (int)s : 0;
}

inline uint64_t ordered_key(double x)
{
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

inline double from_ordered_key(uint64_t k)
{
    uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double x;
    std::memcpy(&x, &u, 8);
    return x;
}

struct QuantParams {
    double a;        // p1 - 0.5
    double d;        // ((p99 + 0.5) - (p1 - 0.5)) + 1e-6
    double scale;    // 26 / d, for the first guess of the level
    double nas;      // -a * scale: q = fma(x, scale, nas) in the staging loops of the encode kernels
    float amb_thr;   // a sample is ambiguous when |frac(q) - 0.5| exceeds this (staging loops of the encode kernels)
    double thr[28];  // thr[k] = smallest x whose level is >= k (k = 1..25); thr[0] = -inf, thr[26..27] = +inf
    int use_thresholds;
};

inline QuantParams make_quant_params(double p1, double p99)
{
    QuantParams q;
    q.a = p1 - 0.5;
    q.d = ((p99 + 0.5) - (p1 - 0.5)) + 1e-6;
    q.scale = 26.0 / q.d;
    q.nas = -(q.a * q.scale);
    const double inf = std::numeric_limits<double>::infinity();
    q.use_thresholds = (q.d > 0.0) && std::isfinite(q.d) && std::isfinite(q.a) && std::isfinite(q.scale);
    // beyond |a * scale| = 1e9 the rounding of fma(x, scale, nas) nears the 1e-4 band of level_f32: every group is then
    // declared ambiguous and takes the exact staircase (slow, exact)
    q.amb_thr = (std::fabs(q.a * q.scale) < 1e9) ? 0.5f - 1e-4f : -1.0f;
    q.thr[0] = -inf;
    q.thr[26] = q.thr[27] = inf;
    for (int k = 1; k <= 25; ++k) q.thr[k] = inf;
    if (!q.use_thresholds) return q;
    const uint64_t lo_all = ordered_key(-inf), hi_all = ordered_key(inf);
    for (int k = 1; k <= 25; ++k) {
        // smallest key in [lo_all, hi_all] with level >= k; level(+inf) = 25 so it exists
        uint64_t lo = lo_all, hi = hi_all;
        while (lo < hi) {
            uint64_t mid = lo + (hi - lo) / 2;
            if (quantize_ref(from_ordered_key(mid), q.a, q.d) >= k) hi = mid; else lo = mid + 1;
        }
        q.thr[k] = from_ordered_key(lo);
    }
    return q;
}

// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t level_from_thresholds(double x, double a, double scale,
                                                          const double *thr /* LDS, 28 entries */)
{
    double q = (x - a) * scale;
    int b = (q >= 0.0) ? ((q < 26.0) ? (int)q : 25) : 0;  // NaN -> 0
    while (x < thr[b]) --b;                                // thr[0] = -inf stops it
    while (b < 25 && x >= thr[b + 1]) ++b;
    return (uint32_t)b;
}
