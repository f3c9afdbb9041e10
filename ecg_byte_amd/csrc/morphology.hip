// morphology.hip -- the reference's record sampling step (ecg_byte/utils/preprocess_utils.py:259-462, preprocess/sample_ecg.py) on MI355X,
// float64 throughout:
//   ecgb_morph_features_f64       extract_features (:259-347): 24 values per lead, one workgroup per (record, lead)
//   ecgb_kmpp_init_f64 / _step    KMeans' greedy k-means++ seeding (sklearn 1.5.2 _kmeans_plusplus); the host draws the random numbers
//   ecgb_kmeans_lloyd_f64         Lloyd iterations (sklearn _kmeans_single_lloyd), a batch of runs of any k, each frozen by its own state
//   ecgb_kmeans_finish_f64        the extra E-step of runs that stopped on tol / max_iter, and the inertia
//   ecgb_silhouette_f64           silhouette_samples over an index subset, per-(point, label) distance sums, no pairwise matrix
//   ecgb_dbscan_f64               DBSCAN(eps, min_samples) labels by streaming passes over the points (no neighbour lists)
// Every reduction runs in a fixed order (lane-strided partial sums, then a tree in LDS): the same inputs give the same bits on every run.  The only atomics are
// integer ones (DBSCAN's min-label hooking, whose fixed point does not depend on their order).  No workgroup waits on another: phases are launch boundaries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "tokenizer.hpp"

namespace {

constexpr int kLeads = 12;
constexpr int kFeat = 24;                 // values per lead, preprocess_utils.py:265-345
constexpr int kMaxL = 5000;
constexpr int kMinL = 8;                  // five db4 levels with one reflection per side need every band >= 7 samples
constexpr int kFs = 250;                  // analyze_morphologies never passes sampling_rate
constexpr int kDistance = 50;             // ceil(0.2 * 250)
constexpr int kNperseg = 1024;
constexpr int kWF = 8;                    // db4 taps
constexpr int kLevels = 5;
constexpr int kFT = 256;                  // features workgroup

__constant__ double kDb4Lo[kWF] = {-0.010597401784997278, 0.032883011666982945, 0.030841381835986965, -0.18703481171888114,
                                    -0.02798376941698385, 0.6308807679295904,  0.7148465705525415,   0.23037781330885523};

__device__ inline double db4_hi(int k) { return ((k & 1) ? 1.0 : -1.0) * kDb4Lo[kWF - 1 - k]; }   // (-1)^(k+1) lo[7 - k]

// block-wide sum in a fixed tree order (every lane gets the result)
template <int NT>
__device__ double block_sum(double v, double *red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// numpy's pairwise summation (add.reduce on a contiguous float64 array) for n <= 128 values: 8 partial sums, combined as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the rest in order; fewer than 8 values are summed in order.
__device__ double np_pairwise_small(const double *a, int n)
{
    if (n < 8) {
        double s = 0.0;                   // numpy starts from -0.0; the first addition makes the result the same
        for (int i = 0; i < n; ++i) s = (i == 0) ? a[0] : s + a[i];
        return n ? s : 0.0;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

// ---- features -------------------------------------------------------------------------------------------------------------------------------
struct FeatArgs {
    const double *x;                      // [records][12][L]
    double *out;                          // [records][288]
    unsigned char *flags;                 // [records]: 1 where the record holds a value that is not finite
    int L, P2, nperseg, nseg, bufN;
};

__device__ double np_lerp(double a, double b, double t)
{
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

__device__ double np_percentile_sorted(const double *s, int n, double q)
{
    const double vi = (double)(n - 1) * q;
    double prev = floor(vi);
    const double gamma = vi - prev;
    int lo = (int)prev, hi = lo + 1;
    if (vi >= (double)(n - 1)) { lo = n - 1; hi = n - 1; }
    return np_lerp(s[lo], s[hi], gamma);
}

__global__ void __launch_bounds__(kFT) features_kernel(FeatArgs A)
{
    extern __shared__ double lds[];
    const int L = A.L, t = threadIdx.x;
    const long long series = blockIdx.x;
    const long long rec = series / kLeads;
    const int lead = (int)(series % kLeads);
    double *sig = lds;                                   // [L]
    double *buf = sig + L;                               // [bufN]: sort, then FFT, then peaks, then wavelet bands
    double *psd = buf + A.bufN;                          // [kNperseg / 2 + 1]
    double *red = psd + (kNperseg / 2 + 1);              // [kFT]
    __shared__ int s_int[8];
    __shared__ double s_dbl[8];
    const double *src = A.x + series * L;

    int bad = 0;
    for (int i = t; i < L; i += kFT) {
        const double v = src[i];
        sig[i] = v;
        bad |= !isfinite(v);
    }
    if (t == 0) s_int[0] = 0;
    __syncthreads();
    if (bad) atomicOr(&s_int[0], 1);
    __syncthreads();
    if (s_int[0] && t == 0) A.flags[rec] = 1;            // every writer stores the same byte

    double f[kFeat];
    // ---- statistics: bitonic sort of a copy (padded with +inf) ----
    for (int i = t; i < A.P2; i += kFT) buf[i] = i < L ? sig[i] : INFINITY;
    __syncthreads();
    for (int k = 2; k <= A.P2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < A.P2; i += kFT) {
                const int p = i ^ j;
                if (p > i) {
                    const double a = buf[i], b = buf[p];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { buf[i] = b; buf[p] = a; }
                }
            }
            __syncthreads();
        }
    }
    double acc = 0.0;
    for (int i = t; i < L; i += kFT) acc += sig[i];
    const double mean = block_sum<kFT>(acc, red) / (double)L;
    acc = 0.0;
    for (int i = t; i < L; i += kFT) { const double d = sig[i] - mean; acc += d * d; }
    const double var = block_sum<kFT>(acc, red) / (double)L;
    const double vmax = buf[L - 1], vmin = buf[0];
    f[0] = mean; f[1] = sqrt(var); f[2] = vmax; f[3] = vmin;
    f[4] = (L & 1) ? buf[L / 2] : (buf[L / 2 - 1] + buf[L / 2]) / 2.0;
    f[5] = np_percentile_sorted(buf, L, 0.25);
    f[6] = np_percentile_sorted(buf, L, 0.75);
    __syncthreads();

    // ---- Welch: periodic Hann, constant detrend per segment, density scaling, one-sided, mean over segments ----
    {
        const int N = A.nperseg;
        const bool pow2 = (N & (N - 1)) == 0;
        double wsq = 0.0;
        for (int i = t; i < N; i += kFT) { double s, c; sincospi(2.0 * i / N, &s, &c); const double w = 0.5 - 0.5 * c; wsq += w * w; }
        const double scale = 1.0 / ((double)kFs * block_sum<kFT>(wsq, red));
        const int nb = N / 2 + 1;
        double pacc[3] = {0.0, 0.0, 0.0};                 // bins t, t + 256, t + 512
        double *re = buf, *im = buf + N;
        int logN = 0;
        while ((1 << logN) < N) ++logN;
        for (int sgi = 0; sgi < A.nseg; ++sgi) {
            const double *seg = sig + sgi * (N / 2);
            double sacc = 0.0;
            for (int i = t; i < N; i += kFT) sacc += seg[i];
            const double smean = block_sum<kFT>(sacc, red) / (double)N;
            if (pow2) {
                for (int i = t; i < N; i += kFT) {
                    double s, c; sincospi(2.0 * i / N, &s, &c);
                    const int r = (int)(__brev((unsigned)i) >> (32 - logN));
                    re[r] = (seg[i] - smean) * (0.5 - 0.5 * c);
                    im[r] = 0.0;
                }
                __syncthreads();
                for (int len = 2; len <= N; len <<= 1) {
                    const int half = len >> 1;
                    for (int b = t; b < N / 2; b += kFT) {
                        const int grp = b / half, pos = b % half;
                        const int i0 = grp * len + pos, i1 = i0 + half;
                        double s, c; sincospi(-2.0 * pos / len, &s, &c);
                        const double tr = re[i1] * c - im[i1] * s, ti = re[i1] * s + im[i1] * c;
                        const double ar = re[i0], ai = im[i0];
                        re[i0] = ar + tr; im[i0] = ai + ti;
                        re[i1] = ar - tr; im[i1] = ai - ti;
                    }
                    __syncthreads();
                }
                for (int q = 0; q < 3; ++q) {
                    const int k = t + q * kFT;
                    if (k < nb) pacc[q] += (re[k] * re[k] + im[k] * im[k]) * scale * ((k == 0 || (k == N / 2 && !(N & 1))) ? 1.0 : 2.0);
                }
                __syncthreads();
            } else {                                      // N = L < 1024, not a power of two: direct DFT of the windowed segment
                for (int i = t; i < N; i += kFT) { double s, c; sincospi(2.0 * i / N, &s, &c); re[i] = (seg[i] - smean) * (0.5 - 0.5 * c); }
                __syncthreads();
                for (int q = 0; q < 3; ++q) {
                    const int k = t + q * kFT;
                    if (k >= nb) continue;
                    double xr = 0.0, xi = 0.0;
                    long long m = 0;
                    for (int i = 0; i < N; ++i) {
                        double s, c; sincospi(-2.0 * (double)m / N, &s, &c);
                        xr += re[i] * c; xi += re[i] * s;
                        m += k; if (m >= N) m -= N;
                    }
                    pacc[q] += (xr * xr + xi * xi) * scale * ((k == 0 || (k == N / 2 && !(N & 1))) ? 1.0 : 2.0);
                }
                __syncthreads();
            }
        }
        for (int q = 0; q < 3; ++q) { const int k = t + q * kFT; if (k < nb) psd[k] = pacc[q] / (double)A.nseg; }
        __syncthreads();
        double tp = 0.0, cp = 0.0;
        const double fstep = 1.0 / ((double)N * (1.0 / kFs));   // scipy.fft.rfftfreq(N, 1 / fs): k * (1 / (N * d))
        for (int k = t; k < nb; k += kFT) { tp += psd[k]; cp += ((double)k * fstep) * psd[k]; }
        const double total = block_sum<kFT>(tp, red);
        const double csum = block_sum<kFT>(cp, red);
        if (t == 0) {                                     // first maximum, in bin order
            int bk = 0;
            for (int k = 1; k < nb; ++k) if (psd[k] > psd[bk]) bk = k;
            s_int[1] = bk;
        }
        __syncthreads();
        f[7] = total; f[8] = psd[s_int[1]]; f[9] = (double)s_int[1] * fstep;
        f[10] = total > 0.0 ? csum / total : 0.0;
        // a constant lead has no spectrum: exactly 0, whatever rounding leaves of the detrended segment (scipy keeps that noise: for 0.1 a total near
        // 8e-34 and a "centroid" of fstep / 3, the Hann window's own)
        if (vmax == vmin) { f[7] = 0.0; f[8] = 0.0; f[9] = 0.0; f[10] = 0.0; }
        __syncthreads();
    }

    // ---- peaks: scipy.signal.find_peaks(x, height=0.5 * max(x), distance=50) ----
    {
        int *cand = reinterpret_cast<int *>(buf);         // [<= L / 2] candidate positions, ascending
        unsigned char *keep = reinterpret_cast<unsigned char *>(cand + L / 2 + 1);
        int *kept = reinterpret_cast<int *>(keep + L / 2 + 8);   // [<= L / 50 + 1] final peaks
        double *qrs = psd;                                // reuse: per-peak QRS widths
        const double hmin = 0.5 * vmax;
        const int chunk = (L + kFT - 1) / kFT;
        const int i0 = max(1, t * chunk), i1 = min(L - 1, (t + 1) * chunk);
        int cnt = 0;
        for (int i = i0; i < i1; ++i) {
            if (!(sig[i - 1] < sig[i])) continue;
            int ia = i + 1;
            while (ia < L - 1 && sig[ia] == sig[i]) ++ia;
            if (sig[ia] < sig[i] && sig[(i + ia - 1) / 2] >= hmin) ++cnt;
        }
        int *scan = reinterpret_cast<int *>(red);
        scan[t] = cnt;
        __syncthreads();
        if (t == 0) { int s = 0; for (int u = 0; u < kFT; ++u) { const int c = scan[u]; scan[u] = s; s += c; } s_int[2] = s; }
        __syncthreads();
        int w = scan[t];
        for (int i = i0; i < i1; ++i) {
            if (!(sig[i - 1] < sig[i])) continue;
            int ia = i + 1;
            while (ia < L - 1 && sig[ia] == sig[i]) ++ia;
            const int mid = (i + ia - 1) / 2;
            if (sig[ia] < sig[i] && sig[mid] >= hmin) cand[w++] = mid;
        }
        const int m = s_int[2];
        __syncthreads();
        for (int i = t; i < m; i += kFT) keep[i] = 1;
        __syncthreads();
        if (t == 0) {
            // scipy's _select_by_peak_distance: candidates by descending height; a kept peak removes its unprocessed neighbours closer than `distance`.
            // Equal heights go later position first (a stable sort walked from the end): the project's rule.  scipy walks numpy's default argsort, which is
            // not stable, so its order among equal heights follows no rule and differs from this one on some leads (morphology.py, deliberate differences).
            for (;;) {
                int j = -1;
                for (int u = 0; u < m; ++u)
                    if (keep[u] == 1 && (j < 0 || sig[cand[u]] >= sig[cand[j]])) j = u;
                if (j < 0) break;
                keep[j] = 2;
                for (int u = j - 1; u >= 0 && cand[j] - cand[u] < kDistance; --u) keep[u] = 0;
                for (int u = j + 1; u < m && cand[u] - cand[j] < kDistance; ++u) keep[u] = 0;
            }
            int np_ = 0;
            for (int u = 0; u < m; ++u) if (keep[u] == 2) kept[np_++] = cand[u];
            s_int[3] = np_;
        }
        __syncthreads();
        const int np_ = s_int[3];
        for (int p = t; p < np_; p += kFT) {              // find_qrs_duration (:349-355): window int(0.1 * 250) = 25
            const int pk = kept[p], st = max(0, pk - 25), en = min(L, pk + 25);
            double mx = sig[st];
            for (int i = st + 1; i < en; ++i) mx = fmax(mx, sig[i]);
            int c = 0;
            for (int i = st; i < en; ++i) c += fabs(sig[i]) > 0.1 * mx;
            qrs[p] = (double)c / (double)kFs;
        }
        __syncthreads();
        if (t == 0) {
            double hr = 0.0, hrv = 0.0, qd = 0.0, tw = 0.0, stdev = 0.0;
            if (np_ > 1) {
                double *rr = psd + 128;                   // np.diff(peaks) / 250
                for (int p = 0; p + 1 < np_; ++p) rr[p] = (double)(kept[p + 1] - kept[p]) / (double)kFs;
                const int nr = np_ - 1;
                const double rmean = np_pairwise_small(rr, nr) / (double)nr;
                hr = 60.0 / rmean;
                double *dd = psd + 256;
                for (int p = 0; p < nr; ++p) { const double d = rr[p] - rmean; dd[p] = d * d; }
                hrv = sqrt(np_pairwise_small(dd, nr) / (double)nr);
                qd = np_pairwise_small(qrs, np_) / (double)np_;
                const int a = kept[np_ - 2], b = kept[np_ - 1];           // find_t_wave_amplitude: ecg[peaks[-2]:peaks[-1]]
                double mx = sig[a], mn = sig[a];
                for (int i = a + 1; i < b; ++i) { mx = fmax(mx, sig[i]); mn = fmin(mn, sig[i]); }
                tw = mx - mn;
                const int stp = b + 20;                                     // find_st_deviation: int(0.08 * 250)
                stdev = stp < L ? sig[stp] - sig[b] : 0.0;
            }
            s_dbl[0] = hr; s_dbl[1] = hrv; s_dbl[2] = qd; s_dbl[3] = tw; s_dbl[4] = stdev;
        }
        __syncthreads();
        for (int q = 0; q < 5; ++q) f[11 + q] = s_dbl[q];
        __syncthreads();
    }

    // ---- wavelet: mean |c| of pywt.wavedec(x, 'db4', level=5), mode symmetric, [cA5, cD5, ..., cD1] ----
    {
        const double *in = sig;
        int N = L;
        const int n1 = (L + kWF - 1) / 2;
        for (int lev = 1; lev <= kLevels; ++lev) {
            const int Nc = (N + kWF - 1) / 2;
            double *outA = buf + ((lev & 1) ? 0 : n1);
            double sa = 0.0, sd = 0.0;
            for (int o = t; o < Nc; o += kFT) {
                double a = 0.0, d = 0.0;
                for (int j = 0; j < kWF; ++j) {
                    int i = 2 * o + 1 - j;
                    if (i < 0) i = -1 - i;
                    else if (i >= N) i = 2 * N - 1 - i;
                    const double v = in[i];
                    a += kDb4Lo[j] * v;
                    d += db4_hi(j) * v;
                }
                outA[o] = a;
                sa += fabs(a);
                sd += fabs(d);
            }
            const double tsd = block_sum<kFT>(sd, red);     // also orders outA's writes before the next level's reads
            f[16 + kLevels + 1 - lev] = tsd / (double)Nc;
            if (lev == kLevels) f[16] = block_sum<kFT>(sa, red) / (double)Nc;
            in = outA;
            N = Nc;
        }
    }

    // ---- differences ----
    {
        double sa = 0.0, sq = 0.0;
        for (int i = t; i + 1 < L; i += kFT) { const double d = sig[i + 1] - sig[i]; sa += fabs(d); sq += d * d; }
        const double ta = block_sum<kFT>(sa, red), tq = block_sum<kFT>(sq, red);
        f[22] = ta / (double)(L - 1);
        f[23] = sqrt(tq / (double)(L - 1));
    }
    if (t < kFeat) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < kFeat; ++q) if (q == t) v = f[q];
        A.out[rec * (kLeads * kFeat) + lead * kFeat + t] = v;
    }
}

// ---- k-means --------------------------------------------------------------------------------------------------------------------------------
// Run r: k[r] centers at rows off[r] .. off[r] + k[r] - 1 of the center arrays; labels [runs][n]; closest [runs][n] (seeding only).
enum : int { kRunning = 0, kDone = 1, kNeedEStep = 2 };
constexpr int kPT = 1024;                 // seeding / per-run workgroups
constexpr int kMaxTrials = 8;             // 2 + int(log(k)) for k <= 256
constexpr int kMaxD = 288;
constexpr int kMaxK = 1024;

__device__ inline double dot_rows(const double *a, const double *b, int D)
{
    double s = 0.0;
    for (int d = 0; d < D; ++d) s += a[d] * b[d];
    return s;
}

__global__ void rownorms_kernel(const double *X, int n, int D, double *xsq)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) xsq[i] = dot_rows(X + i * D, X + i * D, D);
}

template <int NT>
__device__ void block_argmax_first(double &v, int &idx, double *rv, int *ri)
{
    // max value, smallest index among equal values
    const int t = threadIdx.x;
    rv[t] = v; ri[t] = idx;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) {
            const double a = rv[t], b = rv[t + s];
            const int ia = ri[t], ib = ri[t + s];
            if (b > a || (b == a && ib >= 0 && (ia < 0 || ib < ia))) { rv[t] = b; ri[t] = ib; }
        }
        __syncthreads();
    }
    v = rv[0]; idx = ri[0];
    __syncthreads();
}

// c = 0: the first center X[first[r]]; closest = squared distances in sklearn's expanded form, pot = their sum
__global__ void __launch_bounds__(kPT) kmpp_init_kernel(const double *X, const double *xsq, int n, int D, const int *off, const int *first,
                                                         double *centers, double *closest, double *pot)
{
    __shared__ double red[kPT];
    __shared__ double c0[kMaxD];
    const int r = blockIdx.x, t = threadIdx.x;
    const double *x0 = X + (long long)first[r] * D;
    for (int d = t; d < D; d += kPT) { c0[d] = x0[d]; centers[(long long)off[r] * D + d] = x0[d]; }
    __syncthreads();
    const double xx = dot_rows(c0, c0, D);
    double acc = 0.0;
    double *cl = closest + (long long)r * n;
    for (int i = t; i < n; i += kPT) {
        const double v = fmax((-2.0 * dot_rows(c0, X + (long long)i * D, D) + xx) + xsq[i], 0.0);
        cl[i] = v;
        acc += v;
    }
    const double s = block_sum<kPT>(acc, red);
    if (t == 0) pot[r] = s;
}

// center c of every run with k > c: candidates = searchsorted(cumsum(closest), u * pot), their potentials, the first minimum, the min-update
__global__ void __launch_bounds__(kPT) kmpp_step_kernel(const double *X, const double *xsq, int n, int D, const int *k, const int *off,
                                                         const int *trials, int c, const double *u, double *centers, double *closest, double *pot)
{
    __shared__ double red[kPT];
    __shared__ double pref[kPT + 1];
    __shared__ double cand[kMaxTrials * kMaxD];
    __shared__ double candsq[kMaxTrials];
    __shared__ double cpot[kMaxTrials];
    __shared__ int cid[kMaxTrials];
    __shared__ int s_best;
    const int r = blockIdx.x, t = threadIdx.x;
    if (c >= k[r]) return;
    const int T = trials[r];
    double *cl = closest + (long long)r * n;
    const int chunk = (n + kPT - 1) / kPT;
    const int b0 = min(n, t * chunk), b1 = min(n, b0 + chunk);
    double s = 0.0;
    for (int i = b0; i < b1; ++i) s += cl[i];
    red[t] = s;
    if (t < kMaxTrials) cid[t] = n;
    __syncthreads();
    if (t == 0) { double p = 0.0; for (int u2 = 0; u2 < kPT; ++u2) { pref[u2] = p; p += red[u2]; } pref[kPT] = p; }
    __syncthreads();
    const double P0 = pref[t];
    for (int q = 0; q < T; ++q) {
        const double v = u[(long long)r * kMaxTrials + q] * pot[r];
        if (b1 > b0 && (P0 + red[t]) >= v && (t == 0 || P0 < v)) {
            double p = P0;
            for (int i = b0; i < b1; ++i) { p += cl[i]; if (p >= v) { cid[q] = i; break; } }
        }
    }
    __syncthreads();
    for (int e = t; e < T * D; e += kPT) {
        const int q = e / D, d = e % D;
        const int id = min(cid[q], n - 1);
        cand[q * D + d] = X[(long long)id * D + d];
    }
    __syncthreads();
    if (t < T) candsq[t] = dot_rows(cand + t * D, cand + t * D, D);
    __syncthreads();
    double acc[kMaxTrials];
    for (int q = 0; q < kMaxTrials; ++q) acc[q] = 0.0;
    for (int i = t; i < n; i += kPT) {
        const double *xi = X + (long long)i * D;
        const double ci = cl[i];
        for (int q = 0; q < T; ++q) acc[q] += fmin(ci, fmax((-2.0 * dot_rows(cand + q * D, xi, D) + candsq[q]) + xsq[i], 0.0));
    }
    for (int q = 0; q < T; ++q) { const double v = block_sum<kPT>(acc[q], red); if (t == 0) cpot[q] = v; }
    if (t == 0) {
        int b = 0;
        for (int q = 1; q < T; ++q) if (cpot[q] < cpot[b]) b = q;
        s_best = b;
        pot[r] = cpot[b];
    }
    __syncthreads();
    const int b = s_best;
    for (int i = t; i < n; i += kPT) {
        const double v = fmax((-2.0 * dot_rows(cand + b * D, X + (long long)i * D, D) + candsq[b]) + xsq[i], 0.0);
        cl[i] = fmin(cl[i], v);
    }
    for (int d = t; d < D; d += kPT) centers[((long long)off[r] + c) * D + d] = cand[b * D + d];
}

__global__ void center_norms_kernel(const double *centers, int rows, int D, double *cn)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < rows) cn[j] = dot_rows(centers + (long long)j * D, centers + (long long)j * D, D);
}

// E-step: label = first argmin_j (|c_j|^2 - 2 x.c_j) (sklearn's lloyd chunk); runs in state `want` only; changed[r] = 1 if a label moved
__global__ void assign_kernel(const double *X, int n, int D, const int *k, const int *off, const double *centers, const double *cn,
                              int *labels, const int *state, int want, int *changed)
{
    const int r = blockIdx.y;
    if (state[r] != want) return;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *xi = X + i * D;
    const double *C = centers + (long long)off[r] * D;
    const double *N2 = cn + off[r];
    int best = 0;
    double bd = N2[0] + (-2.0 * dot_rows(xi, C, D));
    for (int j = 1; j < k[r]; ++j) {
        const double dj = N2[j] + (-2.0 * dot_rows(xi, C + (long long)j * D, D));
        if (dj < bd) { bd = dj; best = j; }
    }
    int *lab = labels + (long long)r * n + i;
    if (*lab != best) { *lab = best; changed[r] = 1; }
}

// M-step sums: one workgroup per (cluster, run), the run's points in index order, lane-strided, tree-combined
__global__ void __launch_bounds__(256) update_kernel(const double *X, int n, int D, const int *k, const int *off, const int *labels,
                                                      const int *state, double *sums, double *weights)
{
    __shared__ double red[256];
    const int j = blockIdx.x, r = blockIdx.y, t = threadIdx.x;
    if (state[r] != kRunning || j >= k[r]) return;
    const int *lab = labels + (long long)r * n;
    double *S = sums + ((long long)off[r] + j) * D;
    double cnt = 0.0;
    for (int i = t; i < n; i += 256) cnt += lab[i] == j ? 1.0 : 0.0;
    const double w = block_sum<256>(cnt, red);
    if (t == 0) weights[off[r] + j] = w;
    for (int d0 = 0; d0 < D; d0 += 4) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = t; i < n; i += 256) {
            if (lab[i] != j) continue;
            const double *xi = X + (long long)i * D;
            for (int q = 0; q < 4; ++q) if (d0 + q < D) a[q] += xi[d0 + q];
        }
        for (int q = 0; q < 4 && d0 + q < D; ++q) {
            const double v = block_sum<256>(a[q], red);
            if (t == 0) S[d0 + q] = v;
        }
    }
}

// relocation of empty clusters, averaging, center shift, convergence state (sklearn's _relocate_empty_clusters_dense, _average_centers, _center_shift)
__global__ void __launch_bounds__(256) finalize_kernel(const double *X, int n, int D, const int *k, const int *off, const int *labels,
                                                        double *centers, double *sums, double *weights, double *cn, int *state, int *changed,
                                                        int *n_iter, double tol, int max_iter)
{
    __shared__ double rv[256];
    __shared__ int ri[256];
    __shared__ int s_n_empty;
    __shared__ int empties[kMaxK];
    const int r = blockIdx.x, t = threadIdx.x;
    if (state[r] != kRunning) return;
    const int K = k[r];
    double *C = centers + (long long)off[r] * D, *S = sums + (long long)off[r] * D, *W = weights + off[r];
    const int *lab = labels + (long long)r * n;
    if (t == 0) { int e = 0; for (int j = 0; j < K; ++j) if (W[j] == 0.0) empties[e++] = j; s_n_empty = e; }
    __syncthreads();
    const int n_empty = s_n_empty;
    if (n_empty > 0) {
        // the n_empty points farthest from their (old) centers, farthest first (ties: smallest index; two clusters emptying at once is outside the parity claim)
        double last_v = INFINITY; int last_i = -1;
        for (int e = 0; e < n_empty; ++e) {
            const int j = empties[e];
            double bv = -1.0; int bi = -1;
            for (int i = t; i < n; i += 256) {
                double dsq = 0.0;
                const double *xi = X + (long long)i * D, *ci = C + (long long)lab[i] * D;
                for (int d = 0; d < D; ++d) { const double q = xi[d] - ci[d]; dsq += q * q; }
                const bool after = dsq < last_v || (dsq == last_v && i > last_i);
                if (after && (dsq > bv || (dsq == bv && (bi < 0 || i < bi)))) { bv = dsq; bi = i; }
            }
            block_argmax_first<256>(bv, bi, rv, ri);
            if (t == 0 && bi >= 0) {
                const int old = lab[bi];
                const double *xf = X + (long long)bi * D;
                for (int d = 0; d < D; ++d) { S[(long long)old * D + d] -= xf[d]; S[(long long)j * D + d] = xf[d]; }
                W[j] = 1.0;
                W[old] -= 1.0;
            }
            last_v = bv; last_i = bi;
            __syncthreads();
        }
    }
    __syncthreads();
    for (int e = t; e < K * D; e += 256) {
        const int j = e / D;
        if (W[j] > 0.0) { const double alpha = 1.0 / W[j]; S[e] *= alpha; }
    }
    __syncthreads();
    if (t == 0) {
        double tot = 0.0;
        for (int j = 0; j < K; ++j) {
            double s2 = 0.0;
            for (int d = 0; d < D; ++d) { const double q = S[(long long)j * D + d] - C[(long long)j * D + d]; s2 += q * q; }
            const double sh = sqrt(s2);
            tot += sh * sh;
        }
        rv[0] = tot;
    }
    __syncthreads();
    const double tot = rv[0];
    for (int e = t; e < K * D; e += 256) C[e] = S[e];
    __syncthreads();
    for (int j = t; j < K; j += 256) cn[off[r] + j] = dot_rows(C + (long long)j * D, C + (long long)j * D, D);
    if (t == 0) {
        const int it = ++n_iter[r];
        if (!changed[r]) state[r] = kDone;
        else if (tot <= tol || it >= max_iter) state[r] = kNeedEStep;
        changed[r] = 0;
    }
}

__global__ void __launch_bounds__(256) inertia_kernel(const double *X, int n, int D, const int *off, const double *centers, const int *labels,
                                                       int *state, double *inertia)
{
    __shared__ double red[256];
    const int r = blockIdx.x, t = threadIdx.x;
    const int *lab = labels + (long long)r * n;
    const double *C = centers + (long long)off[r] * D;
    double acc = 0.0;
    for (int i = t; i < n; i += 256) {
        const double *xi = X + (long long)i * D, *ci = C + (long long)lab[i] * D;
        double s = 0.0;
        for (int d = 0; d < D; ++d) { const double q = xi[d] - ci[d]; s += q * q; }
        acc += s;
    }
    const double v = block_sum<256>(acc, red);
    if (t == 0) { inertia[r] = v; state[r] = kDone; }
}

// ---- silhouette ------------------------------------------------------------------------------------------------------------------------------
// idx: the subset's rows grouped by label (label l at positions loff[l] .. loff[l + 1] - 1); one workgroup per position
__global__ void __launch_bounds__(256) silhouette_kernel(const double *X, const double *xsq, int D, const int *idx, const int *loff, int n_labels,
                                                          const int *lab_of_pos, double *s_out)
{
    __shared__ double red[256];
    __shared__ double xi[kMaxD];
    const int p = blockIdx.x, t = threadIdx.x;
    const long long row = idx[p];
    for (int d = t; d < D; d += 256) xi[d] = X[row * D + d];
    __syncthreads();
    const double xx = xsq[row];
    const int own = lab_of_pos[p];
    double a = 0.0, b = INFINITY;
    for (int l = 0; l < n_labels; ++l) {
        double acc = 0.0;
        for (int q = loff[l] + t; q < loff[l + 1]; q += 256) {
            if (q == p) continue;                         // the diagonal is 0
            const long long rj = idx[q];
            acc += sqrt(fmax((-2.0 * dot_rows(xi, X + rj * D, D) + xx) + xsq[rj], 0.0));
        }
        const double s = block_sum<256>(acc, red);
        const int cnt = loff[l + 1] - loff[l];
        if (l == own) a = cnt > 1 ? s / (double)(cnt - 1) : NAN;
        else b = fmin(b, s / (double)cnt);
    }
    if (t == 0) {
        double sv = (b - a) / fmax(a, b);
        if (!isfinite(sv)) sv = 0.0;                       // np.nan_to_num: singletons (0 / 0) and coincident clusters
        s_out[p] = sv;
    }
}

// ---- DBSCAN ----------------------------------------------------------------------------------------------------------------------------------
__device__ inline bool within(const double *X, long long i, long long j, int D, double eps2)
{
    double s = 0.0;
    const double *a = X + i * D, *b = X + j * D;
    for (int d = 0; d < D; ++d) { const double q = a[d] - b[d]; s += q * q; }
    return s <= eps2;
}

__global__ void db_core_kernel(const double *X, int n, int D, double eps2, int min_samples, int *core, int *lab)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int c = 0;
    for (int j = 0; j < n && c < min_samples; ++j) c += within(X, i, j, D, eps2);
    core[i] = c >= min_samples;
    lab[i] = i;
}

// lab[i] <- min lab over core neighbours (core i only); integer atomicMin, the fixed point (smallest core index of the component) is order-free
__global__ void db_hook_kernel(const double *X, int n, int D, double eps2, const int *core, int *lab, int *changed)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !core[i]) return;
    int m = lab[i];
    for (int j = 0; j < n; ++j)
        if (core[j] && within(X, i, j, D, eps2)) m = min(m, lab[j]);
    if (m < lab[i]) {
        const int old = atomicMin(&lab[i], m);
        atomicMin(&lab[old], m);                          // hook the old root as well
        *changed = 1;
    }
}

__global__ void db_jump_kernel(int n, const int *core, int *lab)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !core[i]) return;
    int l = lab[i];
    for (int s = 0; s < 32; ++s) { const int l2 = lab[l]; if (l2 == l) break; l = l2; }
    atomicMin(&lab[i], l);
}

// rank[i] = number of component roots (core i with lab[i] == i) before i: cluster numbers in order of each component's smallest core index
__global__ void __launch_bounds__(1024) db_rank_kernel(int n, const int *core, const int *lab, int *rank)
{
    __shared__ int part[1025];
    const int t = threadIdx.x;
    const int chunk = (n + 1023) / 1024;
    const int b0 = min(n, t * chunk), b1 = min(n, b0 + chunk);
    int c = 0;
    for (int i = b0; i < b1; ++i) c += core[i] && lab[i] == i;
    part[t] = c;
    __syncthreads();
    if (t == 0) { int s = 0; for (int u = 0; u < 1024; ++u) { const int v = part[u]; part[u] = s; s += v; } }
    __syncthreads();
    int s = part[t];
    for (int i = b0; i < b1; ++i) { rank[i] = s; s += core[i] && lab[i] == i; }
}

__global__ void db_label_kernel(const double *X, int n, int D, double eps2, const int *core, const int *lab, const int *rank, int *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (core[i]) { out[i] = rank[lab[i]]; return; }
    int m = -1;
    for (int j = 0; j < n; ++j)
        if (core[j] && within(X, i, j, D, eps2)) { const int l = rank[lab[j]]; if (m < 0 || l < m) m = l; }
    out[i] = m;
}

int launch_status(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { ecgb::set_error(std::string(what) + ": " + hipGetErrorString(e)); return ECGB_ERR_HIP; }
    return ECGB_OK;
}

int feature_plan(int L, int &P2, int &nperseg, int &nseg, int &bufN)
{
    if (L < kMinL || L > kMaxL) return ECGB_ERR_UNSUPPORTED;
    P2 = 1;
    while (P2 < L) P2 <<= 1;
    nperseg = std::min(kNperseg, L);
    nseg = (L - nperseg) / (nperseg / 2) + 1;
    const int n1 = (L + kWF - 1) / 2, n2 = (n1 + kWF - 1) / 2;
    const int peaks_bytes = (L / 2 + 1) * 4 + (L / 2 + 8) + (L / kDistance + 2) * 4;
    bufN = std::max({P2, 2 * nperseg, n1 + n2, (peaks_bytes + 7) / 8});
    return ECGB_OK;
}

}  // namespace

extern "C" size_t ecgb_morph_features_lds_bytes(int L)
{
    int P2, nperseg, nseg, bufN;
    if (feature_plan(L, P2, nperseg, nseg, bufN) != ECGB_OK) return 0;
    return (size_t)(L + bufN + kNperseg / 2 + 1 + kFT) * sizeof(double);
}

extern "C" int ecgb_morph_features_f64(const double *x_dev, int records, int L, double *out_dev, unsigned char *flags_dev, void *stream)
{
    if (!x_dev || !out_dev || !flags_dev || records <= 0) { ecgb::set_error("ecgb_morph_features_f64: bad argument"); return ECGB_ERR_INVALID; }
    FeatArgs A{};
    if (feature_plan(L, A.P2, A.nperseg, A.nseg, A.bufN) != ECGB_OK) {
        ecgb::set_error("ecgb_morph_features_f64: L must lie in 8 .. 5000");
        return ECGB_ERR_UNSUPPORTED;
    }
    if ((long long)records * kLeads > 0x7FFFFFFFll) { ecgb::set_error("ecgb_morph_features_f64: too many records"); return ECGB_ERR_UNSUPPORTED; }
    A.x = x_dev; A.out = out_dev; A.flags = flags_dev; A.L = L;
    const size_t lds = ecgb_morph_features_lds_bytes(L);
    if (hipFuncSetAttribute((const void *)features_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        ecgb::set_error("ecgb_morph_features_f64: cannot size the workgroup's LDS");
        return ECGB_ERR_HIP;
    }
    hipLaunchKernelGGL(features_kernel, dim3((unsigned)(records * kLeads)), dim3(kFT), lds, (hipStream_t)stream, A);
    return launch_status("features_kernel");
}

static int km_check(const double *X, int n, int D, int runs, const void *a, const void *b)
{
    if (!X || !a || !b || n <= 0 || runs <= 0) { ecgb::set_error("k-means: bad argument"); return ECGB_ERR_INVALID; }
    if (D < 1 || D > kMaxD) { ecgb::set_error("k-means: D must lie in 1 .. 288"); return ECGB_ERR_UNSUPPORTED; }
    return ECGB_OK;
}

extern "C" int ecgb_kmpp_init_f64(const double *X, int n, int D, int runs, const int *off_dev, const int *first_dev, double *xsq_dev,
                                  double *centers_dev, double *closest_dev, double *pot_dev, void *stream)
{
    int rc = km_check(X, n, D, runs, off_dev, first_dev);
    if (rc) return rc;
    hipLaunchKernelGGL(rownorms_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, X, n, D, xsq_dev);
    hipLaunchKernelGGL(kmpp_init_kernel, dim3(runs), dim3(kPT), 0, (hipStream_t)stream, X, xsq_dev, n, D, off_dev, first_dev, centers_dev, closest_dev, pot_dev);
    return launch_status("kmpp_init_kernel");
}

extern "C" int ecgb_kmpp_step_f64(const double *X, const double *xsq_dev, int n, int D, int runs, const int *k_dev, const int *off_dev, const int *trials_dev,
                                  int c, const double *u_dev, double *centers_dev, double *closest_dev, double *pot_dev, void *stream)
{
    int rc = km_check(X, n, D, runs, k_dev, u_dev);
    if (rc) return rc;
    hipLaunchKernelGGL(kmpp_step_kernel, dim3(runs), dim3(kPT), 0, (hipStream_t)stream, X, xsq_dev, n, D, k_dev, off_dev, trials_dev, c, u_dev,
                       centers_dev, closest_dev, pot_dev);
    return launch_status("kmpp_step_kernel");
}

extern "C" int ecgb_kmeans_lloyd_f64(const double *X, int n, int D, int runs, int k_max, int rows, const int *k_dev, const int *off_dev, double tol,
                                     int max_iter, int iters, double *centers_dev, double *sums_dev, double *weights_dev, double *cn_dev,
                                     int *labels_dev, int *state_dev, int *changed_dev, int *n_iter_dev, void *stream)
{
    int rc = km_check(X, n, D, runs, k_dev, off_dev);
    if (rc) return rc;
    if (k_max < 1 || k_max > kMaxK || rows < k_max || iters < 1) { ecgb::set_error("ecgb_kmeans_lloyd_f64: bad k_max / rows / iters"); return ECGB_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(center_norms_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, centers_dev, rows, D, cn_dev);
    const dim3 ga((n + 255) / 256, runs);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(assign_kernel, ga, dim3(256), 0, s, X, n, D, k_dev, off_dev, centers_dev, cn_dev, labels_dev, state_dev, (int)kRunning, changed_dev);
        hipLaunchKernelGGL(update_kernel, dim3(k_max, runs), dim3(256), 0, s, X, n, D, k_dev, off_dev, labels_dev, state_dev, sums_dev, weights_dev);
        hipLaunchKernelGGL(finalize_kernel, dim3(runs), dim3(256), 0, s, X, n, D, k_dev, off_dev, labels_dev, centers_dev, sums_dev, weights_dev, cn_dev,
                           state_dev, changed_dev, n_iter_dev, tol, max_iter);
    }
    return launch_status("ecgb_kmeans_lloyd_f64");
}

extern "C" int ecgb_kmeans_finish_f64(const double *X, int n, int D, int runs, int rows, const int *k_dev, const int *off_dev, const double *centers_dev,
                                      double *cn_dev, int *labels_dev, int *state_dev, int *changed_dev, double *inertia_dev, void *stream)
{
    int rc = km_check(X, n, D, runs, k_dev, off_dev);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(center_norms_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, centers_dev, rows, D, cn_dev);
    hipLaunchKernelGGL(assign_kernel, dim3((n + 255) / 256, runs), dim3(256), 0, s, X, n, D, k_dev, off_dev, centers_dev, cn_dev, labels_dev, state_dev,
                       (int)kNeedEStep, changed_dev);
    hipLaunchKernelGGL(inertia_kernel, dim3(runs), dim3(256), 0, s, X, n, D, off_dev, centers_dev, labels_dev, state_dev, inertia_dev);
    return launch_status("ecgb_kmeans_finish_f64");
}

extern "C" int ecgb_silhouette_f64(const double *X, const double *xsq_dev, int D, int m, const int *idx_dev, const int *loff_dev, int n_labels,
                                   const int *lab_of_pos_dev, double *s_dev, void *stream)
{
    if (!X || !xsq_dev || !idx_dev || !loff_dev || !lab_of_pos_dev || !s_dev || m <= 0 || n_labels < 1) {
        ecgb::set_error("ecgb_silhouette_f64: bad argument");
        return ECGB_ERR_INVALID;
    }
    if (D < 1 || D > kMaxD) { ecgb::set_error("ecgb_silhouette_f64: D must lie in 1 .. 288"); return ECGB_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(silhouette_kernel, dim3(m), dim3(256), 0, (hipStream_t)stream, X, xsq_dev, D, idx_dev, loff_dev, n_labels, lab_of_pos_dev, s_dev);
    return launch_status("silhouette_kernel");
}

extern "C" int ecgb_dbscan_f64(const double *X, int n, int D, double eps, int min_samples, int *labels_dev, int *work_dev, void *stream)
{
    if (!X || !labels_dev || !work_dev || n <= 0 || D < 1 || !(eps >= 0.0) || min_samples < 1) { ecgb::set_error("ecgb_dbscan_f64: bad argument"); return ECGB_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    int *core = work_dev, *lab = work_dev + n, *rank = work_dev + 2 * (size_t)n, *changed = work_dev + 3 * (size_t)n;
    const double eps2 = eps * eps;
    const dim3 g((n + 255) / 256), b(256);
    hipLaunchKernelGGL(db_core_kernel, g, b, 0, s, X, n, D, eps2, min_samples, core, lab);
    for (int pass = 0; pass < n + 1; ++pass) {
        if (hipMemsetAsync(changed, 0, sizeof(int), s) != hipSuccess) return launch_status("ecgb_dbscan_f64: memset");
        hipLaunchKernelGGL(db_hook_kernel, g, b, 0, s, X, n, D, eps2, core, lab, changed);
        hipLaunchKernelGGL(db_jump_kernel, g, b, 0, s, n, core, lab);
        int h = 0;
        if (hipMemcpyAsync(&h, changed, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return launch_status("ecgb_dbscan_f64: flag read");
        if (!h) break;
    }
    hipLaunchKernelGGL(db_rank_kernel, dim3(1), dim3(1024), 0, s, n, core, lab, rank);
    hipLaunchKernelGGL(db_label_kernel, g, b, 0, s, X, n, D, eps2, core, lab, rank, labels_dev);
    return launch_status("ecgb_dbscan_f64");
}
