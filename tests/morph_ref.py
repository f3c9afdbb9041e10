"""Restatements for the sampling-step tests (ecg_byte_amd/morphology.py): pywt's db4 analysis (PyWavelets is absent here), extract_features
(ecg_byte/utils/preprocess_utils.py:259-347) with numpy / scipy and that db4, and the seeded inputs the goldens were computed on."""
import numpy as np

# db4 decomposition low-pass (the published Daubechies 4 filter, pywt's dec_lo); high-pass = quadrature mirror
DB4_DEC_LO = np.array([-0.010597401784997278, 0.032883011666982945, 0.030841381835986965, -0.18703481171888114,
                       -0.02798376941698385, 0.6308807679295904, 0.7148465705525415, 0.23037781330885523])
DB4_DEC_HI = np.array([(-1.0) ** (k + 1) * DB4_DEC_LO[7 - k] for k in range(8)])


def dwt_db4(x):
    """pywt.dwt(x, 'db4', mode='symmetric'): (len(x) + 7) // 2 coefficients per band, c[o] = sum_j f[j] xe[2 o + 1 - j] over the half-point
    symmetric extension (len(x) >= 7)."""
    x = np.asarray(x, np.float64)
    N, F = len(x), 8
    nc = (N + F - 1) // 2
    i = 2 * np.arange(nc)[:, None] + 1 - np.arange(F)[None, :]
    i = np.where(i < 0, -1 - i, np.where(i >= N, 2 * N - 1 - i, i))
    return (x[i] * DB4_DEC_LO).sum(1), (x[i] * DB4_DEC_HI).sum(1)


def wavedec_db4(x, level=5):
    """pywt.wavedec(x, 'db4', level): [cA_level, cD_level, ..., cD1]."""
    out, a = [], x
    for _ in range(level):
        a, d = dwt_db4(a)
        out.insert(0, d)
    return [a] + out


def lead_features(s, fs=250):
    """The 24 values extract_features appends for one lead."""
    from scipy import signal
    f = [np.mean(s), np.std(s), np.max(s), np.min(s), np.median(s), np.percentile(s, 25), np.percentile(s, 75)]
    freqs, psd = signal.welch(s, fs=fs, nperseg=min(1024, len(s)))
    tp = np.sum(psd)
    f += [tp, np.max(psd), freqs[np.argmax(psd)], np.sum(freqs * psd) / tp if tp > 0 else 0]
    peaks, _ = signal.find_peaks(s, height=0.5 * np.max(s), distance=0.2 * fs)
    if len(peaks) > 1:
        rr = np.diff(peaks) / fs
        w = int(0.1 * fs)
        qrs = []
        for p in peaks:
            seg = s[max(0, p - w):min(len(s), p + w)]
            qrs.append(np.sum(np.abs(seg) > 0.1 * np.max(seg)) / fs)
        f += [60 / np.mean(rr), np.std(rr), np.mean(qrs)]
        reg = s[peaks[-2]:peaks[-1]]
        f.append(np.max(reg) - np.min(reg))
        stp = peaks[-1] + int(0.08 * fs)
        f.append(s[stp] - s[peaks[-1]] if stp < len(s) else 0)
    else:
        f += [0, 0, 0, 0, 0]
    f += [np.mean(np.abs(c)) for c in wavedec_db4(s, 5)]
    d = np.diff(s)
    f += [np.mean(np.abs(d)), np.sqrt(np.mean(np.square(d)))]
    return np.array(f, dtype=np.float64), peaks


def extract_features(ecg):
    return np.concatenate([lead_features(ecg[l])[0] for l in range(ecg.shape[0])])


# index of each value within a lead's 24 (for tolerances)
EXACT = [2, 3, 4, 5, 6, 9, 11, 12, 13, 14, 15]          # order statistics, dominant frequency, peak-derived values
SUMS = [0, 1, 7, 8, 10, 16, 17, 18, 19, 20, 21, 22, 23]


def blobs(D, seed, n_blob=300, n_blobs=5, n_noise=200):
    """Well-separated Gaussian blobs plus a uniform-noise block: the k-means / silhouette goldens' input."""
    rng = np.random.default_rng([seed, D])
    centers = rng.uniform(-6, 6, size=(n_blobs, D))
    pts = [c + 0.6 * rng.standard_normal((n_blob, D)) for c in centers]
    pts.append(rng.uniform(-7, 7, size=(n_noise, D)))
    X = np.concatenate(pts)
    return X[rng.permutation(len(X))]


def dbscan_set(seed):
    """Core, border and noise points: two chains of cores, a border point between them touching both, a Gaussian blob, scattered noise."""
    rng = np.random.default_rng([seed, 77])
    a = np.stack([np.arange(0, 1.01, 0.11), np.zeros(10)], 1)[:10]
    b = np.stack([np.arange(1.9, 2.91, 0.11), np.zeros(10)], 1)[:10]
    a += 1e-3 * rng.standard_normal(a.shape)
    b += 1e-3 * rng.standard_normal(b.shape)
    border = np.array([[(a[:, 0].max() + b[:, 0].min()) / 2, 0.0]])
    blob = np.array([5.0, 5.0]) + 0.3 * rng.standard_normal((300, 2))
    noise = rng.uniform(-10, 10, size=(60, 2))
    return np.concatenate([b, blob, border, a, noise])


E2E_RECORDS, E2E_L, E2E_SEED, E2E_MAX_CLUSTERS, E2E_N_SAMPLES = 240, 2500, 11, 6, 60


def e2e_records():
    from ecg_byte_amd import synth
    return synth.synth_ecg(E2E_RECORDS, E2E_L, seed=E2E_SEED)


def e2e_names():
    return [f"rec_{i:04d}.npy" for i in range(E2E_RECORDS)]
