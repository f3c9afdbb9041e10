"""Restatements for the sampling-step tests (ecg_byte_amd/morphology.py): pywt's db4 analysis (PyWavelets is absent here), extract_features
(ecg_byte/utils/preprocess_utils.py:259-347) with numpy / scipy and that db4, and the seeded inputs the goldens were computed on.

What each restatement claims (tests/test_host_morphology.py pins every one of them on the CPU):
  parity with the reference's libraries    lead_features(peaks="scipy"), find_peaks_ref(stable=False) (scipy, ties as numpy's default argsort orders them),
                                           silhouette_ref / silhouette_ref_expanded (sklearn's silhouette_samples), dbscan_ref (sklearn's DBSCAN),
                                           kmeans_ref on data that never empties a cluster (sklearn's KMeans: labels, inertia)
  the project's own documented rule        find_peaks_ref(stable=True) / lead_features(peaks="stable"): equal heights are taken later position first;
                                           flat_lead_rule: a constant lead has no spectrum (values 7 .. 10 are exactly 0);
                                           kmeans_ref's relocation of emptied clusters: farthest point first, equal distances by ascending index
                                           (sklearn's argpartition order is arbitrary there)."""
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


def local_maxima_ref(x):
    """scipy's _local_maxima_1d: the midpoint (left + right) // 2 of every run of equal samples that rises on its left and falls on its right.  A run
    that reaches the last sample has no falling edge and is no peak; neither end sample is ever one."""
    x = np.asarray(x, np.float64)
    mids, i, i_max = [], 1, len(x) - 1
    while i < i_max:
        if x[i - 1] < x[i]:
            ahead = i + 1
            while ahead < i_max and x[ahead] == x[i]:
                ahead += 1
            if x[ahead] < x[i]:
                mids.append((i + ahead - 1) // 2)
                i = ahead
        i += 1
    return np.array(mids, dtype=np.intp)


def find_peaks_ref(s, height, distance, stable=True):
    """scipy.signal.find_peaks(s, height=height, distance=distance)[0]: local maxima, heights >= height, then _select_by_peak_distance (candidates in
    ascending priority order, walked from the end; a kept one removes every candidate closer than ceil(distance)).  stable=True orders equal heights by a
    stable sort, so the later position goes first: the project's rule.  stable=False uses numpy's default argsort, as scipy does."""
    s = np.asarray(s, np.float64)
    peaks = local_maxima_ref(s)
    peaks = peaks[s[peaks] >= height]
    dist = int(np.ceil(distance))
    keep = np.ones(len(peaks), dtype=bool)
    order = np.argsort(s[peaks], kind="stable") if stable else np.argsort(s[peaks])
    for j in order[::-1]:
        if not keep[j]:
            continue
        k = j - 1
        while k >= 0 and peaks[j] - peaks[k] < dist:
            keep[k] = False
            k -= 1
        k = j + 1
        while k < len(peaks) and peaks[k] - peaks[j] < dist:
            keep[k] = False
            k += 1
    return peaks[keep]


def tied_candidates(s):
    """Largest number of find_peaks candidates (local maxima at or above half the maximum) of one lead that share a height."""
    s = np.asarray(s, np.float64)
    c = local_maxima_ref(s)
    h = s[c][s[c] >= 0.5 * np.max(s)]
    return int(np.unique(h, return_counts=True)[1].max()) if len(h) else 0


def lead_features(s, fs=250, peaks="scipy"):
    """The 24 values extract_features appends for one lead.  peaks="scipy" calls scipy.signal.find_peaks; peaks="stable" uses find_peaks_ref's stable
    order (the two agree wherever no two candidates share a height)."""
    from scipy import signal
    f = [np.mean(s), np.std(s), np.max(s), np.min(s), np.median(s), np.percentile(s, 25), np.percentile(s, 75)]
    freqs, psd = signal.welch(s, fs=fs, nperseg=min(1024, len(s)))
    tp = np.sum(psd)
    f += [tp, np.max(psd), freqs[np.argmax(psd)], np.sum(freqs * psd) / tp if tp > 0 else 0]
    if peaks == "scipy":
        peaks, _ = signal.find_peaks(s, height=0.5 * np.max(s), distance=0.2 * fs)
    elif peaks == "stable":
        peaks = find_peaks_ref(s, 0.5 * np.max(s), 0.2 * fs, stable=True)
    else:
        raise ValueError(peaks)
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


# ---- the flat-lead rule -----------------------------------------------------------------------------------------------------------------------
def flat_lead_rule(s):
    """True where the project writes exactly 0 to values 7 .. 10 (total power, peak power, dominant frequency, spectral centroid): every sample equal.
    scipy's Welch leaves rounding noise there (for 0.1: a total around 8e-34 and a 'centroid' of fstep / 3, the Hann window's own)."""
    s = np.asarray(s)
    return bool(np.max(s) == np.min(s))


# ---- silhouette -------------------------------------------------------------------------------------------------------------------------------
def _silhouette_from_sums(sums, counts, enc):
    """sums [m, labels]: each point's distance sum to every label's points; sklearn's rule: a = own sum / (count - 1), b = min over the other labels of
    sum / count, s = (b - a) / max(a, b); singletons and 0 / 0 give 0."""
    m = len(enc)
    own = counts[enc]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = sums[np.arange(m), enc] / (own - 1)
        other = sums / counts[None, :]
        other[np.arange(m), enc] = np.inf
        b = other.min(1)
        s = (b - a) / np.maximum(a, b)
    s[own == 1] = 0.0
    return np.nan_to_num(s)


def silhouette_ref(X, labels, chunk=500):
    """silhouette_samples(X, labels) by brute force in float64: every distance from the differences, sqrt(sum_d (x_id - x_jd)^2)."""
    X = np.asarray(X, np.float64)
    present, enc = np.unique(np.asarray(labels), return_inverse=True)
    m, nl = len(X), len(present)
    if not 2 <= nl <= m - 1:
        raise ValueError(f"Number of labels is {nl}. Valid values are 2 to n_samples - 1 (inclusive)")
    onehot = np.zeros((m, nl))
    onehot[np.arange(m), enc] = 1.0
    sums = np.empty((m, nl))
    for c0 in range(0, m, chunk):
        d2 = np.zeros((min(chunk, m - c0), m))
        for d in range(X.shape[1]):
            q = X[c0:c0 + chunk, d, None] - X[None, :, d]
            d2 += q * q
        sums[c0:c0 + chunk] = np.sqrt(d2) @ onehot
    return _silhouette_from_sums(sums, np.bincount(enc, minlength=nl).astype(np.float64), enc)


def silhouette_ref_expanded(X, labels, chunk=2000):
    """The same with sklearn's expanded distances, sqrt(max(x.x + y.y - 2 x.y, 0)), the diagonal set to 0 (what the kernel computes)."""
    X = np.asarray(X, np.float64)
    present, enc = np.unique(np.asarray(labels), return_inverse=True)
    m, nl = len(X), len(present)
    onehot = np.zeros((m, nl))
    onehot[np.arange(m), enc] = 1.0
    xsq = (X * X).sum(1)
    sums = np.empty((m, nl))
    for c0 in range(0, m, chunk):
        d2 = np.maximum((-2.0 * (X[c0:c0 + chunk] @ X.T) + xsq[c0:c0 + chunk, None]) + xsq[None, :], 0.0)
        d2[np.arange(d2.shape[0]), c0 + np.arange(d2.shape[0])] = 0.0
        sums[c0:c0 + chunk] = np.sqrt(d2) @ onehot
    return _silhouette_from_sums(sums, np.bincount(enc, minlength=nl).astype(np.float64), enc)


# ---- DBSCAN -----------------------------------------------------------------------------------------------------------------------------------
NEAR = 1e-9                               # make_morph_golden.NEAR


def _pair_d2(X, c0, c1):
    """Squared distances of rows c0 .. c1 - 1 to every row, from the differences."""
    d2 = np.zeros((c1 - c0, len(X)))
    for d in range(X.shape[1]):
        q = X[c0:c1, d, None] - X[None, :, d]
        d2 += q * q
    return d2


def dbscan_ref(X, eps, min_samples, chunk=500, check=True):
    """DBSCAN(eps, min_samples).fit_predict(X) by brute force.  sklearn's order: seeds in ascending index, each cluster expanded to the end before the
    next seed is looked at, a point labelled by the first cluster that reaches it.  So a cluster's number is the rank of its smallest core index and a
    border point gets the smallest number among its core neighbours' clusters, whatever the order of visits inside one cluster (here: whole frontiers).
    check=True asserts that no pair distance lies within NEAR of eps (the tie-free condition of make_morph_golden)."""
    X = np.asarray(X, np.float64)
    n = len(X)
    adj = np.empty((n, n), dtype=bool)
    for c0 in range(0, n, chunk):
        d2 = _pair_d2(X, c0, min(n, c0 + chunk))
        if check:
            assert not np.any(np.abs(np.sqrt(d2) - eps) < NEAR), "a pair distance lies at eps"
        adj[c0:c0 + chunk] = d2 <= eps * eps
    core = adj.sum(1) >= min_samples
    labels = np.full(n, -1, dtype=np.int64)
    cluster = 0
    for i in range(n):
        if labels[i] != -1 or not core[i]:
            continue
        labels[i] = cluster
        frontier = np.array([i])
        while len(frontier):
            reach = adj[frontier].any(0) & (labels == -1)
            labels[reach] = cluster
            frontier = np.flatnonzero(reach & core)
        cluster += 1
    return labels


# ---- k-means ----------------------------------------------------------------------------------------------------------------------------------
STRICT, TOL, MAX_ITER = "strict", "tol", "max_iter"


def _estep(Xc, C):
    """sklearn's lloyd chunk: first argmin_j of |c_j|^2 - 2 x.c_j."""
    return np.argmin((C * C).sum(1)[None, :] - 2.0 * (Xc @ C.T), axis=1)


def kmeans_ref(X, k, n_init=10, random_state=42, max_iter=300, tol=1e-4):
    """KMeans(k, n_init=n_init, random_state=random_state, max_iter=max_iter, tol=tol).fit(X), restated: greedy k-means++ on morphology._draws' random
    numbers, Lloyd with the expanded-distance E-step, the tol and max_iter stops with their extra E-step, the best of n_init by inertia unless it is the
    same clustering.  Returns labels, inertia, the best run's centers (of the centered data `Xc`) and per run n_iter, stop (STRICT / TOL / MAX_ITER),
    relocations and min_weight (the smallest cluster weight after any relocation).
    An emptied cluster takes the farthest point, equal distances by ascending index: the project's rule, not sklearn's argpartition order."""
    from ecg_byte_amd import morphology as M
    X = np.asarray(X, np.float64)
    n, D = X.shape
    tol_abs = np.mean(np.var(X, axis=0)) * tol
    Xc = X - X.mean(0)
    xsq = (Xc * Xc).sum(1)
    first, u, T = M._draws(n, k, n_init, random_state)
    runs, best = [], None
    for r in range(n_init):
        C = np.empty((k, D))
        C[0] = Xc[first[r]]
        closest = np.maximum((-2.0 * (Xc @ C[0]) + C[0] @ C[0]) + xsq, 0.0)
        pot = closest.sum()
        for c in range(1, k):
            ids = np.minimum(np.searchsorted(np.cumsum(closest), u[c - 1, r, :T] * pot), n - 1)
            cand = Xc[ids]
            dist = np.maximum((-2.0 * (cand @ Xc.T) + (cand * cand).sum(1)[:, None]) + xsq[None, :], 0.0)
            np.minimum(closest, dist, out=dist)
            pots = dist.sum(1)
            b = int(np.argmin(pots))
            pot, closest, C[c] = pots[b], dist[b], cand[b]
        labels_old = np.full(n, -1)
        stop, relocations, min_weight = MAX_ITER, 0, np.inf
        for it in range(max_iter):
            labels = _estep(Xc, C)
            W = np.bincount(labels, minlength=k).astype(np.float64)
            S = np.zeros((k, D))
            np.add.at(S, labels, Xc)
            empties = np.flatnonzero(W == 0)
            if len(empties):
                dsq = ((Xc - C[labels]) ** 2).sum(1)
                far = np.lexsort((np.arange(n), -dsq))[:len(empties)]
                for j, f in zip(empties, far):
                    old = labels[f]
                    S[old] -= Xc[f]
                    S[j] = Xc[f]
                    W[j] = 1.0
                    W[old] -= 1.0
                    relocations += 1
                min_weight = min(min_weight, W.min())
            nz = W > 0
            S[nz] *= (1.0 / W[nz])[:, None]
            shift = (np.sqrt(((S - C) ** 2).sum(1)) ** 2).sum()
            C = S
            if np.array_equal(labels, labels_old):
                stop = STRICT
                break
            if shift <= tol_abs:
                stop = TOL
                break
            labels_old = labels
        if stop != STRICT:
            labels = _estep(Xc, C)
        inertia = float(((Xc - C[labels]) ** 2).sum())
        runs.append(dict(n_iter=it + 1, stop=stop, relocations=relocations, min_weight=min_weight, inertia=inertia))
        if best is None or (inertia < best[1] and not same_clustering(labels, best[0])):
            best = (labels, inertia, C)
    return dict(labels=best[0], inertia=best[1], centers=best[2], Xc=Xc, runs=runs)


def same_clustering(a, b):
    """sklearn's _is_same_clustering: every label of `a` goes with one label of `b`."""
    return len(np.unique(a.astype(np.int64) * (int(b.max()) + 1) + b)) == len(np.unique(a))


def tie_free_centers(Xc, centers, chunk=1000):
    """make_morph_golden.tie_free_kmeans on given centers: no point whose two nearest centers lie within NEAR (relative) of each other."""
    if len(centers) < 2:
        return True
    for c0 in range(0, len(Xc), chunk):
        d = ((Xc[c0:c0 + chunk, None, :] - centers[None]) ** 2).sum(-1)
        d.sort(1)
        if not np.all(d[:, 1] - d[:, 0] > NEAR * np.maximum(d[:, 1], 1e-300)):
            return False
    return True


# ---- seeded inputs of the edge tests (seeds are constants; every condition they were picked for is asserted again where they are used) ------------
def blobs_n(n, D, seed, n_blobs=6, spread=0.7, noise_frac=0.1):
    """n points: Gaussian blobs plus a uniform-noise share, shuffled."""
    rng = np.random.default_rng([seed, n, D])
    centers = rng.uniform(-6, 6, size=(n_blobs, D))
    n_noise = int(n * noise_frac)
    which = rng.integers(0, n_blobs, size=n - n_noise)
    X = np.concatenate([centers[which] + spread * rng.standard_normal((n - n_noise, D)), rng.uniform(-7, 7, size=(n_noise, D))])
    return X[rng.permutation(n)]


def heavy_tailed(n, D, seed):
    """Student-t (2 degrees of freedom) points: far outliers, uneven clusters."""
    return np.random.default_rng([seed, n, D, 5]).standard_t(2.0, size=(n, D))


def repeated_locations(n_loc, copies, D, seed):
    """n_loc distinct random locations, each stored `copies` times, shuffled; returns (X, location index of every row)."""
    rng = np.random.default_rng([seed, n_loc, copies])
    loc = rng.uniform(-5, 5, size=(n_loc, D))
    which = rng.permutation(np.repeat(np.arange(n_loc), copies))
    return loc[which], which


def chain(n, eps, order, seed=0):
    """n core points on a line at 0.9 eps spacing (2-D, a little jitter across), stored in ascending, descending or shuffled order."""
    rng = np.random.default_rng([seed, n])
    X = np.stack([0.9 * eps * np.arange(n), 0.01 * eps * rng.standard_normal(n)], 1)
    if order == "descending":
        X = X[::-1]
    elif order == "shuffled":
        X = X[rng.permutation(n)]
    else:
        assert order == "ascending"
    return np.ascontiguousarray(X)


def shared_border(seed=0, eps=0.5):
    """Three tight groups of six points whose innermost points lie 0.9 eps from the origin, 120 degrees apart; the origin is a border point of all three
    (3 neighbours + itself < min_samples 5).  Shuffled, so the smallest cluster number is not the first stored.  Returns (X, the origin's row)."""
    rng = np.random.default_rng([seed, 3])
    pts = [np.zeros((1, 2))]
    for g in range(3):
        ang = 2 * np.pi * g / 3 + 0.2
        dirn = np.array([np.cos(ang), np.sin(ang)])
        inner = 0.9 * eps * dirn
        pts.append(inner[None])
        pts.append(inner + 0.3 * eps * dirn + 0.04 * eps * rng.standard_normal((5, 2)))
    X = np.concatenate(pts)
    perm = rng.permutation(len(X))
    return X[perm], int(np.flatnonzero(perm == 0)[0])


def spikes(L, positions, heights, base_amp=0.3):
    """A slow sinusoid below half the spikes' height with single-sample spikes on top."""
    s = base_amp * np.sin(2 * np.pi * 7.3 * np.arange(L) / 250)
    for p, h in zip(positions, heights):
        s[p] = h
    return s


def equal_height_lead(L, n_equal, seed):
    """n_equal spikes of height exactly 1.0 at random positions (many closer than 50 samples) among lower spikes of distinct heights."""
    rng = np.random.default_rng([seed, L, n_equal])
    pos = np.sort(rng.choice(np.arange(2, L - 2, 2), size=2 * n_equal, replace=False))
    eq = rng.permutation(2 * n_equal)[:n_equal]
    h = rng.uniform(0.55, 0.95, size=2 * n_equal)
    h[eq] = 1.0
    return spikes(L, pos, h)
