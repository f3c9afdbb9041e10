"""The reference's record sampling step (ecg_byte/utils/preprocess_utils.py:259-462, preprocess/sample_ecg.py) on top of csrc/morphology.hip.

Features (extract_features), k-means (KMeans(k, random_state=42, n_init=10), Lloyd, as sklearn 1.5.2 runs it), silhouette and DBSCAN(eps=0.5,
min_samples=5) run on the device in float64; PCA(0.95) and StandardScaler are plumbing (a 288 x 288 covariance on the device, numpy's eigh on the
host).  The host draws k-means++'s random numbers with numpy's own RandomState in sklearn's order.  Neither sklearn, scipy nor pywt is imported.

Deliberate differences from the reference:
  * no PNG: find_optimal_clusters fills a report that the CLI writes to {data_root}/cluster_analysis.json (each k's inertia and silhouette, the
    elbow, the best-silhouette k, the chosen k, whether DBSCAN ran, the cluster sizes);
  * the silhouette subsample is RandomState(seed).permutation(n)[:10000] (the reference uses numpy's unseeded global generator);
  * stratified_sampling draws with random.Random(seed), over the clusters in ascending order, and fills the remainder from the unsampled files in
    their input order (the reference draws from an unseeded `random` and a `set`, whose order varies between runs);
  * a file holding a NaN / infinity raises ValueError naming it (the reference fails later, inside PCA).
  * find_peaks candidates of exactly equal height are taken "later position first" (a stable sort walked from the end).  The reference's order
    there is whatever numpy's default argsort gives, which follows no rule: restating scipy's selection with a stable sort differed from
    scipy.signal.find_peaks on 16 of 200 seeded leads with 3-16 equal-height candidates and on 98 of 200 with 17-119 (numpy 2.2.6, AVX-512 sort);
    with np.argsort's own order it matched 200 of 200.  Ties are common in quantised records: synth_ecg(20, 2500, seed=1) rounded to a step of 0.005
    has them in 230 of 240 leads, to 0.001 in 106.  Without equal heights the two agree exactly;
  * a constant lead (max == min) gets exactly 0 for total power, peak power, dominant frequency and spectral centroid.  The reference keeps the
    rounding noise of scipy's Welch there: for a constant 0.1 a total power near 8e-34 and a "centroid" of 0.08138... = fstep / 3, the Hann window's
    own.
"""
from __future__ import annotations

import ctypes as C
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib

LEADS, FEATURES_PER_LEAD = 12, 24
N_FEATURES = LEADS * FEATURES_PER_LEAD
MAX_TRIALS = 8                 # 2 + int(log(k)) for k <= 1024 fits
MAX_K = 1024
_BATCH = 2048                  # records per features launch


def _L():
    return _lib.lib()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _device_f64(x):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float64):
        raise TypeError("expected a float64 CUDA tensor")
    _lib.require_current(x.device)
    return x.contiguous()


# ---- features -------------------------------------------------------------------------------------------------------------------------------
def features(x):
    """extract_features for a float64 CUDA batch [records, 12, L] -> (features [records, 288], nonfinite flags [records] uint8)."""
    x = _device_f64(x)
    if x.dim() != 3 or x.shape[1] != LEADS:
        raise ValueError("features: a batch [records, 12, L]")
    R, _, L = x.shape
    out = torch.empty((R, N_FEATURES), dtype=torch.float64, device=x.device)
    flags = torch.zeros(R, dtype=torch.uint8, device=x.device)
    if R:
        _lib.check(_L().ecgb_morph_features_f64(_p(x), R, L, _p(out), _p(flags), _st()))
    return out, flags


def load_features(paths, workers=None, device=None):
    """np.load every path (threads, in order), the features kernel on batches of records: [len(paths), 288] on the device.  A file with a NaN /
    infinity raises ValueError naming it."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    workers = workers or min(16, os.cpu_count() or 1)
    out, L = [], None
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for b0 in range(0, len(paths), _BATCH):
            chunk = paths[b0:b0 + _BATCH]
            recs = list(pool.map(lambda p: np.load(p).astype(np.float64, copy=False), chunk))
            for p, r in zip(chunk, recs):
                if r.ndim != 2 or r.shape[0] != LEADS or (L is not None and r.shape[1] != L):
                    raise ValueError(f"{p}: expected a ({LEADS}, L) record with the same L as the others, got {r.shape}")
                L = r.shape[1]
            f, flags = features(torch.from_numpy(np.stack(recs)).to(device))
            bad = torch.nonzero(flags).flatten().tolist()
            if bad:
                raise ValueError(f"{chunk[bad[0]]}: the record holds a NaN or an infinity")
            out.append(f)
    if not out:
        raise ValueError("no .npy records")
    return torch.cat(out)


# ---- PCA(0.95) and StandardScaler -----------------------------------------------------------------------------------------------------------
def pca_components(F, n_components=0.95):
    """sklearn's covariance_eigh solver: (mean, components [ncomp, features], explained variance ratio).  Component count =
    searchsorted(cumsum(ratio), n_components, side='right') + 1; signs as svd_flip(u_based_decision=False) sets them."""
    n = F.shape[0]
    mean = F.mean(0)
    Cv = F.T @ F
    Cv -= n * mean[:, None] * mean[None, :]
    Cv /= n - 1
    ev, vec = np.linalg.eigh(Cv.cpu().numpy())
    ev, vec = ev[::-1].copy(), vec[:, ::-1].copy()
    ev[ev < 0.0] = 0.0
    ratio = ev / ev.sum()
    k = int(np.searchsorted(np.cumsum(ratio), n_components, side="right")) + 1
    k = min(k, F.shape[1])
    comp = vec.T[:k]
    signs = np.sign(comp[np.arange(k), np.argmax(np.abs(comp), axis=1)])
    comp = comp * signs[:, None]
    return mean, torch.from_numpy(comp).to(F.device), ratio


def standard_scale(X):
    """StandardScaler().fit_transform: ddof 0; a feature sklearn deems constant gets scale 1."""
    n = X.shape[0]
    mean = X.mean(0)
    var = ((X - mean) ** 2).mean(0)
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = torch.where(constant, torch.ones_like(var), torch.sqrt(var))
    return (X - mean) / scale


def pca_scale(F):
    """PCA(n_components=0.95).fit_transform, then StandardScaler (preprocess_utils.py:369-377)."""
    mean, comp, _ = pca_components(F)
    Xt = F @ comp.T - (mean[None, :] @ comp.T)
    return standard_scale(Xt).contiguous()


# ---- k-means --------------------------------------------------------------------------------------------------------------------------------
def _draws(n, k, n_init, random_state):
    """sklearn's k-means++ random numbers for KMeans(k, random_state, n_init): per run one choice(n, p=uniform), then uniform(size=2 + int(log k))
    for every further center, from one RandomState in order."""
    rs = np.random.RandomState(random_state)
    T = 2 + int(np.log(k))
    p = np.ones(n) / float(n)
    first = np.empty(n_init, dtype=np.int32)
    u = np.zeros((max(k - 1, 0), n_init, MAX_TRIALS))
    for r in range(n_init):
        first[r] = rs.choice(n, p=p)
        for c in range(1, k):
            u[c - 1, r, :T] = rs.uniform(size=T)
    return first, u, T


def _same_clustering(a, b):
    """sklearn's _is_same_clustering: every label of `a` maps to one label of `b`."""
    pairs = torch.unique(a.long() * (int(b.max()) + 1) + b.long())
    return pairs.numel() == torch.unique(a).numel()


def kmeans_many(X, ks, n_init=10, random_state=42, max_iter=300, tol=1e-4, sync_every=8):
    """KMeans(k, random_state, n_init).fit(X) for every k of `ks` in one batch of n_init * len(ks) device runs.  Returns {k: (labels int32 [n] on the
    device, inertia)}: the best run by sklearn's rule."""
    X = _device_f64(X)
    n, D = X.shape
    ks = [int(k) for k in ks]
    for k in ks:
        if n < k:
            raise ValueError(f"n_samples={n} should be >= n_clusters={k}.")
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k-means: 1 <= k <= {MAX_K}")
    tol_abs = float(torch.var(X, dim=0, unbiased=False).mean()) * tol
    Xc = (X - X.mean(0)).contiguous()
    dev = X.device
    runs = len(ks) * n_init
    k_run = np.repeat(np.array(ks, dtype=np.int32), n_init)
    off = np.zeros(runs, dtype=np.int32)
    off[1:] = np.cumsum(k_run)[:-1]
    rows, kmax = int(k_run.sum()), max(ks)
    firsts, u_all = np.empty(runs, np.int32), np.zeros((max(kmax - 1, 0), runs, MAX_TRIALS))
    trials = np.empty(runs, np.int32)
    for g, k in enumerate(ks):
        f, u, T = _draws(n, k, n_init, random_state)
        firsts[g * n_init:(g + 1) * n_init] = f
        u_all[:k - 1, g * n_init:(g + 1) * n_init] = u
        trials[g * n_init:(g + 1) * n_init] = T
    it = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    k_d, off_d, first_d, trials_d = it(k_run), it(off), it(firsts), it(trials)
    u_d = it(u_all)
    xsq = torch.empty(n, dtype=torch.float64, device=dev)
    centers = torch.empty((rows, D), dtype=torch.float64, device=dev)
    closest = torch.empty((runs, n), dtype=torch.float64, device=dev)
    pot = torch.empty(runs, dtype=torch.float64, device=dev)
    _lib.check(_L().ecgb_kmpp_init_f64(_p(Xc), n, D, runs, _p(off_d), _p(first_d), _p(xsq), _p(centers), _p(closest), _p(pot), _st()))
    for c in range(1, kmax):
        _lib.check(_L().ecgb_kmpp_step_f64(_p(Xc), _p(xsq), n, D, runs, _p(k_d), _p(off_d), _p(trials_d), c, _p(u_d[c - 1]), _p(centers),
                                           _p(closest), _p(pot), _st()))
    del closest
    sums = torch.empty_like(centers)
    weights = torch.empty(rows, dtype=torch.float64, device=dev)
    cn = torch.empty(rows, dtype=torch.float64, device=dev)
    labels = torch.full((runs, n), -1, dtype=torch.int32, device=dev)
    state = torch.zeros(runs, dtype=torch.int32, device=dev)
    changed = torch.zeros(runs, dtype=torch.int32, device=dev)
    n_iter = torch.zeros(runs, dtype=torch.int32, device=dev)
    done = 0
    while done < max_iter:
        step = min(sync_every, max_iter - done)
        _lib.check(_L().ecgb_kmeans_lloyd_f64(_p(Xc), n, D, runs, kmax, rows, _p(k_d), _p(off_d), tol_abs, max_iter, step, _p(centers), _p(sums),
                                              _p(weights), _p(cn), _p(labels), _p(state), _p(changed), _p(n_iter), _st()))
        done += step
        if not bool((state == 0).any()):
            break
    inertia = torch.empty(runs, dtype=torch.float64, device=dev)
    _lib.check(_L().ecgb_kmeans_finish_f64(_p(Xc), n, D, runs, rows, _p(k_d), _p(off_d), _p(centers), _p(cn), _p(labels), _p(state), _p(changed),
                                           _p(inertia), _st()))
    inertia = inertia.cpu().numpy()
    out = {}
    for g, k in enumerate(ks):
        best = None
        for r in range(g * n_init, (g + 1) * n_init):
            if best is None or (inertia[r] < inertia[best] and not _same_clustering(labels[r], labels[best])):
                best = r
        out[k] = (labels[best].clone(), float(inertia[best]))
    return out


def kmeans(X, k, n_init=10, random_state=42):
    """KMeans(k, random_state=42, n_init=10).fit: (labels int32 [n] on the device, inertia)."""
    return kmeans_many(X, [k], n_init=n_init, random_state=random_state)[k]


# ---- silhouette -----------------------------------------------------------------------------------------------------------------------------
def silhouette_subset(X, labels, idx):
    """mean(silhouette_samples(X[idx], labels[idx])) (sklearn's expanded euclidean distances; s = 0 for singletons)."""
    X = _device_f64(X)
    dev = X.device
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64, device=dev)
    m = idx.numel()
    lab = torch.as_tensor(labels, device=dev).long()[idx]
    present, enc = torch.unique(lab, return_inverse=True)
    nl = present.numel()
    if not 2 <= nl <= m - 1:
        raise ValueError(f"Number of labels is {nl}. Valid values are 2 to n_samples - 1 (inclusive)")
    order = torch.argsort(enc, stable=True)
    loff = torch.zeros(nl + 1, dtype=torch.int32, device=dev)
    loff[1:] = torch.cumsum(torch.bincount(enc, minlength=nl), 0).to(torch.int32)
    idx_sorted = idx[order].to(torch.int32).contiguous()
    lab_sorted = enc[order].to(torch.int32).contiguous()
    xsq = (X * X).sum(1).contiguous()
    s_sorted = torch.empty(m, dtype=torch.float64, device=dev)
    _lib.check(_L().ecgb_silhouette_f64(_p(X), _p(xsq), X.shape[1], m, _p(idx_sorted), _p(loff), nl, _p(lab_sorted), _p(s_sorted), _st()))
    s = torch.empty_like(s_sorted)
    s[order] = s_sorted
    return float(np.mean(s.cpu().numpy()))


def silhouette_score(X, labels, sample_size=10000, seed=0):
    """silhouette_score(X, labels, sample_size, random_state=seed): the subset is RandomState(seed).permutation(n)[:sample_size]."""
    idx = np.random.RandomState(seed).permutation(X.shape[0])[:sample_size]
    return silhouette_subset(X, labels, idx)


# ---- DBSCAN ---------------------------------------------------------------------------------------------------------------------------------
def dbscan(X, eps=0.5, min_samples=5):
    """DBSCAN(eps, min_samples).fit_predict(X): int32 labels [n] on the device."""
    X = _device_f64(X)
    n, D = X.shape
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    work = torch.empty(3 * n + 1, dtype=torch.int32, device=X.device)
    _lib.check(_L().ecgb_dbscan_f64(_p(X), n, D, float(eps), int(min_samples), _p(labels), _p(work), _st()))
    return labels


# ---- the reference's driver ------------------------------------------------------------------------------------------------------------------
def find_elbow_point(inertias):
    """preprocess_utils.py:441-445: argmin(diff(inertias)) + 2."""
    return int(np.argmin(np.diff(inertias))) + 2


def choose_k(inertias, silhouettes):
    """find_optimal_clusters' rule: (elbow, best-silhouette k, min of the two)."""
    elbow = find_elbow_point(inertias)
    best = silhouettes.index(max(silhouettes)) + 2
    return elbow, best, min(elbow, best)


def find_optimal_clusters(data, max_clusters, seed=0, report=None):
    """preprocess_utils.py:395-439: KMeans(k, random_state=42, n_init=10) for k = 2 .. max_clusters, the silhouette of each, the elbow; returns the
    chosen k.  `report` (a dict) receives each k's inertia and silhouette, the elbow and the best-silhouette k (instead of the reference's PNG)."""
    ks = list(range(2, max_clusters + 1))
    fits = kmeans_many(data, ks)
    inertias = [fits[k][1] for k in ks]
    sils = [silhouette_score(data, fits[k][0], sample_size=10000, seed=seed) for k in ks]
    elbow, best, chosen = choose_k(inertias, sils)
    print(f"Elbow method suggests {elbow} clusters")
    print(f"Highest silhouette score at {best} clusters")
    print(f"Chosen number of clusters: {chosen}")
    if report is not None:
        report.update(k=ks, inertia=inertias, silhouette=sils, elbow=elbow, best_silhouette_k=best, chosen_k=chosen)
    return chosen


def final_clusters(data, n_clusters, report=None):
    """preprocess_utils.py:382-392: KMeans(n_clusters) labels, or DBSCAN(eps=0.5, min_samples=5) labels when KMeans yields fewer than 3 clusters."""
    labels, _ = kmeans(data, n_clusters)
    ran = False
    if torch.unique(labels).numel() < 3:
        print("KMeans produced too few clusters. Trying DBSCAN...")
        labels = dbscan(data, eps=0.5, min_samples=5)
        ran = True
    clusters = labels.cpu().numpy().astype(np.int64)
    if report is not None:
        u, c = np.unique(clusters, return_counts=True)
        report.update(dbscan=ran, cluster_sizes={int(a): int(b) for a, b in zip(u, c)})
    return clusters, ran


def analyze_paths(paths, max_clusters=100, seed=0, workers=None, report=None):
    """analyze_morphologies on a given list of record paths (in that order): (file_paths, clusters, n_clusters)."""
    paths = list(paths)
    print("Loading and extracting features from ECG files...")
    F = load_features(paths, workers=workers)
    X = pca_scale(F)
    del F
    n_clusters = find_optimal_clusters(X, max_clusters, seed=seed, report=report)
    print(f"Optimal number of clusters determined: {n_clusters}")
    print("Clustering all data...")
    clusters, _ = final_clusters(X, n_clusters, report=report)
    return paths, clusters, len(np.unique(clusters))


def list_records(directory, subset_size=10000):
    """preprocess_utils.py:355-366: the first subset_size + 1 .npy files of os.listdir(directory), in that order."""
    out = []
    for filename in os.listdir(directory):
        if filename.endswith('.npy'):
            out.append(os.path.join(directory, filename))
            if len(out) == subset_size + 1:
                break
    return out


def analyze_morphologies(directory, max_clusters=100, subset_size=10000, seed=0, workers=None, report=None):
    """preprocess_utils.py:349-393: (file_paths, clusters, n_clusters)."""
    return analyze_paths(list_records(directory, subset_size), max_clusters, seed=seed, workers=workers, report=report)


def stratified_sampling(file_paths, clusters, n_samples=100000, seed=0):
    """preprocess_utils.py:447-462 with random.Random(seed): clusters in ascending order, then the remainder from the unsampled files in input order."""
    rng = random.Random(seed)
    clusters = np.asarray(clusters)
    unique_clusters = np.unique(clusters)
    per = n_samples // len(unique_clusters)
    sampled = []
    for cluster in unique_clusters:
        files = [file_paths[i] for i in range(len(file_paths)) if clusters[i] == cluster]
        sampled.extend(rng.sample(files, min(per, len(files))))
    remaining = n_samples - len(sampled)
    if remaining > 0:
        taken = set(sampled)
        rest = [f for f in file_paths if f not in taken]
        sampled.extend(rng.sample(rest, min(remaining, len(rest))))
    return sampled
