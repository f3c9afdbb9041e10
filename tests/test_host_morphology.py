"""Host-side pieces of the sampling step (ecg_byte_amd/morphology.py) and the restatements the GPU tests lean on (tests/morph_ref.py)."""
import random

import numpy as np
import pytest
import torch

import morph_ref as R
from ecg_byte_amd import morphology as M
from ecg_byte_amd import sample_ecg


def test_db4_known_answers():
    lo, hi = R.DB4_DEC_LO, R.DB4_DEC_HI
    # pywt's published db4 table carries about 12 significant digits: the identities hold to ~1e-12, not to the last bit
    assert abs(lo.sum() - np.sqrt(2)) < 1e-11 and abs((lo ** 2).sum() - 1) < 1e-11 and abs(hi.sum()) < 1e-11
    assert abs(np.dot(lo, hi)) < 1e-15
    assert all(abs(np.dot(lo[2 * m:], lo[:8 - 2 * m])) < 1e-11 for m in (1, 2, 3))      # orthogonal to its even shifts
    for n in (7, 8, 250, 2500, 5000):
        ca, cd = R.dwt_db4(np.random.default_rng(n).standard_normal(n))
        assert len(ca) == len(cd) == (n + 7) // 2
    x = np.zeros(64); x[20] = 1.0                        # an impulse away from the edges: c[o] = f[2 o + 1 - 20]
    ca, cd = R.dwt_db4(x)
    for o in range(len(ca)):
        j = 2 * o + 1 - 20
        assert ca[o] == (lo[j] if 0 <= j < 8 else 0.0) and cd[o] == (hi[j] if 0 <= j < 8 else 0.0)
    ca, cd = R.dwt_db4(np.arange(64, dtype=np.float64))  # a ramp: db4 has 4 vanishing moments, interior details vanish
    assert np.all(np.abs(cd[4:-4]) < 1e-12)
    assert [len(c) for c in R.wavedec_db4(np.zeros(2500))] == [84, 84, 162, 318, 630, 1253]


def test_feature_restatement_against_scipy():
    from scipy import signal
    x = np.random.default_rng(3).standard_normal(2500)
    f, peaks = R.lead_features(x)
    fr, p = signal.welch(x, fs=250, nperseg=1024)
    assert f[7] == np.sum(p) and f[9] == fr[np.argmax(p)]
    assert np.array_equal(peaks, signal.find_peaks(x, height=0.5 * x.max(), distance=50)[0])
    tie = np.zeros(300); tie[50] = tie[80] = 1.0
    assert list(R.lead_features(tie)[1]) == [80]
    assert len(f) == 24


def test_elbow_and_choice():
    assert M.find_elbow_point([100.0, 40.0, 30.0, 25.0]) == 2
    assert M.find_elbow_point([100.0, 90.0, 30.0, 25.0]) == 3
    assert M.choose_k([100.0, 90.0, 30.0, 25.0], [0.3, 0.2, 0.5, 0.1]) == (3, 4, 3)
    assert M.choose_k([100.0, 40.0, 30.0, 25.0], [0.3, 0.2, 0.5, 0.1]) == (2, 4, 2)


def test_stratified_sampling_determinism_and_counts():
    paths = [f"f{i}" for i in range(100)]
    clusters = np.array([i % 3 for i in range(90)] + [3] * 10)
    a = M.stratified_sampling(paths, clusters, 40, seed=5)
    assert a == M.stratified_sampling(paths, clusters, 40, seed=5)
    assert len(a) == 40 and len(set(a)) == 40
    assert sum(1 for p in a if int(p[1:]) >= 90) == 10
    b = M.stratified_sampling(paths, clusters, 95, seed=1)
    assert len(b) == 95 and len(set(b)) == 95
    rng = random.Random(1)                                    # the remainder comes from the unsampled files in input order
    per = 95 // 4
    want = []
    for c in range(4):
        want += rng.sample([p for i, p in enumerate(paths) if clusters[i] == c], min(per, int((clusters == c).sum())))
    rest = [p for p in paths if p not in set(want)]
    want += rng.sample(rest, 95 - len(want))
    assert b == want


@pytest.mark.parametrize("n", [300, 4000])
def test_pca_component_count_against_sklearn(n):
    PCA = pytest.importorskip("sklearn.decomposition").PCA
    rng = np.random.default_rng(n)
    F = rng.standard_normal((n, 288)) * np.geomspace(100, 0.01, 288) + rng.standard_normal(288)
    mean, comp, ratio = M.pca_components(torch.from_numpy(F))
    p = PCA(n_components=0.95).fit(F)
    assert comp.shape[0] == p.n_components_
    np.testing.assert_allclose(ratio[:comp.shape[0]], p.explained_variance_ratio_, rtol=1e-8)
    Xt = F @ comp.numpy().T - mean.numpy() @ comp.numpy().T
    np.testing.assert_allclose(np.abs(Xt), np.abs(p.transform(F)), rtol=1e-7, atol=1e-9)


def test_standard_scale_against_sklearn():
    SS = pytest.importorskip("sklearn.preprocessing").StandardScaler
    X = np.random.default_rng(2).standard_normal((500, 4)) * [1, 10, 0, 3]
    np.testing.assert_allclose(M.standard_scale(torch.from_numpy(X)).numpy(), SS().fit_transform(X), rtol=1e-12, atol=1e-12)


def test_cli_arguments():
    a = sample_ecg.get_args(["--unseg_dir", "d"])
    assert (a.unseg_dir, a.max_clusters, a.n_samples, a.data_root, a.seed, a.workers) == ("d", 200, 200000, "./data", 0, None)
    a = sample_ecg.get_args(["--unseg_dir=x", "--max_clusters", "9", "--n_samples", "7", "--data_root", "r", "--seed", "3", "--workers", "2"])
    assert (a.max_clusters, a.n_samples, a.data_root, a.seed, a.workers) == (9, 7, "r", 3, 2)


def test_kmeans_draws_follow_sklearn_order():
    first, u, T = M._draws(1000, 17, 10, 42)
    rs = np.random.RandomState(42)
    assert T == 2 + int(np.log(17))
    for r in range(10):
        assert first[r] == rs.choice(1000, p=np.ones(1000) / 1000.0)
        for c in range(1, 17):
            assert np.array_equal(u[c - 1, r, :T], rs.uniform(size=T))


def test_sample_step_imports_no_sklearn_scipy_pywt():
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys, ecg_byte_amd.sample_ecg, ecg_byte_amd.morphology; print(any(m.split('.')[0] in ('sklearn', 'scipy', 'pywt') for m in sys.modules))"
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, check=True).stdout.strip()
    assert out == "False"


# ---- the restatements the GPU edge tests call (tests/test_gpu_morphology_edges.py), pinned to scipy / sklearn -------------------------------------
PEAK_LENGTHS = [8, 9, 15, 49, 51, 255, 256, 257, 777, 1024, 2500, 5000]


def test_find_peaks_ref_equals_scipy_without_ties():
    from scipy import signal
    checked = 0
    for L in PEAK_LENGTHS:
        for s in range(45):
            x = np.random.default_rng([L, s]).standard_normal(L)
            if R.tied_candidates(x) > 1:
                continue
            want = signal.find_peaks(x, height=0.5 * x.max(), distance=50.0)[0]
            for stable in (True, False):
                assert np.array_equal(R.find_peaks_ref(x, 0.5 * x.max(), 50.0, stable=stable), want), (L, s, stable)
            assert np.array_equal(R.lead_features(x, peaks="stable")[0], R.lead_features(x)[0])
            checked += 1
    assert checked >= 500
    pl = np.zeros(40); pl[10:14] = 1.0; pl[20:23] = 2.0; pl[36:] = 3.0        # plateau midpoints; a plateau reaching the last sample is no peak
    assert list(R.local_maxima_ref(pl)) == [11, 21] == list(signal.find_peaks(pl)[0])


def test_find_peaks_ref_on_ties_is_scipy_with_numpys_argsort():
    """With equal heights scipy's answer is numpy's default argsort order (not a rule); stable=True is the project's rule, later position first."""
    from scipy import signal
    from ecg_byte_amd import synth
    leads = []
    for step in (0.005, 0.001):
        leads += list((np.round(synth.synth_ecg(20, 2500, seed=1) / step) * step).reshape(-1, 2500))
    leads += [R.equal_height_lead(2500, c, seed=s) for c in (3, 9, 16, 17, 40, 119) for s in range(10)]
    tied = 0
    for x in leads:
        want = signal.find_peaks(x, height=0.5 * x.max(), distance=50.0)[0]
        assert np.array_equal(R.find_peaks_ref(x, 0.5 * x.max(), 50.0, stable=False), want)
        tied += R.tied_candidates(x) > 1
    assert tied >= 230 + 106 + 60
    x = np.zeros(300); x[[50, 80, 110, 200]] = 1.0          # equal heights closer than 50: the later goes first, so 200, 110 (removes 80), 50
    assert list(R.find_peaks_ref(x, 0.5, 50.0, stable=True)) == [50, 110, 200]
    x = np.zeros(300); x[[50, 80]] = 1.0
    assert list(R.find_peaks_ref(x, 0.5, 50.0, stable=True)) == [80] == list(R.lead_features(x, peaks="stable")[1])


def test_flat_lead_reference_is_rounding_noise():
    """What the project's flat-lead rule (values 7 .. 10 exactly 0) replaces: scipy's Welch of a constant that is no dyadic number."""
    for c in (0.1, -3.3, 1e-7):
        f, peaks = R.lead_features(np.full(2500, c))
        assert R.flat_lead_rule(np.full(2500, c)) and len(peaks) == 0
        assert 0.0 < f[7] < 1e-11 * c * c and f[8] < 1e-11 * c * c
        assert abs(f[10] - (250.0 / 1024) / 3) < 1e-12    # the Hann window's own centroid, fstep / 3
    assert not R.flat_lead_rule(np.array([0.1, 0.1, 0.2]))


def _silhouette_cases():
    rng = np.random.default_rng(0)
    for m in (3, 255, 257):
        for D in (1, 40, 288):
            lab = rng.integers(0, 6, size=m)
            lab[:3] = [0, 1, 1]
            yield R.blobs_n(400, D, 1)[:m], lab
    lab = rng.integers(0, 7, size=600); lab[[10, 20, 30]] = [7, 8, 9]            # singletons
    yield R.blobs_n(600, 5, 2), lab
    yield R.blobs_n(2000, 5, 2), np.random.default_rng(3).permutation(np.arange(2000) % 300)


def _duplicates_case():
    X, which = R.repeated_locations(40, 10, 8, 0)
    X = X.copy()
    X[::3] += 0.5 * np.random.default_rng(0).standard_normal((len(X[::3]), 8))
    return X, which % 5


def test_silhouette_ref_against_sklearn():
    sil = pytest.importorskip("sklearn.metrics").silhouette_samples
    for X, lab in _silhouette_cases():
        want = sil(X, lab)
        # no coincident points: both forms agree with sklearn far inside the GPU tests' 1e-9
        assert np.abs(R.silhouette_ref(X, lab) - want).max() < 1e-12, X.shape
        assert np.abs(R.silhouette_ref_expanded(X, lab) - want).max() < 1e-12, X.shape
    X, lab = _duplicates_case()
    direct, expanded, want = R.silhouette_ref(X, lab), R.silhouette_ref_expanded(X, lab), sil(X, lab)
    # exact duplicates: sqrt of a cancelled difference, about sqrt(eps) |x| per coincident pair, in sklearn as in the expanded restatement.  Measured
    # here: 1.4e-9 / 2.0e-9 per sample (expanded / sklearn against direct), 1.22e-10 on the mean; the GPU test allows ten times the latter.
    assert np.abs(direct - want).max() < 1e-8 and np.abs(expanded - want).max() < 1e-8
    assert abs(direct.mean() - expanded.mean()) < 10 * 1.22e-10
    s = R.silhouette_ref(np.array([[0.0], [0.0], [1.0], [1.0], [5.0]]), np.array([0, 0, 1, 1, 2]))
    assert list(s[:2]) == [1.0, 1.0] and s[4] == 0.0       # a = 0 gives 1, a singleton 0
    assert list(R.silhouette_ref(np.zeros((4, 2)), np.array([0, 0, 1, 1]))) == [0.0] * 4       # 0 / 0


def _dbscan_cases():
    rng = np.random.default_rng(0)
    yield rng.uniform(-100, 100, size=(500, 3)), 5
    yield 0.1 * rng.standard_normal((400, 2)), 5
    yield R.dbscan_set(3), 1
    yield R.repeated_locations(30, 4, 2, 1)[0], 5
    yield R.repeated_locations(30, 5, 2, 1)[0], 5
    for order in ("ascending", "descending", "shuffled"):
        yield R.chain(3000, 0.5, order), 3
    yield R.shared_border()[0], 5
    for n in (1, 4, 1024, 1025):
        yield R.blobs_n(n, 2, 4, spread=0.3), 5
    X = R.blobs_n(10001, 40, 0, n_blobs=8, spread=0.1)
    yield (X - X.mean(0)) / X.std(0), 5


def test_dbscan_ref_against_sklearn():
    DBSCAN = pytest.importorskip("sklearn.cluster").DBSCAN
    for X, ms in _dbscan_cases():
        got = R.dbscan_ref(X, 0.5, ms)                     # asserts the tie-free condition: no pair within 1e-9 of eps
        assert np.array_equal(got, DBSCAN(eps=0.5, min_samples=ms).fit_predict(X)), (X.shape, ms)
    with pytest.raises(AssertionError):
        R.dbscan_ref(np.array([[0.0, 0.0], [0.5, 0.0]]), 0.5, 1)


KMEANS_CASES = ([(R.blobs_n(600, D, 0), k, {}) for D in (5, 40, 288) for k in (3, 9)]
                + [(R.blobs_n(n, 3, 0), 5, {}) for n in (5, 6, 37, 1023, 1025)]
                + [(R.blobs_n(600, 3, 0), k, {}) for k in (1, 4)]
                + [(R.blobs_n(3000, 6, 0), 12, kw) for kw in ({"max_iter": 1}, {"max_iter": 2}, {"max_iter": 5}, {"tol": 0.5})]
                + [(R.blobs_n(3000, 6, 0), 3, kw) for kw in ({}, {"max_iter": 5}, {"tol": 0.5})]
                + [(R.blobs_n(10001, 24, 0, n_blobs=40), k, {}) for k in (2, 7, 200)])


def test_kmeans_ref_against_sklearn():
    """Labels equal KMeans(...).labels_, inertia within 1e-10 relative, on every input of the GPU k-means tests; each is tie-free."""
    KMeans = pytest.importorskip("sklearn.cluster").KMeans
    import warnings
    reasons = set()
    for X, k, kw in KMEANS_CASES:
        ref = R.kmeans_ref(X, k, **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                # ConvergenceWarning at max_iter
            km = KMeans(n_clusters=k, random_state=42, n_init=10, **kw).fit(X)
        assert R.tie_free_centers(ref["Xc"], ref["centers"]), (X.shape, k, kw)
        assert np.array_equal(ref["labels"], km.labels_), (X.shape, k, kw)
        assert abs(ref["inertia"] - km.inertia_) <= 1e-10 * km.inertia_, (X.shape, k, kw)
        np.testing.assert_allclose(ref["centers"] + X.mean(0), km.cluster_centers_, rtol=1e-9, atol=1e-9)
        assert all(r["relocations"] == 0 for r in ref["runs"])
        if kw.get("max_iter"):
            assert all(r["n_iter"] <= kw["max_iter"] for r in ref["runs"])
        reasons |= {r["stop"] for r in ref["runs"]}
    assert reasons == {R.STRICT, R.TOL, R.MAX_ITER}


def test_kmeans_relocation_is_rare_and_keeps_weights_positive():
    """No seeded heavy-tailed run empties a cluster (so the parity tests never enter the relocation); with fewer distinct rows than clusters every run
    does, and the relocation arithmetic (S[old] -= x, W[old] -= 1) never leaves a cluster without weight."""
    for n, k, D in ((120, 40, 2), (300, 60, 2), (200, 17, 1), (1000, 100, 3)):
        for seed in range(3):
            assert all(r["relocations"] == 0 for r in R.kmeans_ref(R.heavy_tailed(n, D, seed), k)["runs"])
    for n_loc, copies, k in ((16, 20, 17), (16, 20, 24)):
        X, which = R.repeated_locations(n_loc, copies, 3, 0)
        ref = R.kmeans_ref(X, k)
        assert all(r["relocations"] > 0 and r["min_weight"] >= 1.0 for r in ref["runs"])
        assert all(len(set(ref["labels"][which == l])) == 1 for l in range(n_loc))
        assert ref["inertia"] <= 1e-10 * (X * X).sum()
    ref = R.kmeans_ref(R.repeated_locations(40, 5, 3, 0)[0], 40)
    assert ref["inertia"] <= 1e-10


def test_same_clustering_rule():
    a = np.array([0, 0, 1, 1, 2])
    assert R.same_clustering(a, np.array([2, 2, 0, 0, 1])) and not R.same_clustering(a, np.array([0, 1, 1, 1, 2]))
    assert M._same_clustering(torch.from_numpy(a), torch.tensor([2, 2, 0, 0, 1])) and not M._same_clustering(torch.from_numpy(a), torch.tensor([0, 1, 1, 1, 2]))
