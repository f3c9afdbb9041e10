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
