"""The sampling step on the device (ecg_byte_amd/morphology.py, csrc/morphology.hip) against numpy / scipy restatements (tests/morph_ref.py) and
sklearn's answers stored in tests/golden/morph_golden.npz (tests/golden/make_morph_golden.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import morph_ref as R
from ecg_byte_amd import morphology as M
from ecg_byte_amd import preprocess_utils as PU
from ecg_byte_amd import synth, _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "morph_golden.npz"))


def _edge_leads(L):
    t = np.arange(L)
    leads = [np.full(L, 0.5), -1.0 - np.abs(np.sin(t / 7.0)), np.zeros(L)]
    base = 0.3 * np.sin(2 * np.pi * 7.3 * t / 250)       # below half the peaks' height (no peaks of its own); gives the spectrum a clear maximum
    one = base.copy(); one[L // 2] = 1.0; leads.append(one)                                          # one peak
    two = base.copy(); two[L // 4] = 1.0; two[3 * L // 4] = 0.8; leads.append(two)                  # two peaks
    pl = base.copy(); pl[L // 3:L // 3 + 4] = 1.0; pl[2 * L // 3] = 0.9; leads.append(pl)           # plateau peak (midpoint)
    tie = base.copy(); tie[L // 2] = 1.0; tie[L // 2 + 30] = 1.0; tie[L // 5] = 0.7; leads.append(tie)   # equal heights closer than 50: the later wins
    rng = np.random.default_rng(L)
    while len(leads) < 12:
        leads.append(rng.standard_normal(L))
    return np.stack(leads)


def _check_features(x, peaks="scipy"):
    got, flags = M.features(torch.from_numpy(x).cuda())
    got = got.cpu().numpy().reshape(len(x), 12, 24)
    assert not flags.any()
    for r in range(len(x)):
        for l in range(12):
            want, _ = R.lead_features(x[r, l], peaks=peaks)
            g = got[r, l]
            for q in R.EXACT:
                assert g[q] == want[q], (r, l, q, g[q], want[q])
            scale = np.max(np.abs(x[r, l]))
            for q in R.SUMS:
                # values linear in x (mean, std, wavelet bands, differences) may also differ by 1e-11 max|x|, the power terms by 1e-11 max|x|^2
                tol = 1e-11 * abs(want[q]) + {7: 1e-11 * scale ** 2, 8: 1e-11 * scale ** 2, 10: 0.0}.get(q, 1e-11 * scale)
                assert abs(g[q] - want[q]) <= tol, (r, l, q, g[q], want[q])


@pytest.mark.parametrize("L", [250, 500, 2500, 5000])
def test_features_synthetic(L):
    _check_features(synth.synth_ecg(3, L, seed=L))


@pytest.mark.parametrize("L", [250, 1250, 2500])
def test_features_edge_leads(L):
    x = _edge_leads(L)[None]
    _check_features(x)
    _, peaks = R.lead_features(x[0, 6])
    assert list(peaks) == [L // 5, L // 2 + 30]


def test_features_flags_nonfinite_and_refuses_lengths():
    x = synth.synth_ecg(3, 500, seed=1)
    x[1, 4, 7] = np.nan
    _, flags = M.features(torch.from_numpy(x).cuda())
    assert flags.cpu().tolist() == [0, 1, 0]
    for L in (4, 5001):
        with pytest.raises(_lib.EcgbError):
            M.features(torch.zeros((1, 12, L), dtype=torch.float64, device="cuda"))


def test_features_single_record_name():
    x = synth.synth_ecg(1, 2500, seed=4)[0]
    f = PU.extract_features(x)
    assert f.shape == (288,)
    np.testing.assert_allclose(f, R.extract_features(x), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("D", [1, 3, 8])
def test_kmeans_matches_sklearn(G, D):
    X = torch.from_numpy(R.blobs(D, int(G[f"blobs_seed_D{D}"]))).cuda()
    fits = M.kmeans_many(X, [2, 3, 8, 17])
    for k in (2, 3, 8, 17):
        labels, inertia = fits[k]
        assert np.array_equal(labels.cpu().numpy(), G[f"km_labels_D{D}_k{k}"]), (D, k)
        assert abs(inertia - float(G[f"km_inertia_D{D}_k{k}"])) <= 1e-10 * float(G[f"km_inertia_D{D}_k{k}"])
    one, inertia1 = M.kmeans(X, 8)                 # a k alone gives what the batch gave
    assert torch.equal(one, fits[8][0]) and inertia1 == fits[8][1]


@pytest.mark.parametrize("D", [1, 3, 8])
def test_silhouette_matches_sklearn(G, D):
    X = torch.from_numpy(R.blobs(D, int(G[f"blobs_seed_D{D}"]))).cuda()
    for k in (2, 3, 8):
        lab = torch.from_numpy(G[f"km_labels_D{D}_k{k}"].astype(np.int64)).cuda()
        for s in (0, 5):
            idx = np.random.RandomState(s).permutation(X.shape[0])[:700]
            got = M.silhouette_subset(X, lab, idx)
            assert abs(got - float(G[f"sil_D{D}_k{k}_s{s}"])) <= 1e-9, (D, k, s)
            assert got == M.silhouette_score(X, lab, sample_size=700, seed=s)


def test_dbscan_matches_sklearn(G):
    Y = torch.from_numpy(R.dbscan_set(0)).cuda()
    got = M.dbscan(Y, eps=0.5, min_samples=5).cpu().numpy()
    assert np.array_equal(got, G["dbscan_labels"])


def test_determinism():
    x = torch.from_numpy(synth.synth_ecg(4, 2500, seed=9)).cuda()
    a, b = M.features(x)[0], M.features(x)[0]
    assert torch.equal(a, b)
    X = torch.from_numpy(R.blobs(3, 0)).cuda()
    f1, f2 = M.kmeans_many(X, [3, 5]), M.kmeans_many(X, [3, 5])
    for k in (3, 5):
        assert torch.equal(f1[k][0], f2[k][0]) and f1[k][1] == f2[k][1]
    lab = f1[5][0]
    assert M.silhouette_score(X, lab, 500, 1) == M.silhouette_score(X, lab, 500, 1)
    assert torch.equal(M.dbscan(X), M.dbscan(X))


def test_kmeans_refusals():
    X = torch.zeros((5, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        M.kmeans(X, 6)
    with pytest.raises(ValueError):
        M.kmeans(torch.zeros((2000, 2), dtype=torch.float64, device="cuda"), M.MAX_K + 1)
    with pytest.raises(_lib.EcgbError):
        M.kmeans(torch.zeros((50, 289), dtype=torch.float64, device="cuda"), 2)


@pytest.fixture(scope="module")
def e2e_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("unseg")
    for name, r in zip(R.e2e_names(), R.e2e_records()):
        np.save(d / name, r)
    return d


def test_end_to_end_path_list(G, e2e_dir):
    paths = [str(e2e_dir / n) for n in R.e2e_names()]
    report = {}
    fp, clusters, n_clusters = M.analyze_paths(paths, R.E2E_MAX_CLUSTERS, seed=0, report=report)
    assert report["chosen_k"] == int(G["e2e_k"]) and report["dbscan"] == bool(G["e2e_dbscan"])
    assert np.array_equal(clusters, G["e2e_labels"])
    assert n_clusters == len(np.unique(G["e2e_labels"]))
    sampled = M.stratified_sampling(fp, clusters, R.E2E_N_SAMPLES, seed=0)
    assert [os.path.basename(p) for p in sampled] == list(G["e2e_sampled"])


def test_final_fit_without_dbscan():
    X = torch.from_numpy(R.blobs(3, 0)).cuda()
    report = {}
    clusters, ran = M.final_clusters(X, 5, report=report)
    assert not ran and len(np.unique(clusters)) == 5
    assert np.array_equal(clusters, M.kmeans(X, 5)[0].cpu().numpy())
    assert sum(report["cluster_sizes"].values()) == X.shape[0]


def test_cli_writes_list_and_report(e2e_dir, tmp_path):
    root = tmp_path / "data"
    cmd = [sys.executable, "-m", "ecg_byte_amd.sample_ecg", "--unseg_dir", str(e2e_dir), "--max_clusters", str(R.E2E_MAX_CLUSTERS),
           "--n_samples", str(R.E2E_N_SAMPLES), "--data_root", str(root), "--workers", "4"]
    subprocess.run(cmd, cwd=ROOT, check=True, timeout=600)
    listed = open(root / f"sampled_ecg_files_{R.E2E_N_SAMPLES}.txt").read().split("\n")[:-1]
    fp, clusters, _ = PU.analyze_morphologies(str(e2e_dir), R.E2E_MAX_CLUSTERS, R.E2E_N_SAMPLES)
    assert listed == PU.stratified_sampling(fp, clusters, R.E2E_N_SAMPLES, seed=0)
    rep = json.load(open(root / "cluster_analysis.json"))
    for key in ("k", "inertia", "silhouette", "elbow", "best_silhouette_k", "chosen_k", "dbscan", "cluster_sizes"):
        assert key in rep
    assert len(rep["inertia"]) == R.E2E_MAX_CLUSTERS - 1
