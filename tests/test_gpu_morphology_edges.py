"""The sampling step's kernels (csrc/morphology.hip) at the lengths, ties, amplitudes and sizes the command line reaches, against the float64
restatements of tests/morph_ref.py (pinned to scipy / sklearn on the CPU by tests/test_host_morphology.py).  Tolerances are those of
tests/test_gpu_morphology.py; where a case follows the project's own rule instead of the reference's libraries, the test says so."""
import numpy as np
import pytest
import torch

import morph_ref as R
from test_gpu_morphology import _check_features
from ecg_byte_amd import morphology as M
from ecg_byte_amd import synth

pytestmark = pytest.mark.gpu


def _record(leads, L, seed=0):
    """[1, 12, L]: the given leads, filled up with random ones."""
    rng = np.random.default_rng([seed, L])
    leads = [np.asarray(s, np.float64) for s in leads]
    assert len(leads) <= 12 and all(len(s) == L for s in leads)
    while len(leads) < 12:
        leads.append(rng.standard_normal(L))
    return np.stack(leads)[None]


# ---- features ---------------------------------------------------------------------------------------------------------------------------------
# odd L (median branch, odd-N one-sided doubling), radix-2 below 1024 (8, 256, 512), the direct DFT (9 .. 1023), the Welch segment-count steps
# (1535 | 1536, 2047 | 2048), the shortest length
@pytest.mark.parametrize("L", [8, 9, 15, 49, 51, 255, 256, 257, 512, 1023, 1024, 1025, 1535, 1536, 2047, 2048, 4096, 4999])
def test_features_lengths(L):
    x = np.random.default_rng([7, L]).standard_normal((2, 12, L))
    assert all(R.tied_candidates(s) <= 1 for s in x.reshape(-1, L))
    _check_features(x)
    _check_features(synth.synth_ecg(2, L, seed=L))


@pytest.mark.parametrize("L", [777, 2500])
def test_features_peaks_at_the_ends(L):
    chunk = -(-L // 256)                                  # samples per lane in the candidate scan
    leads, want_in, want_out = [], [], []
    leads.append(R.spikes(L, [1, L // 2, L - 2], [1.0, 0.8, 0.9])); want_in.append([1, L - 2]); want_out.append([])
    leads.append(R.spikes(L, [L // 3, L - 10], [1.0, 0.9])); want_in.append([L - 10]); want_out.append([])          # st deviation: peak + 20 >= L
    leads.append(R.spikes(L, [10, L // 2, L - 12], [0.9, 1.0, 0.8])); want_in.append([10, L - 12]); want_out.append([])   # clipped QRS windows
    pl = R.spikes(L, [L // 4, L // 2], [1.0, 0.9]); pl[L - 5:] = 1.0                                                  # a plateau to the last sample: no peak
    leads.append(pl); want_in.append([L // 4, L // 2]); want_out.append(list(range(L - 6, L)))
    b = chunk * (L // (2 * chunk))
    st = R.spikes(L, [L // 5], [0.8]); st[b - 2:b + 3] = 1.0                                                          # a plateau over a lane boundary
    leads.append(st); want_in.append([b]); want_out.append([])
    for s, inside, outside in zip(leads, want_in, want_out):
        peaks = list(R.lead_features(s)[1])
        assert all(p in peaks for p in inside) and not any(p in peaks for p in outside), (peaks, inside, outside)
        assert R.tied_candidates(s) <= 1
    assert list(R.lead_features(leads[1])[1])[-1] + 20 >= L
    _check_features(_record(leads, L))


def test_features_most_peaks():
    """Spacing 50 on samples 1 .. 4998 allows 100 kept peaks (1, 51, .. 4951: a 101st would need sample 5001); then twice as many candidates."""
    L = 5000
    rng = np.random.default_rng(50)
    full = R.spikes(L, 1 + 50 * np.arange(100), rng.permutation(np.linspace(0.6, 1.0, 100)))
    assert len(R.lead_features(full)[1]) == 100
    dense = R.spikes(L, 1 + 25 * np.arange(199), rng.permutation(np.linspace(0.6, 1.0, 199)))
    assert 50 <= len(R.lead_features(dense)[1]) <= 100
    _check_features(_record([full, dense], L))


def test_features_amplitude():
    x = synth.synth_ecg(2, 2500, seed=21)
    for y in (x * 1e-3, x * 3e4, x + 1000.0):
        _check_features(y)


@pytest.mark.parametrize("step", [0.005, 0.001])
def test_features_quantised_ties(step):
    """Equal candidate heights: the project's rule (later position first, lead_features(peaks="stable")), not numpy's default argsort order."""
    x = np.round(synth.synth_ecg(20, 2500, seed=1) / step) * step
    tied = sum(R.tied_candidates(s) > 1 for s in x.reshape(-1, 2500))
    assert tied >= 100, tied                               # 230 of 240 leads at 0.005, 106 at 0.001
    _check_features(x, peaks="stable")


def test_features_many_equal_heights():
    L, counts = 2500, [17, 18, 25, 33, 40, 57, 64, 80, 99, 110, 118, 119]
    leads = [R.equal_height_lead(L, c, seed=c) for c in counts]
    assert [R.tied_candidates(s) for s in leads] == counts
    _check_features(_record(leads, L), peaks="stable")


@pytest.mark.parametrize("L", [250, 1000, 1024, 2500, 4999])
def test_features_flat_leads(L):
    """The project's rule for a constant lead: values 7 .. 10 are exactly 0.  The reference's are rounding noise (asserted: its powers lie below the
    power tolerance), its 'centroid' the Hann window's own, fstep / 3 for the non-dyadic constants."""
    consts = [0.1, -3.3, 1e-7]
    x = _record([np.full(L, c) for c in consts], L)
    got, flags = M.features(torch.from_numpy(x).cuda())
    got = got.cpu().numpy().reshape(12, 24)
    assert not flags.any()
    for l, c in enumerate(consts):
        assert R.flat_lead_rule(x[0, l])
        want, peaks = R.lead_features(x[0, l])
        scale = abs(c)
        assert len(peaks) == 0
        assert abs(want[7]) < 1e-11 * scale ** 2 and abs(want[8]) < 1e-11 * scale ** 2, (c, want[7], want[8])
        assert all(got[l, q] == 0.0 for q in (7, 8, 9, 10)), (c, got[l, 7:11])
        for q in R.EXACT:
            if q != 9:
                assert got[l, q] == want[q], (c, q, got[l, q], want[q])
        for q in R.SUMS:
            if q not in (7, 8, 10):
                assert abs(got[l, q] - want[q]) <= 1e-11 * abs(want[q]) + 1e-11 * scale, (c, q, got[l, q], want[q])
    _check_features(np.concatenate([x[:, 3:], x[:, 3:6]], axis=1))   # the random leads beside them


def test_features_batch_above_launch_size():
    n = M._BATCH + 1
    x = synth.synth_ecg(n, 250, seed=5)
    bad = [700, n - 1]
    x[700, 3, 17] = np.nan
    x[n - 1, 11, 249] = np.inf
    xd = torch.from_numpy(x).cuda()
    got, flags = M.features(xd)
    assert torch.nonzero(flags).flatten().tolist() == bad
    for r in range(n):
        one, f1 = M.features(xd[r:r + 1])
        assert int(f1[0]) == (r in bad)
        if r not in bad:
            assert torch.equal(one[0], got[r]), r


def test_load_features_batches_and_errors(tmp_path, monkeypatch):
    monkeypatch.setattr(M, "_BATCH", 64)
    recs = synth.synth_ecg(150, 250, seed=8)
    paths = []
    for i, r in enumerate(recs):
        paths.append(str(tmp_path / f"r{i:03d}.npy"))
        np.save(paths[-1], r)
    F = M.load_features(paths, workers=4)
    assert torch.equal(F, M.features(torch.from_numpy(recs).cuda())[0])             # three launches, the input order kept
    perm = np.random.RandomState(0).permutation(150)
    assert torch.equal(M.load_features([paths[i] for i in perm], workers=3), F[torch.from_numpy(perm).cuda()])
    r = recs[140].copy(); r[5, 100] = np.nan
    np.save(tmp_path / "nan.npy", r)
    with pytest.raises(ValueError, match=r"nan\.npy: the record holds a NaN or an infinity"):
        M.load_features(paths[:140] + [str(tmp_path / "nan.npy")] + paths[141:])    # in the third batch
    np.save(tmp_path / "short.npy", recs[0][:, :200])
    with pytest.raises(ValueError, match=r"short\.npy: expected a \(12, L\) record with the same L"):
        M.load_features(paths[:130] + [str(tmp_path / "short.npy")])
    np.save(tmp_path / "leads.npy", recs[0][:11])
    with pytest.raises(ValueError, match=r"leads\.npy: expected a \(12, L\) record"):
        M.load_features([str(tmp_path / "leads.npy")] + paths[:3])
    np.save(tmp_path / "flat.npy", recs[0].ravel())
    with pytest.raises(ValueError, match=r"flat\.npy: expected a \(12, L\) record"):
        M.load_features(paths[:70] + [str(tmp_path / "flat.npy")])
    with pytest.raises(ValueError, match="no .npy records"):
        M.load_features([])


# ---- k-means ----------------------------------------------------------------------------------------------------------------------------------
def _check_kmeans(X, ks, **kw):
    """Labels equal kmeans_ref's, inertia within 1e-10 relative; the input is tie-free at the reference's final centers.  Returns the stop reasons."""
    fits = M.kmeans_many(torch.from_numpy(X).cuda(), ks, **kw)
    reasons = set()
    for k in ks:
        ref = R.kmeans_ref(X, k, **kw)
        assert R.tie_free_centers(ref["Xc"], ref["centers"]), (X.shape, k)
        assert sum(r["relocations"] for r in ref["runs"]) == 0
        labels, inertia = fits[k]
        assert np.array_equal(labels.cpu().numpy(), ref["labels"]), (X.shape, k, kw)
        assert abs(inertia - ref["inertia"]) <= 1e-10 * ref["inertia"], (X.shape, k, kw, inertia, ref["inertia"])
        reasons |= {r["stop"] for r in ref["runs"]}
    return reasons


def test_kmeans_cli_size():
    """n = 10001 records, k up to 200 (T = 2 .. 7 trials per seeding step), D = 24, one batch of 30 runs."""
    _check_kmeans(R.blobs_n(10001, 24, 0, n_blobs=40), [2, 7, 200])


@pytest.mark.parametrize("D", [5, 40, 288])
def test_kmeans_dimensions(D):
    _check_kmeans(R.blobs_n(600, D, 0), [3, 9])


@pytest.mark.parametrize("n", [5, 6, 37, 1023, 1025])
def test_kmeans_point_counts_around_the_seeding_chunks(n):
    """n = k, k + 1 and either side of the seeding kernels' 1024 lanes."""
    _check_kmeans(R.blobs_n(n, 3, 0), [5])


def test_kmeans_one_cluster():
    _check_kmeans(R.blobs_n(600, 3, 0), [1])
    _check_kmeans(R.blobs_n(600, 3, 0), [1, 4])


def test_kmeans_stop_paths():
    X = R.blobs_n(3000, 6, 0)
    reasons = set()
    for mi in (1, 2, 5):
        reasons |= _check_kmeans(X, [12], max_iter=mi)
    reasons |= _check_kmeans(X, [12], tol=0.5)
    assert {R.TOL, R.MAX_ITER} <= reasons, reasons          # both early stops (and their extra E-step) were entered


@pytest.mark.parametrize("kw", [{}, {"max_iter": 5}, {"tol": 0.5}])
def test_kmeans_sync_interval_changes_nothing(kw):
    X = torch.from_numpy(R.blobs_n(3000, 6, 0)).cuda()
    base = M.kmeans_many(X, [3, 12], sync_every=8, **kw)
    for se in (1, 3, 300):
        fits = M.kmeans_many(X, [3, 12], sync_every=se, **kw)
        for k in (3, 12):
            assert torch.equal(fits[k][0], base[k][0]) and fits[k][1] == base[k][1], (kw, se, k)


@pytest.mark.parametrize("n_loc,copies,k", [(16, 20, 17), (16, 20, 24), (40, 5, 40)])
def test_kmeans_fewer_locations_than_clusters(n_loc, copies, k):
    """The relocation of emptied clusters is reached only with fewer distinct rows than clusters, where every distance ties and sklearn's argpartition
    order is arbitrary: no parity claim, invariants instead."""
    X, which = R.repeated_locations(n_loc, copies, 3, 0)
    if n_loc < k:
        assert sum(r["relocations"] for r in R.kmeans_ref(X, k)["runs"]) > 0       # the restatement (the kernel's tie rule) does relocate here
    Xd = torch.from_numpy(X).cuda()
    labels, inertia = M.kmeans(Xd, k)
    lab = labels.cpu().numpy()
    assert lab.min() >= 0 and lab.max() < k
    assert all(len(set(lab[which == l])) == 1 for l in range(n_loc))
    assert 0.0 <= inertia <= 1e-10 * float((X * X).sum())
    again, inertia2 = M.kmeans(Xd, k)
    assert torch.equal(again, labels) and inertia2 == inertia


# ---- silhouette -------------------------------------------------------------------------------------------------------------------------------
def _check_silhouette(X, labels, idx, tol=1e-9):
    got = M.silhouette_subset(torch.from_numpy(X).cuda(), torch.from_numpy(labels).cuda(), idx)
    want = float(np.mean(R.silhouette_ref(X[idx], labels[idx])))
    assert abs(got - want) <= tol, (got, want)


@pytest.mark.parametrize("D", [1, 40, 288])
@pytest.mark.parametrize("m", [3, 255, 257])
def test_silhouette_subset_sizes(m, D):
    X = R.blobs_n(400, D, 1)
    rng = np.random.default_rng([m, D])
    labels = rng.integers(0, 6, size=400)
    idx = rng.permutation(400)[:m]
    labels[idx[:3]] = [0, 1, 1]                            # at least two labels, fewer than m
    if m == 3:
        labels[idx] = [0, 1, 1]
    _check_silhouette(X, labels, idx)


def test_silhouette_singletons_and_absent_labels():
    X = R.blobs_n(900, 5, 2)
    rng = np.random.default_rng(2)
    labels = rng.integers(0, 7, size=900)
    labels[[10, 20, 30]] = [7, 8, 9]                       # singleton clusters
    idx = np.flatnonzero(labels != 3)                      # label 3 is in `labels`, not in the subset
    idx = idx[rng.permutation(len(idx))[:600]]
    idx = np.unique(np.concatenate([idx, [10, 20, 30]]))
    sub = labels[idx]
    assert 3 not in sub and all((sub == s).sum() == 1 for s in (7, 8, 9))
    s = R.silhouette_ref(X[idx], sub)
    assert all(s[sub == q][0] == 0.0 for q in (7, 8, 9))
    _check_silhouette(X, labels, idx)


def test_silhouette_more_labels_than_lanes():
    X = R.blobs_n(2000, 5, 2)
    labels = np.random.default_rng(3).permutation(np.arange(2000) % 300)      # every one of the 300 labels, 6 or 7 points each
    assert len(np.unique(labels)) == 300
    _check_silhouette(X, labels, np.arange(2000))


def test_silhouette_cli_size():
    X = R.blobs_n(10001, 24, 0, n_blobs=40)
    labels = R.kmeans_ref(X, 200, n_init=1)["labels"]
    idx = np.random.RandomState(0).permutation(10001)[:10000]
    assert len(np.unique(labels[idx])) == 200
    _check_silhouette(X, labels, idx)


def test_silhouette_coincident_points():
    """Exact duplicates inside a cluster: the expanded form's sqrt of a cancelled difference is inherent (sklearn shares it).  On the CPU the mean of the
    expanded-form restatement lies 1.22e-10 from the direct one on this input; ten times that is allowed."""
    rng = np.random.default_rng(0)
    X, which = R.repeated_locations(40, 10, 8, 0)
    X = X.copy()
    X[::3] += 0.5 * rng.standard_normal((len(X[::3]), 8))
    labels = which % 5
    _check_silhouette(X, labels, np.arange(len(X)), tol=10 * 1.22e-10)


def test_silhouette_refuses_label_counts():
    X = torch.from_numpy(R.blobs_n(50, 3, 0)).cuda()
    with pytest.raises(ValueError, match="Number of labels is 1"):
        M.silhouette_subset(X, torch.zeros(50, dtype=torch.int64), np.arange(50))
    with pytest.raises(ValueError, match="Number of labels is 20"):
        M.silhouette_subset(X, torch.arange(50), np.arange(20))
    with pytest.raises(ValueError):
        R.silhouette_ref(X.cpu().numpy(), np.zeros(50, dtype=np.int64))


# ---- DBSCAN -----------------------------------------------------------------------------------------------------------------------------------
def _check_dbscan(X, eps=0.5, min_samples=5):
    want = R.dbscan_ref(X, eps, min_samples)               # asserts that no pair lies within 1e-9 of eps
    got = M.dbscan(torch.from_numpy(np.ascontiguousarray(X)).cuda(), eps=eps, min_samples=min_samples).cpu().numpy()
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:10], got[got != want][:10], want[got != want][:10])
    return want


def test_dbscan_all_noise_and_one_cluster():
    rng = np.random.default_rng(0)
    assert (_check_dbscan(rng.uniform(-100, 100, size=(500, 3))) == -1).all()
    assert (_check_dbscan(0.1 * rng.standard_normal((400, 2))) == 0).all()


def test_dbscan_every_point_a_core():
    want = _check_dbscan(R.dbscan_set(3), min_samples=1)
    assert want.min() == 0 and want.max() > 10


def test_dbscan_exact_duplicates():
    X, which = R.repeated_locations(30, 4, 2, 1)           # 4 copies: a location is a cluster only with a neighbouring location
    want = _check_dbscan(X)
    assert (want == -1).any() and want.max() >= 1
    X5, _ = R.repeated_locations(30, 5, 2, 1)              # 5 copies: every location is a core of its own
    assert (_check_dbscan(X5) >= 0).all()


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_dbscan_long_chain(order):
    """3000 cores in a line, each reaching only its two neighbours (min_samples 3: itself and both): the hook / jump passes must carry one label along
    the whole chain whatever the storage order."""
    want = _check_dbscan(R.chain(3000, 0.5, order), min_samples=3)
    assert (want == 0).all()


def test_dbscan_border_shared_by_three_clusters():
    X, row = R.shared_border()
    want = _check_dbscan(X)
    near = np.flatnonzero((((X - X[row]) ** 2).sum(1) <= 0.25) & (np.arange(len(X)) != row))
    assert sorted(want[near]) == [0, 1, 2] and want[row] == 0 and want.max() == 2


def test_dbscan_final_clusters_shape():
    """n = 10001, D = 40, standardised blobs: what final_clusters passes."""
    X = R.blobs_n(10001, 40, 0, n_blobs=8, spread=0.1)
    X = (X - X.mean(0)) / X.std(0)
    want = _check_dbscan(X)
    assert want.max() == 7 and (want == -1).sum() >= 500


@pytest.mark.parametrize("n", [1, 4, 1024, 1025])
def test_dbscan_point_counts(n):
    _check_dbscan(R.blobs_n(n, 2, 4, spread=0.3))
