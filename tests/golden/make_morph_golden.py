"""Writes tests/golden/morph_golden.npz: what numpy, scipy and sklearn answer for the sampling step (ecg_byte_amd/morphology.py), each called with
the reference's arguments (ecg_byte/utils/preprocess_utils.py:259-462).  The inputs are regenerated from seeds by tests/morph_ref.py, not stored.

    python tests/golden/make_morph_golden.py        (needs sklearn and scipy; run from the repository root)
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import morph_ref as R  # noqa: E402
from sklearn.cluster import DBSCAN, KMeans  # noqa: E402
from sklearn.decomposition import PCA  # noqa: E402
from sklearn.metrics import silhouette_score  # noqa: E402
from sklearn.preprocessing import StandardScaler  # noqa: E402

KS = (2, 3, 8, 17)
DS = (1, 3, 8)
NEAR = 1e-9


def tie_free_kmeans(X, km):
    """No point whose two nearest final centers lie within NEAR (relative) of each other."""
    d = ((X[:, None, :] - km.cluster_centers_[None]) ** 2).sum(-1)
    d.sort(1)
    return bool(np.all(d[:, 1] - d[:, 0] > NEAR * np.maximum(d[:, 1], 1e-300)))


def main():
    out = {}
    for D in DS:
        for seed in range(100):
            X = R.blobs(D, seed)
            fits = {k: KMeans(n_clusters=k, random_state=42, n_init=10).fit(X) for k in KS}
            if all(tie_free_kmeans(X, fits[k]) for k in KS):
                break
        else:
            raise SystemExit(f"no tie-free seed for D={D}")
        out[f"blobs_seed_D{D}"] = np.int64(seed)
        for k in KS:
            out[f"km_labels_D{D}_k{k}"] = fits[k].labels_.astype(np.int16)
            out[f"km_inertia_D{D}_k{k}"] = np.float64(fits[k].inertia_)
        for k in (2, 3, 8):
            for s in (0, 5):
                idx = np.random.RandomState(s).permutation(len(X))[:700]
                out[f"sil_D{D}_k{k}_s{s}"] = np.float64(silhouette_score(X[idx], fits[k].labels_[idx]))
                assert np.isclose(out[f"sil_D{D}_k{k}_s{s}"], silhouette_score(X, fits[k].labels_, sample_size=700, random_state=s), rtol=1e-12)
    Y = R.dbscan_set(0)
    d = np.sqrt(((Y[:, None] - Y[None]) ** 2).sum(-1))
    assert not np.any(np.abs(d - 0.5) < NEAR), "a pair distance lies at eps"
    db = DBSCAN(eps=0.5, min_samples=5).fit(Y)
    core = np.zeros(len(Y), bool)
    core[db.core_sample_indices_] = True
    border = 310
    nb = np.flatnonzero((d[border] <= 0.5) & core)
    assert not core[border] and len(set(db.labels_[nb])) == 2 and db.labels_[border] == min(db.labels_[nb]), "the border point must touch two clusters"
    assert (db.labels_ == -1).any()
    out["dbscan_labels"] = db.labels_.astype(np.int16)

    # end to end on synthetic records, in a fixed path order, with the CLI's seeding rules (seed 0)
    recs = R.e2e_records()
    F = np.stack([R.extract_features(r) for r in recs])
    X = StandardScaler().fit_transform(PCA(n_components=0.95).fit_transform(F))
    out["e2e_D"] = np.int64(X.shape[1])
    ks = list(range(2, R.E2E_MAX_CLUSTERS + 1))
    fits = [KMeans(n_clusters=k, random_state=42, n_init=10).fit(X) for k in ks]
    inert = [f.inertia_ for f in fits]
    sils = [silhouette_score(X, f.labels_, sample_size=10000, random_state=0) for f in fits]
    elbow = int(np.argmin(np.diff(inert))) + 2
    best = sils.index(max(sils)) + 2
    k = min(elbow, best)
    labels = KMeans(n_clusters=k, random_state=42, n_init=10).fit_predict(X)
    ran = len(np.unique(labels)) < 3
    if ran:
        labels = DBSCAN(eps=0.5, min_samples=5).fit_predict(X)
    names = R.e2e_names()
    rng = random.Random(0)
    per = R.E2E_N_SAMPLES // len(np.unique(labels))
    sampled = []
    for c in np.unique(labels):
        files = [names[i] for i in range(len(names)) if labels[i] == c]
        sampled.extend(rng.sample(files, min(per, len(files))))
    rem = R.E2E_N_SAMPLES - len(sampled)
    if rem > 0:
        taken = set(sampled)
        rest = [f for f in names if f not in taken]
        sampled.extend(rng.sample(rest, min(rem, len(rest))))
    out.update(e2e_k=np.int64(k), e2e_elbow=np.int64(elbow), e2e_best_sil=np.int64(best), e2e_dbscan=np.bool_(ran),
               e2e_labels=labels.astype(np.int16), e2e_sampled=np.array(sampled), e2e_inertia=np.array(inert), e2e_sil=np.array(sils))
    path = os.path.join(ROOT, "tests", "golden", "morph_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; e2e: D", X.shape[1], "k", k, "dbscan", ran, "clusters", np.unique(labels))


if __name__ == "__main__":
    main()
