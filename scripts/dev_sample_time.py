"""Times the sampling step (ecg_byte_amd/morphology.py) on the device with events: features, PCA + scaler, the k-means sweep k = 2 .. max_clusters
(n_init 10) with a silhouette per k, the final fit and DBSCAN.  The batch is resident in HBM, tiled from `--base` synthetic records with a gain per
copy.  The sweep is timed on the real PCA output and on forced dimensions (--force_D: the top D components, scaled).  One JSON line per phase.

    python scripts/dev_sample_time.py --records 200001 --L 2500 --max_clusters 200 --force_D 8 32
    rocprofv3 --kernel-trace --stats -d prof_out -- python scripts/dev_sample_time.py ...   (a separate run for the kernel table)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecg_byte_amd import morphology as M, synth  # noqa: E402


def timed(name, fn, **extra):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    print(json.dumps(dict(phase=name, ms=round(a.elapsed_time(b), 3), wall_ms=round(1e3 * (time.perf_counter() - w), 3), **extra)), flush=True)
    return out


def sweep(X, max_clusters, seed, tag):
    ks = list(range(2, max_clusters + 1))
    fits = timed(f"kmeans_sweep_{tag}", lambda: M.kmeans_many(X, ks), n=X.shape[0], D=X.shape[1], ks=len(ks))
    timed(f"silhouette_{tag}", lambda: [M.silhouette_score(X, fits[k][0], 10000, seed) for k in ks], n=X.shape[0], D=X.shape[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200001)
    ap.add_argument("--L", type=int, default=2500)
    ap.add_argument("--base", type=int, default=256)
    ap.add_argument("--max_clusters", type=int, default=200)
    ap.add_argument("--force_D", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--skip_sweep", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    base = torch.from_numpy(synth.synth_ecg(a.base, a.L, seed=3)).cuda()
    gains = torch.from_numpy(np.random.default_rng(1).uniform(0.5, 2.0, a.records)).cuda()
    x = torch.empty((a.records, 12, a.L), dtype=torch.float64, device="cuda")
    for s in range(0, a.records, a.base):
        e = min(a.records, s + a.base)
        x[s:e] = base[: e - s] * gains[s:e, None, None]
    M.features(x[:16])                                         # load the library, size the kernel
    F, flags = timed("features", lambda: M.features(x), records=a.records, L=a.L, bytes=x.numel() * 8)
    assert not bool(flags.any())
    del x
    X = timed("pca_scale", lambda: M.pca_scale(F))
    print(json.dumps(dict(phase="pca", D=X.shape[1])), flush=True)
    if not a.skip_sweep:
        sweep(X, a.max_clusters, a.seed, f"D{X.shape[1]}")
    timed("dbscan", lambda: M.dbscan(X), n=X.shape[0], D=X.shape[1])
    mean, comp, _ = M.pca_components(F)
    for D in a.force_D:
        if a.skip_sweep:
            break
        c = comp[:D] if comp.shape[0] >= D else None
        if c is None:
            _, vec = torch.linalg.eigh(torch.cov(F.T))
            c = vec.flip(1)[:, :D].T.contiguous()
        Xd = M.standard_scale(F @ c.T).contiguous()
        sweep(Xd, a.max_clusters, a.seed, f"forcedD{D}")


if __name__ == "__main__":
    main()
