"""python -m ecg_byte_amd.sample_ecg --unseg_dir D --max_clusters 200 --n_samples 200000: the reference's preprocess/sample_ecg.py on the device.

Writes {data_root}/sampled_ecg_files_{n_samples}.txt (one path per line: what `train_tokenizer --sampled_files` reads) and, instead of the
reference's PNG, {data_root}/cluster_analysis.json.  --seed seeds the silhouette subsample and the stratified draw (see ecg_byte_amd/morphology.py
for the deliberate differences); --workers sizes the file-reading threads."""
import argparse
import json
import os

from . import morphology as M


def get_args(argv=None):
    parser = argparse.ArgumentParser(description=None)
    parser.add_argument('--unseg_dir', type=str, default=None, help='Please specify the path to the unsegmented ecgs')
    parser.add_argument('--max_clusters', type=int, default=200, help='Please choose the maximum number of clusters to consider')
    parser.add_argument('--n_samples', type=int, default=200000, help='Please choose the number of samples to consider')
    parser.add_argument('--data_root', type=str, default='./data', help='where the sampled list and cluster_analysis.json go')
    parser.add_argument('--seed', type=int, default=0, help='seed of the silhouette subsample and the stratified draw')
    parser.add_argument('--workers', type=int, default=None, help='file-reading threads')
    return parser.parse_args(argv)


def main(args):
    os.makedirs(args.data_root, exist_ok=True)
    print("Analyzing ECG morphologies...")
    report = {}
    file_paths, clusters, n_clusters = M.analyze_morphologies(args.unseg_dir, args.max_clusters, args.n_samples, seed=args.seed,
                                                              workers=args.workers, report=report)
    print(f"Optimal number of clusters: {n_clusters}")
    print("Performing stratified sampling...")
    sampled_files = M.stratified_sampling(file_paths, clusters, args.n_samples, seed=args.seed)
    print(f"Sampled {len(sampled_files)} files.")
    out = os.path.join(args.data_root, f"sampled_ecg_files_{args.n_samples}.txt")
    with open(out, "w") as f:
        for file in sampled_files:
            f.write(f"{file}\n")
    js = os.path.join(args.data_root, "cluster_analysis.json")
    with open(js, "w") as f:
        json.dump(report, f, indent=1)
    print(f"Sampling complete. Sampled file list saved to '{out}'.")
    print(f"Cluster analysis saved as '{js}'.")
    return out


if __name__ == "__main__":
    main(get_args())
