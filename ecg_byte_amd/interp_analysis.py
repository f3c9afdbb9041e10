"""Mirror of ecg_byte/interp_analysis.py (the attention-interpretation CLI): load a trained checkpoint, run
`runners.interpreter` over the test split at batch 1 and save what it returns.

    python -m ecg_byte_amd.interp_analysis --model <dir> --tokenizer_check tokenizer_3500_100_mimic2 --batch_size=1 --pad_to_max=2046 \
        --toy --peft --num_merges=3500 --bins=100 --percentiles=<stats.npy> --checkpoint <run dir> --dataset ptb_qa --interpret

Differences from the reference, all deliberate: the options are main.py's plus the reference script's `--bins` (accepted, unused
there and here); `--data_root` / `--runs_root` / `--workers` as in main.py; the dataset is ECGTokenDataset in its training-item form
(the reference names a class that does not exist); no hub login; the plots are not built -- the result is written to
`{runs_root}/{seed}/{checkpoint}/interpret_{dataset}.npz` with one array per sample and component (`signal/attentions/3`,
`question/sequences/0`, `signal/signal/1` for the decoded symbols, ...)."""
from __future__ import annotations

import argparse
import gc
import random

import numpy as np
import torch


def get_args(argv=None):
    """interp_analysis.py:21-48, plus --bins (scripts/interpret.sh) and --data_root / --runs_root / --workers."""
    p = argparse.ArgumentParser(description=None)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--epochs", type=int, default=150)
    p.add_argument("--device", type=str, default=None)
    p.add_argument("--dataset", type=str, default="mimic_500")
    p.add_argument("--model", type=str, default=None)
    p.add_argument("--beta1", type=float, default=0.9)
    p.add_argument("--beta2", type=float, default=0.99)
    p.add_argument("--eps", type=float, default=1e-8)
    p.add_argument("--warmup", type=int, default=500)
    p.add_argument("--weight_decay", type=float, default=1e-2)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--patience", type=int, default=5)
    p.add_argument("--dev", action="store_true")
    p.add_argument("--inference", action="store_true")
    p.add_argument("--interpret", action="store_true")
    p.add_argument("--checkpoint", type=str)
    p.add_argument("--log", action="store_true")
    p.add_argument("--tokenizer_check", type=str)
    p.add_argument("--num_merges", type=int, default=1000)
    p.add_argument("--pad_to_max", type=int, default=1000)
    p.add_argument("--toy", action="store_true")
    p.add_argument("--peft", action="store_true", default=None)
    p.add_argument("--percentiles", type=str, default=None)
    p.add_argument("--bins", type=int, default=None)
    p.add_argument("--data_root", type=str, default="./data")
    p.add_argument("--runs_root", type=str, default="./runs")
    p.add_argument("--workers", type=int, default=4, help="reader threads of the batch loader")
    return p.parse_args(argv)


def save_result(result, path):
    """The interpreter's dict as one .npz: key `{component}/{field}/{sample}`."""
    arrays = {}
    for component, fields in result.items():
        for field, items in fields.items():
            for k, v in enumerate(items):
                arrays[f"{component}/{field}/{k}"] = np.asarray(v)
    np.savez(path, **arrays)
    return path


def main(argv=None):
    """interp_analysis.py:50-145"""
    from .data_loader import DeviceBatchLoader, ECGTokenDataset
    from .file_utils import align_signal_text_files, load_vocab_and_merges, sample_N_percent_from_lists
    from .main import build_model_and_tokenizer
    from .runners import interpreter
    args = get_args(argv)
    device = torch.device(args.device or "cuda:0")
    if device.type == "cuda":
        torch.cuda.set_device(device)           # ctypes-launched kernels go to the current device's current stream
    if args.dev:
        args.epochs = 2
    gc.collect()
    random.seed(args.seed)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    vocab, merges = load_vocab_and_merges(f"{args.data_root}/{args.tokenizer_check}.pkl")
    model, tokenizer = build_model_and_tokenizer(args, vocab, device)
    data = f"{args.data_root}/{args.dataset}"
    test_signals, test_texts = align_signal_text_files(f"{data}/ecg/test", f"{data}/text/test")
    if args.toy:
        test_signals, test_texts = sample_N_percent_from_lists(test_signals, test_texts, 0.25)
    test_data = ECGTokenDataset(test_signals, test_texts, vocab, merges, args=args, tokenizer=tokenizer)
    test_loader = DeviceBatchLoader(test_data, batch_size=1, workers=args.workers)
    ckpt_dir = f"{args.runs_root}/{args.seed}/{args.checkpoint}"
    print(f"Interpreting {args.checkpoint}")
    checkpoint = torch.load(f"{ckpt_dir}/best_model.pth", map_location=device)
    model.load_state_dict(checkpoint["model"])
    print("Model Loaded")
    out = interpreter(model, test_loader, tokenizer, vocab, args)
    path = save_result(out, f"{ckpt_dir}/interpret_{args.dataset}.npz")
    print(f"{len(out['signal']['attentions'])} samples -> {path}")
    print("Interpretation Complete")
    return out


if __name__ == "__main__":
    main()
