"""Mirror of the reference's ecg_byte/utils/tokenizer_utils.py (same names, argument meaning and
return shapes) with the compute on the MI355X.  The plot helper of the reference (track_encoding)
is out of scope.  decode_batch / reconstruct_batch are the batched, on-device
forms of decode_text / reverse_normalize_all (csrc/detokenize.hip).
"""
from __future__ import annotations

import pickle
from collections import Counter

import numpy as np
import torch

from . import rust_bpe
from .tokenizer import HipTokenizer
from .tokenizer import quantize as _quantize_dev

ALPHABET = list("abcdefghijklmnopqrstuvwxyz")          # tokenizer_utils.py:12
_ALPHABET_ARR = np.array(ALPHABET, dtype="<U1")


def normalize_all(signal, percentiles):
    """tokenizer_utils.py:14-19 -> (clipped_normalized float64, symbol_signal '<U1'), same shape.

    Accepts a numpy array (any float dtype; promoted to float64 as NumPy 2 does with the
    float64 percentile scalars) or a CUDA float64 tensor."""
    if isinstance(signal, torch.Tensor):
        x = signal.to(device="cuda", dtype=torch.float64)
    else:
        x = torch.from_numpy(np.ascontiguousarray(signal, dtype=np.float64)).cuda()
    clipped, sym = _quantize_dev(x, percentiles, want_clipped=True)
    return clipped.cpu().numpy(), _ALPHABET_ARR[sym.cpu().numpy()]


def quantize_symbols(signal, percentiles) -> np.ndarray:
    """Alphabet indices (uint8) only -- what every consumer of normalize_all actually uses."""
    x = signal if isinstance(signal, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(signal, dtype=np.float64))
    return _quantize_dev(x.to(device="cuda", dtype=torch.float64), percentiles).cpu().numpy()


def reverse_normalize_all(symbol_signal, percentiles):
    """tokenizer_utils.py:22-28 (not an exact inverse: index/25 * (max-min) + min)."""
    min_vals = percentiles["percentile_1"] - 0.5
    max_vals = percentiles["percentile_99"] + 0.5
    s = np.asarray(symbol_signal)
    idx = (s.view(np.uint32).reshape(s.shape) - ord("a")) if s.dtype.kind == "U" else s
    clipped_normalized = idx.astype(np.float64) / (len(ALPHABET) - 1)
    return clipped_normalized * (max_vals - min_vals) + min_vals


def encode_text(text, merges):
    """tokenizer_utils.py:71-73."""
    return rust_bpe.encode_text(text, merges)


def decode_text(encoded_ids, vocab):
    """tokenizer_utils.py:75-77."""
    return "".join(vocab[i] for i in encoded_ids)


def save_vocab_and_merges(vocab, merges, filename):
    """tokenizer_utils.py:62-64: pickle of the 2-tuple."""
    with open(filename, "wb") as f:
        pickle.dump((vocab, merges), f)


def load_vocab_and_merges(filename):
    """tokenizer_utils.py:66-69."""
    with open(filename, "rb") as f:
        vocab, merges = pickle.load(f)
    return vocab, merges


def process_ecg(ecg, percentiles):
    """tokenizer_utils.py:56-59: path to a (12, L) .npy -> lead-major symbol string."""
    sig = np.load(ecg)
    return (quantize_symbols(sig, percentiles).reshape(-1) + ord("a")).astype(np.uint8).tobytes().decode("ascii")


def process_large_file(file_path, percentiles, num_processes=1, n=None):
    """tokenizer_utils.py:79-93: concatenated symbol strings of the listed .npy files, in file
    order.  `num_processes` is accepted for compatibility; records are quantised on the GPU in
    batches instead of in a process pool."""
    paths = []
    with open(file_path, "r") as f:
        for i, line in enumerate(f):
            if n is not None and i >= n:
                break
            paths.append(line.strip())
    return process_paths(paths, percentiles).decode("ascii")


def process_paths(paths, percentiles) -> bytes:
    """Concatenated symbol bytes ('a'..'z') of the given .npy records, in order; records are quantised on the GPU in batches."""
    parts = []
    batch, shape = [], None
    def flush():
        if batch:
            x = torch.from_numpy(np.stack(batch)).cuda()
            s = _quantize_dev(x, percentiles).cpu().numpy().reshape(-1)
            parts.append((s + ord("a")).astype(np.uint8).tobytes())
            batch.clear()
    for p in paths:
        sig = np.ascontiguousarray(np.load(p), dtype=np.float64)
        if shape is not None and sig.shape != shape:
            flush()
        shape = sig.shape
        batch.append(sig)
        if len(batch) >= 256:
            flush()
    flush()
    return b"".join(parts)


_BATCH = 256        # records per device batch (process_paths)


def _tokenizer_of(merges) -> HipTokenizer:
    return merges if isinstance(merges, HipTokenizer) else HipTokenizer(merges)


def decode_batch(ids, counts, merges):
    """decode_text for a batch, on the device: ids int32 `(B, stride)` and counts int32 `(B,)` (CUDA tensors or arrays, as
    `HipTokenizer.quantize_encode` returns them) -> list of B `bytes`.  `merges` is the reference's list or a HipTokenizer.
    Raises KeyError naming the first id that is not in the vocabulary, as `vocab[id]` would."""
    tk = _tokenizer_of(merges)
    ids = torch.as_tensor(np.asarray(ids) if not isinstance(ids, torch.Tensor) else ids).to(device="cuda", dtype=torch.int32)
    counts = torch.as_tensor(np.asarray(counts) if not isinstance(counts, torch.Tensor) else counts).to(device="cuda", dtype=torch.int32)
    if ids.dim() == 1:
        ids = ids[None]
    out, n_sym, flags = tk.detokenize(ids, counts)
    flags = flags.cpu().numpy()
    if (flags & 1).any():
        lens = tk.expansions()[1]
        b = int(np.flatnonzero(flags & 1)[0])
        row = ids[b, : min(int(counts[b]), ids.shape[1])].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        bad = row[(row >= lens.size) | (lens[np.minimum(row, lens.size - 1)] == 0)]
        raise KeyError(int(bad[0]))
    out, n_sym = out.cpu().numpy(), n_sym.cpu().numpy()
    return [out[b, : n_sym[b]].tobytes() for b in range(out.shape[0])]


def reconstruct_batch(signal, percentiles, merges):
    """Quantise + encode -> detokenise back to signal, against the original, in one pass on the device: the self-check of
    train_tokenizer.py:44-66 for a batch.  signal: `(B, 12, L)` or `(B, n)` float64 (numpy or CUDA tensor).  Returns a list of B
    `(round_trip_ok, max_abs_diff, n_tokens)`: the decoded symbols are the quantised ones and all of them came back; the largest
    |signal - dequantised| (what the reference prints); the record's token count."""
    tk = _tokenizer_of(merges)
    x = signal if isinstance(signal, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(signal, dtype=np.float64))
    x = x.to(device="cuda", dtype=torch.float64).contiguous()
    B = x.shape[0]
    n = x.numel() // B if B else 0
    if B == 0 or n == 0:
        return [(True, 0.0, 0)] * B
    ids, counts = tk.quantize_encode(x, percentiles)
    _, n_sym, flags, diff, mism = tk.detokenize_signal(ids, counts, percentiles, n, original=x)
    n_sym, flags, diff, mism, counts = (t.cpu().numpy() for t in (n_sym, flags, diff, mism, counts))
    return [(bool(n_sym[b] == n and flags[b] == 0 and mism[b] == 0), float(diff[b]), int(counts[b])) for b in range(B)]


def _record_batches(paths):
    """Records of the listed .npy files as float64 batches of equal shape, in order (the batching of process_paths)."""
    batch, shape = [], None
    for p in paths:
        sig = np.ascontiguousarray(np.load(p), dtype=np.float64)
        if batch and (sig.shape != shape or len(batch) >= _BATCH):
            yield np.stack(batch)
            batch = []
        shape = sig.shape
        batch.append(sig)
    if batch:
        yield np.stack(batch)


def analyze_token_distribution(test_data, merges, percentiles, num_workers=None):
    """tokenizer_utils.py analyze_token_distribution: `(Counter of token ids over the test set, [token count of each record])`.
    test_data: paths of (12, L) .npy records.  `num_workers` is accepted for compatibility; records are encoded on the GPU in
    batches and counted there (ecgb_token_histogram_hip)."""
    tk = _tokenizer_of(merges)
    total, lengths = None, []
    for x in _record_batches(list(test_data)):
        ids, counts = tk.quantize_encode(torch.from_numpy(x).cuda(), percentiles)
        hist, over = tk.token_histogram(ids, counts)
        assert int(over) == 0, "the encoder emitted an id outside the tokenizer's id range"
        total = hist if total is None else total + hist
        lengths.extend(int(c) for c in counts.cpu().numpy())
    token_counts = Counter()
    if total is not None:
        total = total.cpu().numpy()
        token_counts.update({int(k): int(total[k]) for k in np.flatnonzero(total)})
    return token_counts, lengths
