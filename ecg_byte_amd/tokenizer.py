"""Device tokenizer handle: the trie the reference rebuilds inside every
`rust_bpe.encode_text` call (ecg_byte/rust_bpe/src/lib.rs:153-161) is built once here and kept
in HBM; batches of ECG records are quantised and encoded on the GPU.

torch is used for device memory and streams only; all compute goes through the C ABI.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


def flatten_merges(merges):
    """[(list[int] expansion, int id), ...] -> (flat u32, offsets u32[n+1], ids u32[n])."""
    n = len(merges)
    lens = np.fromiter((len(m[0]) for m in merges), dtype=np.int64, count=n)
    offsets = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum(lens, out=offsets[1:])
    flat = np.empty(int(offsets[-1]), dtype=np.uint32)
    ids = np.empty(n, dtype=np.uint32)
    for i, (seq, tid) in enumerate(merges):
        flat[offsets[i]:offsets[i + 1]] = seq
        ids[i] = tid
    return flat, offsets, ids


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def set_encode_plan(mode: int) -> None:
    """0 = automatic, 1 = workgroup-per-stream kernel, 2 / 3 = wave-per-stream kernel, 4 = lane-per-chunk kernel (encode_long_kernel; opt-in), 6 = the same with stager and walker waves in one workgroup (encode_pipe_kernel) (tests/tuning)."""
    _lib.check(_lib.lib().ecgb_set_encode_plan(int(mode)))


class HipTokenizer:
    """Immutable device tokenizer built from the reference's `merges` list."""

    def __init__(self, merges):
        L = _lib.lib()
        flat, offsets, ids = flatten_merges(merges)
        if torch.cuda.is_available():
            torch.cuda.current_device()  # make torch's device/context current before the upload
            torch.zeros(1, device="cuda")
        h = C.c_void_p()
        u32p = C.POINTER(C.c_uint32)
        _lib.check(L.ecgb_tokenizer_create(flat.ctypes.data_as(u32p), offsets.ctypes.data_as(u32p),
                                           ids.ctypes.data_as(u32p), len(merges), C.byref(h)))
        self._h = h
        self.n_merges = len(merges)
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _lib.check(L.ecgb_tokenizer_info(h, C.byref(a), C.byref(b), C.byref(c)))
        self.n_nodes, self.max_depth, self.n_classes = a.value, b.value, c.value
        self._scratch = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().ecgb_tokenizer_destroy(h)
            except Exception:
                pass
            self._h = None

    def nodes(self) -> np.ndarray:
        """Packed trie nodes (host copy): bitmap | first_child<<32 | token<<48."""
        out = np.empty(self.n_nodes, dtype=np.uint64)
        _lib.lib().ecgb_tokenizer_copy_nodes(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size)
        return out

    # ---- device paths -------------------------------------------------------------------
    def _get_scratch(self, batch: int, n: int, device) -> torch.Tensor:
        need = _lib.lib().ecgb_encode_scratch_bytes(self._h, batch, n)
        key = (device.index, torch.cuda.current_stream().cuda_stream)
        buf = self._scratch.get(key)
        if buf is None or buf.numel() < need:
            buf = torch.empty(need, dtype=torch.uint8, device=device)
            self._scratch[key] = buf
        return buf

    def quantize_encode(self, signal: torch.Tensor, percentiles, ids_stride: int | None = None,
                        out: tuple | None = None):
        """Quantise + encode a batch of records (reference: data_loader.py:74-76 per sample).

        signal: CUDA float64 tensor `(B, 12, L)` or `(B, n)`, C-contiguous.
        Returns `(ids, counts)`: int32 `(B, ids_stride)` and int32 `(B,)`; record b's tokens are
        `ids[b, :counts[b]]` (entries past `counts[b]` are unspecified).  `ids_stride`
        defaults to the worst case n (one token per symbol); tokens past it are dropped.
        """
        if not (isinstance(signal, torch.Tensor) and signal.is_cuda):
            raise TypeError("quantize_encode needs a CUDA tensor (no CPU fallback)")
        if signal.dtype != torch.float64:
            raise TypeError("signal must be float64 (the reference quantises in float64)")
        _lib.require_current(signal.device)
        if not signal.is_contiguous():
            signal = signal.contiguous()
        B = signal.shape[0]
        n = signal.numel() // B if B else 0
        stride = int(ids_stride) if ids_stride else max(1, n)
        if out is None:
            ids = torch.empty((B, stride), dtype=torch.int32, device=signal.device)
            counts = torch.empty((B,), dtype=torch.int32, device=signal.device)
        else:
            ids, counts = out
        if B == 0:
            return ids, counts
        scratch = self._get_scratch(B, n, signal.device)
        _lib.check(_lib.lib().ecgb_quantize_encode_hip(
            self._h, _ptr(signal), B, n, float(percentiles["percentile_1"]),
            float(percentiles["percentile_99"]), _ptr(ids), stride, _ptr(counts), _ptr(scratch),
            scratch.numel(), _stream_ptr()))
        return ids, counts

    def encode_bytes(self, text: torch.Tensor, ids_stride: int | None = None):
        """Encode a batch of raw byte streams: CUDA uint8 `(B, n)` -> `(ids, counts)`."""
        if not (isinstance(text, torch.Tensor) and text.is_cuda and text.dtype == torch.uint8):
            raise TypeError("encode_bytes needs a CUDA uint8 tensor (no CPU fallback)")
        _lib.require_current(text.device)
        if text.dim() == 1:
            text = text[None]
        text = text.contiguous()
        B, n = text.shape
        stride = int(ids_stride) if ids_stride else max(1, n)
        ids = torch.empty((B, stride), dtype=torch.int32, device=text.device)
        counts = torch.empty((B,), dtype=torch.int32, device=text.device)
        if B == 0:
            return ids, counts
        scratch = self._get_scratch(B, n, text.device)
        _lib.check(_lib.lib().ecgb_encode_hip(self._h, _ptr(text), B, n, _ptr(ids), stride, _ptr(counts),
                                              _ptr(scratch), scratch.numel(), _stream_ptr()))
        return ids, counts

    # ---- detokenise: the inverse direction (csrc/detokenize.hip) ---------------------------------
    def expansions(self):
        """Host copy of the expansion table: `(offsets u32[n_ids], lens u32[n_ids], bytes u8[n_bytes])`; id k stands for
        `bytes[offsets[k]:offsets[k] + lens[k]]`, length 0 = not in the vocabulary."""
        L = _lib.lib()
        n_ids = L.ecgb_tokenizer_copy_expansions(self._h, None, None, 0, None, 0)
        n_bytes = L.ecgb_tokenizer_expansion_bytes(self._h)
        off, lens = np.empty(n_ids, dtype=np.uint32), np.empty(n_ids, dtype=np.uint32)
        raw = np.empty(n_bytes, dtype=np.uint8)
        u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        L.ecgb_tokenizer_copy_expansions(self._h, off.ctypes.data_as(u32p), lens.ctypes.data_as(u32p), n_ids, raw.ctypes.data_as(u8p), n_bytes)
        return off, lens, raw

    def _check_ids(self, ids, counts, who):
        if not (isinstance(ids, torch.Tensor) and ids.is_cuda and isinstance(counts, torch.Tensor) and counts.is_cuda):
            raise TypeError(f"{who} needs CUDA tensors (no CPU fallback)")
        if ids.dtype != torch.int32 or counts.dtype != torch.int32:
            raise TypeError("ids and counts must be int32, as quantize_encode returns them")
        if ids.dim() != 2 or counts.dim() != 1 or counts.shape[0] != ids.shape[0] or ids.stride(1) != 1 and ids.shape[1] > 1:
            raise ValueError("ids must be (B, ids_stride) with unit inner stride and counts (B,)")
        _lib.require_current(ids.device)
        return ids if ids.is_contiguous() else ids.contiguous(), counts.contiguous()

    def _exp_lens_dev(self, device):
        lens = getattr(self, "_exp_lens", None)
        if lens is None or lens.device != device:
            lens = torch.from_numpy(self.expansions()[1].astype(np.int64)).to(device)
            self._exp_lens = lens
        return lens

    def expanded_lengths(self, ids, counts) -> torch.Tensor:
        """Symbols each record expands to (int64 `(B,)`, on the device): one gather of the length table and a masked row sum."""
        ids, counts = self._check_ids(ids, counts, "expanded_lengths")
        lens = self._exp_lens_dev(ids.device)
        valid = torch.arange(ids.shape[1], device=ids.device)[None, :] < counts[:, None]
        idx = ids.long() & 0xFFFFFFFF
        known = valid & (idx < lens.numel())
        return torch.where(known, lens[torch.where(known, idx, torch.zeros_like(idx))], torch.zeros_like(idx)).sum(dim=1)

    def _out_stride(self, ids, counts, out_stride):
        if out_stride is not None:
            if int(out_stride) < 1:
                raise ValueError("out_stride must be at least 1")
            return int(out_stride)
        return max(1, int(self.expanded_lengths(ids, counts).max())) if ids.shape[0] else 1

    def detokenize(self, ids, counts, out_stride: int | None = None, out: torch.Tensor | None = None):
        """Token ids back to symbol bytes (reference: tokenizer_utils.py:75-77 decode_text, for a batch).

        ids, counts: what `quantize_encode` / `encode_bytes` return.  Returns `(bytes, n_sym, flags)`: uint8 `(B, out_stride)`, int32 `(B,)`, int32
        `(B,)`; record b's text is `bytes[b, :n_sym[b]]`, the rest of the row is left as it was (zeros when the row is allocated here).  flags: bit 0 an id
        without expansion was met (skipped), bit 1 the row was cut at out_stride.  `out_stride` defaults to the longest expansion of the batch, which costs
        one small reduction and a host read; pass it where it is known (12 * L for encoded records)."""
        ids, counts = self._check_ids(ids, counts, "detokenize")
        stride = self._out_stride(ids, counts, out_stride)
        B = ids.shape[0]
        if out is None:
            out = torch.zeros((B, stride), dtype=torch.uint8, device=ids.device)
        n_sym = torch.zeros((B,), dtype=torch.int32, device=ids.device)
        flags = torch.zeros((B,), dtype=torch.int32, device=ids.device)
        if B:
            _lib.check(_lib.lib().ecgb_detokenize_hip(self._h, _ptr(ids), ids.shape[1], _ptr(counts), B, _ptr(out), stride, _ptr(n_sym),
                                                      _ptr(flags), _stream_ptr()))
        return out, n_sym, flags

    def expand(self, ids, counts, values, out_stride: int, out: torch.Tensor | None = None):
        """One value per token spread over the symbols the token covers (the interpret run's expand_attention, for a batch): `values` float32
        `(B, ids_stride)` -> `(expanded float32 (B, out_stride), n_sym, flags)`; bits pass untouched."""
        ids, counts = self._check_ids(ids, counts, "expand")
        if not (isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float32 and values.shape == ids.shape):
            raise TypeError("values must be a CUDA float32 tensor of the shape of ids")
        values = values.contiguous()
        stride = self._out_stride(ids, counts, out_stride)
        B = ids.shape[0]
        if out is None:
            out = torch.zeros((B, stride), dtype=torch.float32, device=ids.device)
        n_sym = torch.zeros((B,), dtype=torch.int32, device=ids.device)
        flags = torch.zeros((B,), dtype=torch.int32, device=ids.device)
        if B:
            _lib.check(_lib.lib().ecgb_detokenize_values_f32_hip(self._h, _ptr(ids), ids.shape[1], _ptr(counts), B, _ptr(values), _ptr(out), stride,
                                                                 _ptr(n_sym), _ptr(flags), _stream_ptr()))
        return out, n_sym, flags

    def detokenize_signal(self, ids, counts, percentiles, out_stride: int, original: torch.Tensor | None = None, out: torch.Tensor | None = None):
        """Token ids back to the dequantised signal (decode_text + reverse_normalize_all, tokenizer_utils.py:22-28; the bits numpy gives).

        Returns `(signal float64 (B, out_stride), n_sym, flags)`; flag bit 2 = a decoded byte outside 'a'..'z' (NaN there).  With `original` (CUDA
        float64, B records of at least n_sym samples, e.g. the tensor that was encoded) also `max_abs_diff` float64 `(B,)` (NaN where a difference is
        NaN, as np.max) and `n_mismatch` int32 `(B,)`, the positions whose quantised original is not the decoded symbol."""
        ids, counts = self._check_ids(ids, counts, "detokenize_signal")
        stride = self._out_stride(ids, counts, out_stride)
        B = ids.shape[0]
        if out is None:
            out = torch.zeros((B, stride), dtype=torch.float64, device=ids.device)
        n_sym = torch.zeros((B,), dtype=torch.int32, device=ids.device)
        flags = torch.zeros((B,), dtype=torch.int32, device=ids.device)
        diff = mism = None
        o_stride = 0
        if original is not None:
            if not (isinstance(original, torch.Tensor) and original.is_cuda and original.dtype == torch.float64 and original.shape[0] == B):
                raise TypeError("original must be a CUDA float64 tensor with one record per row of ids")
            _lib.require_current(original.device)
            original = original.contiguous()
            o_stride = original.numel() // B if B else 0
            diff = torch.zeros((B,), dtype=torch.float64, device=ids.device)
            mism = torch.zeros((B,), dtype=torch.int32, device=ids.device)
        if B:
            _lib.check(_lib.lib().ecgb_detokenize_signal_f64_hip(
                self._h, _ptr(ids), ids.shape[1], _ptr(counts), B, float(percentiles["percentile_1"]), float(percentiles["percentile_99"]),
                _ptr(out), stride, _ptr(n_sym), _ptr(flags), _ptr(original), o_stride, _ptr(diff), _ptr(mism), _stream_ptr()))
        return (out, n_sym, flags) if original is None else (out, n_sym, flags, diff, mism)

    def token_histogram(self, ids, counts, n_bins: int | None = None):
        """Occurrences of every id over the valid tokens of the batch: `(hist int64 (n_bins,), overflow int64 scalar tensor)`; `n_bins` defaults to the
        table's id range (largest id + 1), ids at or above it are counted in `overflow`."""
        ids, counts = self._check_ids(ids, counts, "token_histogram")
        if n_bins is None:
            n_bins = int(_lib.lib().ecgb_tokenizer_copy_expansions(self._h, None, None, 0, None, 0)) or 256 + self.n_merges
        hist = torch.empty((int(n_bins),), dtype=torch.int64, device=ids.device)
        over = torch.empty((), dtype=torch.int64, device=ids.device)
        _lib.check(_lib.lib().ecgb_token_histogram_hip(_ptr(ids), max(1, ids.shape[1]), _ptr(counts), ids.shape[0], _ptr(hist), int(n_bins), _ptr(over),
                                                       _stream_ptr()))
        return hist, over


def detokenize_tile():
    """(tokens per chunk, output positions per tile) of the detokenise kernel."""
    a, b = C.c_uint32(), C.c_uint32()
    _lib.lib().ecgb_detokenize_tile(C.byref(a), C.byref(b))
    return a.value, b.value


def quantize(signal: torch.Tensor, percentiles, want_clipped: bool = False):
    """normalize_all on the GPU: CUDA float64 tensor -> uint8 alphabet indices (same shape)
    [and the clipped float64 tensor, the reference's first return value]."""
    if not (isinstance(signal, torch.Tensor) and signal.is_cuda and signal.dtype == torch.float64):
        raise TypeError("quantize needs a CUDA float64 tensor (no CPU fallback)")
    _lib.require_current(signal.device)
    x = signal.contiguous()
    sym = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    clipped = torch.empty_like(x) if want_clipped else None
    _lib.check(_lib.lib().ecgb_quantize_hip(_ptr(x), x.numel(), float(percentiles["percentile_1"]),
                                            float(percentiles["percentile_99"]), _ptr(sym), _ptr(clipped),
                                            _stream_ptr()))
    return (clipped, sym) if want_clipped else sym
