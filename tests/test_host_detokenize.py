"""CPU tests of the detokenise feature's host side: the expansion table the tokenizer handle builds (byte ids, merge ids, duplicates, unknown
ids, expansions longer than a byte can count), the device entry points' behaviour without a GPU, and the new CLI option.  No kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import load_tokenizer, random_merges

NODEVICE = -5


@pytest.fixture(scope="module")
def lib():
    from ecg_byte_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def _make_tok(lib, merges):
    from ecg_byte_amd.tokenizer import flatten_merges
    flat, off, ids = flatten_merges(merges)
    h = C.c_void_p()
    u32p = C.POINTER(C.c_uint32)
    rc = lib.ecgb_tokenizer_create(flat.ctypes.data_as(u32p), off.ctypes.data_as(u32p), ids.ctypes.data_as(u32p), len(merges), C.byref(h))
    assert rc == 0, rc
    return h


def _expansions(lib, h):
    """{id: bytes} for every id with a non-zero length, and the id range, through the C inspector (sizes first, then the copy)."""
    n_ids = lib.ecgb_tokenizer_copy_expansions(h, None, None, 0, None, 0)
    n_bytes = lib.ecgb_tokenizer_expansion_bytes(h)
    off, lens = np.full(n_ids, 0xDEAD, dtype=np.uint32), np.full(n_ids, 0xDEAD, dtype=np.uint32)
    raw = np.zeros(n_bytes, dtype=np.uint8)
    u32p = C.POINTER(C.c_uint32)
    assert lib.ecgb_tokenizer_copy_expansions(h, off.ctypes.data_as(u32p), lens.ctypes.data_as(u32p), n_ids, raw.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              n_bytes) == n_ids
    assert n_ids == 0 or int((off.astype(np.int64) + lens)[lens > 0].max()) <= n_bytes
    return {k: raw[off[k]: off[k] + lens[k]].tobytes() for k in range(n_ids) if lens[k]}, n_ids


@pytest.mark.parametrize("tag,n_merges,longest", [("c1", 1000, 51), ("c2", 4000, 194)])
def test_fixture_tokenizers_expand_to_their_vocab(lib, tag, n_merges, longest):
    vocab, merges, _ = load_tokenizer(tag)
    assert len(merges) == n_merges
    h = _make_tok(lib, merges)
    try:
        exp, n_ids = _expansions(lib, h)
    finally:
        lib.ecgb_tokenizer_destroy(h)
    assert n_ids == 256 + n_merges and sorted(exp) == list(range(n_ids))
    for b in range(256):
        assert exp[b] == bytes([b])
    for k in range(256, n_ids):
        assert exp[k] == vocab[k].encode(), k
    assert max(len(v) for v in exp.values()) == longest


def test_python_surface_gives_the_same_table():
    from ecg_byte_amd.tokenizer import HipTokenizer
    _, merges, _ = load_tokenizer("c1")
    off, lens, raw = HipTokenizer(merges).expansions()
    want = dict((tid, bytes(seq)) for seq, tid in merges)
    assert off.size == lens.size == 256 + len(merges)
    for tid, seq in want.items():
        assert raw[off[tid]: off[tid] + lens[tid]].tobytes() == seq


def test_later_duplicate_wins_like_a_dict(lib):
    rng = np.random.default_rng(11)
    merges = random_merges(rng, 400, dup_frac=0.3)
    # random_merges repeats EXPANSIONS under new ids; re-use ids too, so that one id names different expansions
    merges += [([97 + int(v) for v in rng.integers(0, 6, size=int(rng.integers(2, 9)))], int(rng.integers(256, 656))) for _ in range(120)]
    want = {b: bytes([b]) for b in range(256)}
    want.update({tid: bytes(seq) for seq, tid in merges})          # a dict built in list order
    h = _make_tok(lib, merges)
    try:
        exp, _ = _expansions(lib, h)
    finally:
        lib.ecgb_tokenizer_destroy(h)
    assert exp == want

    hand = [([97, 98], 300), ([99, 100, 101], 301), ([102, 102, 102, 102], 300)]
    h = _make_tok(lib, hand)
    try:
        exp, n_ids = _expansions(lib, h)
    finally:
        lib.ecgb_tokenizer_destroy(h)
    assert n_ids == 302 and exp[300] == b"ffff" and exp[301] == b"cde"


def test_unknown_ids_have_length_zero(lib):
    h = _make_tok(lib, [([97, 98], 260), ([98, 99], 300)])
    try:
        exp, n_ids = _expansions(lib, h)
        n = lib.ecgb_tokenizer_copy_expansions(h, None, None, 0, None, 0)
        lens = np.empty(n, dtype=np.uint32)
        lib.ecgb_tokenizer_copy_expansions(h, None, lens.ctypes.data_as(C.POINTER(C.c_uint32)), n, None, 0)
    finally:
        lib.ecgb_tokenizer_destroy(h)
    assert n_ids == 301
    assert sorted(exp) == list(range(256)) + [260, 300]
    holes = [k for k in range(256, 301) if k not in (260, 300)]
    assert (lens[holes] == 0).all() and (lens[:256] == 1).all() and lens[260] == 2 and lens[300] == 2


def test_long_expansions_keep_their_length(lib):
    rng = np.random.default_rng(5)
    a = [97 + int(v) for v in rng.integers(0, 26, size=300)]
    b = [97 + int(v) for v in rng.integers(0, 26, size=70_000)]
    h = _make_tok(lib, [(a, 256), (b, 257)])
    try:
        exp, n_ids = _expansions(lib, h)
    finally:
        lib.ecgb_tokenizer_destroy(h)
    assert n_ids == 258 and exp[256] == bytes(a) and exp[257] == bytes(b)


def test_copy_respects_capacities(lib):
    h = _make_tok(lib, [([97, 98, 99], 256)])
    try:
        off, lens = np.full(300, 77, dtype=np.uint32), np.full(300, 77, dtype=np.uint32)
        raw = np.full(300, 77, dtype=np.uint8)
        u32p = C.POINTER(C.c_uint32)
        n = lib.ecgb_tokenizer_copy_expansions(h, off.ctypes.data_as(u32p), lens.ctypes.data_as(u32p), 10, raw.ctypes.data_as(C.POINTER(C.c_uint8)), 5)
    finally:
        lib.ecgb_tokenizer_destroy(h)
    assert n == 257 and (off[10:] == 77).all() and (lens[10:] == 77).all() and (raw[5:] == 77).all()
    assert (lens[:10] == 1).all() and list(raw[:5]) == [0, 1, 2, 3, 4]


def test_tile_constants_are_reported(lib):
    chunk, tile = C.c_uint32(), C.c_uint32()
    lib.ecgb_detokenize_tile(C.byref(chunk), C.byref(tile))
    assert chunk.value >= 64 and tile.value >= 64 and tile.value % 16 == 0
    lib.ecgb_detokenize_tile(None, None)


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_device_entry_points_report_no_device(lib):
    """Without a GPU every entry point answers with a status; with one present the handle has a device copy and this test has nothing to say
    (tests/test_gpu_detokenize.py runs them)."""
    h = _make_tok(lib, [([97, 98], 256)])
    buf = np.zeros(64, dtype=np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    try:
        # bad arguments are refused on any machine, before anything is touched
        assert lib.ecgb_detokenize_hip(h, None, 4, p, 1, p, 8, p, p, None) == -1
        assert lib.ecgb_detokenize_hip(h, p, 4, p, 1, p, 0, p, p, None) == -1
        assert lib.ecgb_detokenize_values_f32_hip(h, p, 4, p, 1, p, None, 8, p, p, None) == -1
        assert lib.ecgb_detokenize_signal_f64_hip(None, p, 4, p, 1, 0.0, 1.0, p, 8, p, p, None, 0, None, None, None) == -1
        assert lib.ecgb_token_histogram_hip(p, 4, p, 1, None, 8, p, None) == -1
        assert lib.ecgb_token_histogram_hip(p, 4, p, 1, p, 0, p, None) == -1
        assert lib.ecgb_last_error()
        if _no_gpu():
            assert lib.ecgb_detokenize_hip(h, p, 4, p, 1, p, 8, p, p, None) == NODEVICE
            assert lib.ecgb_detokenize_values_f32_hip(h, p, 4, p, 1, p, p, 8, p, p, None) == NODEVICE
            assert lib.ecgb_detokenize_signal_f64_hip(h, p, 4, p, 1, 0.0, 1.0, p, 8, p, p, p, 8, p, p, None) == NODEVICE
            assert lib.ecgb_token_histogram_hip(p, 4, p, 1, p, 8, p, None) == NODEVICE
            assert b"GPU" in lib.ecgb_last_error()
            assert not buf.any()
    finally:
        lib.ecgb_tokenizer_destroy(h)


def test_wide_ids_have_no_table_and_say_so(lib):
    h = _make_tok(lib, [([97, 98], 1 << 22)])
    buf = np.zeros(8, dtype=np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    try:
        assert lib.ecgb_tokenizer_copy_expansions(h, None, None, 0, None, 0) == 0
        assert lib.ecgb_tokenizer_expansion_bytes(h) == 0
        assert lib.ecgb_detokenize_hip(h, p, 4, p, 1, p, 8, p, p, None) == -3
    finally:
        lib.ecgb_tokenizer_destroy(h)


def test_cli_parses_check_files():
    from ecg_byte_amd.train_tokenizer import get_args
    assert get_args(["--check_files", "x"]).check_files == "x"
    assert get_args([]).check_files is None


def test_python_methods_refuse_cpu_tensors():
    import torch
    from ecg_byte_amd.tokenizer import HipTokenizer
    tk = HipTokenizer([([97, 98], 256)])
    ids, counts = torch.zeros((1, 4), dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    for call in (lambda: tk.detokenize(ids, counts, 8), lambda: tk.expand(ids, counts, ids.float(), 8),
                 lambda: tk.detokenize_signal(ids, counts, {"percentile_1": 0.0, "percentile_99": 1.0}, 8), lambda: tk.token_histogram(ids, counts)):
        with pytest.raises(TypeError):
            call()
