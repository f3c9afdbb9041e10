"""GPU tests of detokenise (csrc/detokenize.hip): token ids back to symbol bytes, per-symbol values and dequantised signal, the token histogram, and
the Python surface above them.  Every output row is filled with a sentinel first: what lies past n_sym in a row, and past the last row, must stay.
Edge cases are placed from ecgb_detokenize_tile, not from a copy of the kernel's constants."""
import os
from collections import Counter

import numpy as np
import pytest
import torch

from helpers import GOLDEN, load_tokenizer, random_merges
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TAIL = 0x7FFFFFFF           # what the id rows hold past counts[b]: never to be read as an id
S_U8, S_F32, S_F64 = 0xAA, 0xAAAAAAAA, 0xAAAAAAAAAAAAAAAA


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ecg_byte_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "HIP extension not built -- no fallback exists"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def blocking(dev):
    from ecg_byte_amd.tokenizer import detokenize_tile
    return detokenize_tile()


def _sentinel(rows, stride, dtype, guard=64):
    """(flat buffer with `guard` extra elements, its (rows, stride) view), every byte 0xAA."""
    size = torch.empty((), dtype=dtype).element_size()
    flat = torch.full(((rows * stride + guard) * size,), 0xAA, dtype=torch.uint8, device="cuda").view(dtype)
    return flat, flat[: rows * stride].view(rows, stride)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _pack(records, pad=7):
    """id lists -> (ids int32 (B, stride) with TAIL past each count, counts int32 (B,)) on the device; stride exceeds every count."""
    stride = max(len(r) for r in records) + pad
    ids = np.full((len(records), stride), TAIL, dtype=np.int64)
    for b, r in enumerate(records):
        ids[b, : len(r)] = r
    counts = np.array([len(r) for r in records], dtype=np.int32)
    return torch.from_numpy(ids.astype(np.uint32).view(np.int32)).cuda(), torch.from_numpy(counts).cuda()


def _expand_py(record, table):
    return b"".join(table.get(int(t), b"") for t in record)


def _table(merges):
    t = {b: bytes([b]) for b in range(256)}
    t.update({tid: bytes(seq) for seq, tid in merges})
    return t


def _check_rows(got_flat, got, n_sym, want_rows, sentinel):
    """Rows equal the expectation up to n_sym, hold the sentinel after it, and the guard past the last row is untouched."""
    g, gf, n_sym = _bits(got.cpu().numpy()), _bits(got_flat.cpu().numpy()), n_sym.cpu().numpy()
    for b, want in enumerate(want_rows):
        w = _bits(want)
        assert n_sym[b] == w.size, (b, n_sym[b], w.size)
        assert np.array_equal(g[b, : w.size], w), f"record {b}: first difference at {int(np.flatnonzero(g[b, : w.size] != w)[0])}"
        assert (g[b, w.size:] == sentinel).all(), f"record {b}: written past n_sym"
    assert (gf[g.size:] == sentinel).all(), "written past the last row"


# ---- round trip on the fixture tokenizers ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[("c1", 4, 1000), ("c2", 2, 5000)], ids=["c1-4x12x1000", "c2-2x12x5000"])
def trip(request, dev):
    from ecg_byte_amd import synth
    from ecg_byte_amd.tokenizer import HipTokenizer
    tag, B, L = request.param
    vocab, merges, pc = load_tokenizer(tag)
    tk = HipTokenizer(merges)
    x = synth.synth_ecg(B, L, seed=7)
    xd = torch.from_numpy(x).cuda()
    ids, counts = tk.quantize_encode(xd, pc)
    sym = np.stack([O.quantize(x[b], pc["percentile_1"], pc["percentile_99"]).reshape(-1) for b in range(B)])
    return dict(tk=tk, vocab=vocab, merges=merges, pc=pc, x=x, xd=xd, ids=ids, counts=counts, sym=sym, n=12 * L, B=B)


def _run_all(t, stride):
    tk, ids, counts = t["tk"], t["ids"], t["counts"]
    fb, ob = _sentinel(t["B"], stride, torch.uint8)
    fs, os_ = _sentinel(t["B"], stride, torch.float64)
    rb = tk.detokenize(ids, counts, stride, out=ob)
    rs = tk.detokenize_signal(ids, counts, t["pc"], stride, original=t["xd"], out=os_)
    hist = tk.token_histogram(ids, counts)
    torch.cuda.synchronize()
    return fb, rb, fs, rs, hist


def test_round_trip_bytes_signal_and_error(trip):
    t = trip
    stride = t["n"] + 5
    fb, (ob, nb, flb), fs, (os_, ns, fls, diff, mism), _ = _run_all(t, stride)
    p1, p99 = t["pc"]["percentile_1"], t["pc"]["percentile_99"]
    want_bytes = [(t["sym"][b] + ord("a")).astype(np.uint8) for b in range(t["B"])]
    _check_rows(fb, ob, nb, want_bytes, S_U8)
    ids, counts = t["ids"].cpu().numpy(), t["counts"].cpu().numpy()
    for b in range(t["B"]):
        text = O.decode_text([int(v) for v in ids[b, : counts[b]]], t["vocab"])
        assert ob[b, : t["n"]].cpu().numpy().tobytes() == text.encode()
    assert (flb.cpu().numpy() == 0).all() and (fls.cpu().numpy() == 0).all()
    rebuilt = [O.dequantize(t["sym"][b], p1, p99) for b in range(t["B"])]
    _check_rows(fs, os_, ns, rebuilt, S_F64)
    want_diff = np.array([np.max(np.abs(t["x"][b].reshape(-1) - rebuilt[b])) for b in range(t["B"])])
    assert np.array_equal(_bits(diff.cpu().numpy()), _bits(want_diff))
    assert (mism.cpu().numpy() == 0).all()


def test_every_output_is_the_same_on_a_second_call(trip):
    a, b = _run_all(trip, trip["n"] + 5), _run_all(trip, trip["n"] + 5)

    def flat(r):
        fb, rb, fs, rs, hist = r
        return [fb, *rb, fs, *rs, *hist]
    for u, v in zip(flat(a), flat(b)):
        assert np.array_equal(_bits(u.cpu().numpy()), _bits(v.cpu().numpy()))


def test_default_out_stride_is_the_longest_record(trip):
    out, n_sym, flags = trip["tk"].detokenize(trip["ids"], trip["counts"])
    assert out.shape == (trip["B"], trip["n"]) and (n_sym.cpu().numpy() == trip["n"]).all() and (flags.cpu().numpy() == 0).all()


def test_nan_sample_gives_nan_error_for_its_record_only(trip):
    t = trip
    x = t["x"].copy()
    x[1, 3, 17] = np.nan
    xd = torch.from_numpy(x).cuda()
    ids, counts = t["tk"].quantize_encode(xd, t["pc"])
    _, _, _, diff, mism = t["tk"].detokenize_signal(ids, counts, t["pc"], t["n"], original=xd)
    _, _, _, clean, _ = t["tk"].detokenize_signal(t["ids"], t["counts"], t["pc"], t["n"], original=t["xd"])
    diff, clean = diff.cpu().numpy(), clean.cpu().numpy()
    assert np.isnan(diff[1]) and not np.isnan(np.delete(diff, 1)).any()
    assert np.array_equal(_bits(np.delete(diff, 1)), _bits(np.delete(clean, 1)))
    assert (mism.cpu().numpy() == 0).all()


def test_histogram_counts_the_valid_tokens(trip):
    t = trip
    ids, counts = t["ids"].cpu().numpy(), t["counts"].cpu().numpy()
    valid = np.concatenate([ids[b, : counts[b]] for b in range(t["B"])]).astype(np.int64)
    n_ids = 256 + len(t["merges"])
    hist, over = t["tk"].token_histogram(t["ids"], t["counts"])
    hist2, over2 = t["tk"].token_histogram(t["ids"], t["counts"])
    assert np.array_equal(hist.cpu().numpy(), np.bincount(valid, minlength=n_ids)) and int(over) == 0
    assert int(hist.sum()) == int(counts.sum())
    assert torch.equal(hist, hist2) and torch.equal(over, over2)
    small, over = t["tk"].token_histogram(t["ids"], t["counts"], n_bins=300)
    assert np.array_equal(small.cpu().numpy(), np.bincount(valid, minlength=n_ids)[:300])
    assert int(over) == int((valid >= 300).sum()) and int(small.sum()) + int(over) == int(counts.sum())


# ---- edges of the blocking, with a hand-made tokenizer ------------------------------------------------------------------------------------------
LENS = (2, 3, 64, 65, 255, 256, 300)


def _edge_merges(rng):
    return [([97 + int(v) for v in rng.integers(0, 6, size=n)], 256 + i) for i, n in enumerate(LENS)]


def _record_of_total(rng, total, lens_by_id):
    """Random tokens whose expansions add up to exactly `total` (1-byte tokens fill the end)."""
    rec, left = [], total
    ids = sorted(lens_by_id)
    while left > 400:
        t = ids[int(rng.integers(len(ids)))]
        rec.append(t)
        left -= lens_by_id[t]
    rec += [97 + int(v) for v in rng.integers(0, 6, size=left)]
    return rec


@pytest.fixture(scope="module")
def edges(dev, blocking):
    from ecg_byte_amd.tokenizer import HipTokenizer
    chunk, tile = blocking
    rng = np.random.default_rng(3)
    merges = _edge_merges(rng)
    table = _table(merges)
    lens = {tid: len(seq) for seq, tid in merges}
    lens.update({97 + k: 1 for k in range(6)})
    every = sorted(lens)
    id300 = 256 + LENS.index(300)

    def n_tokens(n):
        return [every[int(k)] for k in rng.integers(0, len(every), size=n)]
    records = [n_tokens(chunk - 1), n_tokens(chunk), n_tokens(chunk + 1), n_tokens(2 * chunk + 1),
               _record_of_total(rng, tile - 1, lens), _record_of_total(rng, tile, lens), _record_of_total(rng, tile + 1, lens),
               _record_of_total(rng, tile - 10, lens) + [id300] + n_tokens(30),          # a 300-byte token that starts 10 bytes before a tile edge
               [97 + int(v) for v in rng.integers(0, 6, size=3000)],                     # 1-byte tokens only
               [id300] * 40,                                                             # 300-byte tokens only
               [256 + LENS.index(65)],                                                   # one token
               []]                                                                       # counts == 0
    want = [np.frombuffer(_expand_py(r, table), dtype=np.uint8) for r in records]
    assert [w.size for w in want[4:7]] == [tile - 1, tile, tile + 1]
    ids, counts = _pack(records)
    return dict(tk=HipTokenizer(merges), records=records, want=want, ids=ids, counts=counts, stride=max(w.size for w in want) + 3, rng=rng)


def test_edges_bytes(edges):
    e = edges
    flat, out = _sentinel(len(e["records"]), e["stride"], torch.uint8)
    _, n_sym, flags = e["tk"].detokenize(e["ids"], e["counts"], e["stride"], out=out)
    _check_rows(flat, out, n_sym, e["want"], S_U8)
    assert (flags.cpu().numpy() == 0).all() and int(n_sym[-1]) == 0


def test_edges_expand_values_as_bits(edges):
    e = edges
    rng = np.random.default_rng(8)
    bits = rng.integers(0, 2 ** 32, size=tuple(e["ids"].shape), dtype=np.uint64).astype(np.uint32)       # random patterns: NaNs and infinities among them
    bits[:, 0], bits[:, 1], bits[:, 2] = 0x80000000, 0x7FC12345, 0xFFC00001                              # -0.0 and two NaN payloads
    values = torch.from_numpy(bits.view(np.float32)).cuda()
    flat, out = _sentinel(len(e["records"]), e["stride"], torch.float32)
    _, n_sym, flags = e["tk"].expand(e["ids"], e["counts"], values, e["stride"], out=out)
    table = _table(_edge_merges(np.random.default_rng(3)))
    want = [np.repeat(bits[b, : len(r)], [len(table[t]) for t in r]) if r else np.zeros(0, np.uint32) for b, r in enumerate(e["records"])]
    _check_rows(flat, out, n_sym, want, S_F32)
    assert (flags.cpu().numpy() == 0).all()


def test_edges_signal(edges):
    e = edges
    pc = {"percentile_1": -1.25, "percentile_99": 2.5}
    flat, out = _sentinel(len(e["records"]), e["stride"], torch.float64)
    _, n_sym, flags = e["tk"].detokenize_signal(e["ids"], e["counts"], pc, e["stride"], out=out)
    want = [O.dequantize(w - ord("a"), pc["percentile_1"], pc["percentile_99"]) if w.size else np.zeros(0) for w in e["want"]]
    _check_rows(flat, out, n_sym, want, S_F64)
    assert (flags.cpu().numpy() == 0).all()


@pytest.mark.parametrize("stride", [1001, 1003])
def test_rows_that_start_unaligned(edges, stride):
    e = edges
    rng = np.random.default_rng(stride)
    merges = _edge_merges(np.random.default_rng(3))
    table, lens = _table(merges), {tid: len(seq) for seq, tid in merges}
    records = [_record_of_total(rng, n, lens) for n in (stride, stride - 7, 500)]
    want = [np.frombuffer(_expand_py(r, table), dtype=np.uint8) for r in records]
    ids, counts = _pack(records)
    pc = {"percentile_1": 0.0, "percentile_99": 1.0}
    bits = rng.integers(0, 2 ** 32, size=tuple(ids.shape), dtype=np.uint64).astype(np.uint32)
    flat, out = _sentinel(3, stride, torch.uint8)
    _, n_sym, flags = e["tk"].detokenize(ids, counts, stride, out=out)
    _check_rows(flat, out, n_sym, want, S_U8)
    flat, out = _sentinel(3, stride, torch.float32)
    _, n_sym, _ = e["tk"].expand(ids, counts, torch.from_numpy(bits.view(np.float32)).cuda(), stride, out=out)
    _check_rows(flat, out, n_sym, [np.repeat(bits[b, : len(r)], [len(table[t]) for t in r]) for b, r in enumerate(records)], S_F32)
    flat, out = _sentinel(3, stride, torch.float64)
    _, n_sym, _ = e["tk"].detokenize_signal(ids, counts, pc, stride, out=out)
    _check_rows(flat, out, n_sym, [O.dequantize(w - ord("a"), 0.0, 1.0) for w in want], S_F64)
    assert (flags.cpu().numpy() == 0).all()


# ---- flags ----------------------------------------------------------------------------------------------------------------------------------------
def test_unknown_ids_flag_their_record_only(dev):
    from ecg_byte_amd.tokenizer import HipTokenizer
    from ecg_byte_amd.tokenizer_utils import decode_batch
    merges = [([97, 98], 256), ([98, 99, 100], 257), ([101, 101], 259)]                  # 258 is a hole
    table = _table(merges)
    tk = HipTokenizer(merges)
    rng = np.random.default_rng(2)
    base = [[int(v) for v in rng.choice([97, 98, 99, 256, 257, 259], size=n)] for n in (50, 60, 70, 80)]
    records = [base[0], base[1][:20] + [256 + len(merges) + 4741] + base[1][20:], base[2][:5] + [258] + base[2][5:], base[3]]
    ids, counts = _pack(records)
    stride = 400
    flat, out = _sentinel(4, stride, torch.uint8)
    _, n_sym, flags = tk.detokenize(ids, counts, stride, out=out)
    _check_rows(flat, out, n_sym, [np.frombuffer(_expand_py(r, table), dtype=np.uint8) for r in records], S_U8)    # an unknown id contributes nothing
    assert flags.cpu().numpy().tolist() == [0, 1, 1, 0]
    with pytest.raises(KeyError) as err:
        decode_batch(ids, counts, tk)
    assert err.value.args[0] == 256 + len(merges) + 4741
    assert decode_batch(ids[[0, 3]], counts[[0, 3]], merges) == [_expand_py(records[0], table), _expand_py(records[3], table)]


def test_rows_are_cut_at_out_stride(edges):
    e = edges
    table = _table(_edge_merges(np.random.default_rng(3)))
    id300 = 256 + LENS.index(300)
    a = [97] * 50 + [id300] + [98] * 20
    full = [np.frombuffer(_expand_py(r, table), dtype=np.uint8) for r in (a, [99] * 30)]
    ids, counts = _pack([a, [99] * 30])
    for stride, cut in ((full[0].size - 1, True), (200, True), (full[0].size, False)):   # one byte short; in the middle of the 300-byte token; exact fit
        flat, out = _sentinel(2, stride, torch.uint8)
        _, n_sym, flags = e["tk"].detokenize(ids, counts, stride, out=out)
        _check_rows(flat, out, n_sym, [full[0][:stride], full[1]], S_U8)
        assert flags.cpu().numpy().tolist() == [2 if cut else 0, 0] and int(n_sym[0]) == stride
        flat, out = _sentinel(2, stride, torch.float64)
        _, n_sym, flags = e["tk"].detokenize_signal(ids, counts, {"percentile_1": 0.0, "percentile_99": 1.0}, stride, out=out)
        _check_rows(flat, out, n_sym, [O.dequantize(full[0][:stride] - ord("a"), 0.0, 1.0), O.dequantize(full[1] - ord("a"), 0.0, 1.0)], S_F64)
        assert flags.cpu().numpy().tolist() == [2 if cut else 0, 0]


def test_bytes_outside_the_alphabet_become_nan(dev):
    from ecg_byte_amd.tokenizer import HipTokenizer
    merges = [([97, 35, 98], 256), ([99, 100], 257)]                                   # '#' is no symbol
    table = _table(merges)
    tk = HipTokenizer(merges)
    records = [[97, 257, 256, 122, 257], [257, 98, 98, 257], [35, 97, 123, 96]]
    ids, counts = _pack(records)
    flat, out = _sentinel(3, 16, torch.float64)
    _, n_sym, flags = tk.detokenize_signal(ids, counts, {"percentile_1": -0.5, "percentile_99": 0.5}, 16, out=out)
    assert flags.cpu().numpy().tolist() == [4, 0, 4]
    got = out.cpu().numpy()
    for b, r in enumerate(records):
        text = np.frombuffer(_expand_py(r, table), dtype=np.uint8)
        ok = (text >= ord("a")) & (text <= ord("z"))
        assert int(n_sym[b]) == text.size
        assert np.array_equal(np.isnan(got[b, : text.size]), ~ok)
        want = O.dequantize(np.where(ok, text - ord("a"), 0).astype(np.uint8), -0.5, 0.5)
        assert np.array_equal(_bits(got[b, : text.size][ok]), _bits(want[ok]))
        assert (_bits(got[b, text.size:]) == S_F64).all()


# ---- the general trie form ------------------------------------------------------------------------------------------------------------------------
def test_general_form_detokenises_its_own_encode(dev):
    from ecg_byte_amd import _lib
    from ecg_byte_amd.tokenizer import HipTokenizer
    rng = np.random.default_rng(9)
    alphabet = bytes(range(60, 100))                                                    # 40 byte values: more classes than the packed trie has
    merges = random_merges(rng, 300, alphabet=alphabet, max_len=9)
    tk = HipTokenizer(merges)
    assert _lib.lib().ecgb_tokenizer_copy_nodes(tk._h, None, 0) == 0 and tk.n_classes == 0, "expected the general form"
    spliced = b"".join(bytes(merges[int(k)][0]) for k in rng.integers(0, 300, size=600))[:2000].ljust(2000, b"A")
    texts = [spliced] + [bytes(rng.choice(list(alphabet), size=2000).astype(np.uint8)) for _ in range(2)]
    text = torch.from_numpy(np.stack([np.frombuffer(t, dtype=np.uint8) for t in texts])).cuda()
    ids, counts = tk.encode_bytes(text)
    assert int(counts.min()) < 2000                                                     # merges did hit
    flat, out = _sentinel(3, 2003, torch.uint8)
    _, n_sym, flags = tk.detokenize(ids, counts, 2003, out=out)
    _check_rows(flat, out, n_sym, [np.frombuffer(t, dtype=np.uint8) for t in texts], S_U8)
    assert (flags.cpu().numpy() == 0).all()


# ---- the Python layers above ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five_records(dev, tmp_path_factory):
    from ecg_byte_amd import synth
    d = tmp_path_factory.mktemp("records")
    x = synth.synth_ecg(5, 500, seed=21)
    paths = []
    for b in range(5):
        paths.append(str(d / f"ecg_{b}.npy"))
        np.save(paths[-1], x[b])
    return d, x, paths


def test_analyze_token_distribution(five_records):
    from ecg_byte_amd.tokenizer_utils import analyze_token_distribution
    _, x, paths = five_records
    _, merges, pc = load_tokenizer("c1")
    want, lengths = Counter(), []
    for b in range(5):
        enc = O.encode_text(O.symbols_to_text(O.quantize(x[b], pc["percentile_1"], pc["percentile_99"])), merges)
        want.update(int(v) for v in enc)
        lengths.append(len(enc))
    got, got_lengths = analyze_token_distribution(paths, merges, pc, num_workers=3)
    assert isinstance(got, Counter) and got == want and got_lengths == lengths


def test_reconstruct_batch(five_records):
    from ecg_byte_amd.tokenizer_utils import reconstruct_batch
    _, x, _ = five_records
    _, merges, pc = load_tokenizer("c1")
    res = reconstruct_batch(x, pc, merges)
    for b, (ok, diff, n_tok) in enumerate(res):
        sym = O.quantize(x[b], pc["percentile_1"], pc["percentile_99"])
        assert ok and n_tok == len(O.encode_text(O.symbols_to_text(sym), merges))
        assert diff == float(np.max(np.abs(x[b] - O.dequantize(sym, pc["percentile_1"], pc["percentile_99"]))))


def test_cli_check_files(five_records, capsys):
    from ecg_byte_amd import train_tokenizer as T
    d, x, paths = five_records
    _, _, pc = load_tokenizer("c1")
    (d / "list.txt").write_text("\n".join(paths) + "\n")

    def run(pcs, name):
        np.save(str(d / name), pcs, allow_pickle=True)
        ok = T.main(T.get_args(["--loaded", os.path.join(GOLDEN, "tokenizer_c1.pkl"), "--percentiles", str(d / name), "--check_ecg", paths[0],
                                "--check_files", str(d / "list.txt")]))
        return ok, capsys.readouterr().out
    ok, text = run(pc, "pc.npy")
    assert ok and "records checked: 5" in text and "round trips failed: 0" in text and f"total: {5 * 12 * 500} symbols -> " in text
    worst = [ln for ln in text.splitlines() if ln.startswith("largest |signal - dequantised| = ") and " in " in ln]
    assert len(worst) == 1 and worst[0].rsplit(" in ", 1)[1] in paths
    # the round trip is a property of the tokenizer, not of the scale: other percentiles still round-trip, with another error
    ok2, text2 = run({"percentile_1": pc["percentile_1"] - 0.3, "percentile_99": pc["percentile_99"] + 0.7}, "pc_wrong.npy")
    worst2 = [ln for ln in text2.splitlines() if ln.startswith("largest |signal - dequantised| = ") and " in " in ln]
    assert ok2 and "round trips failed: 0" in text2 and worst2 and worst2[0].split(" in ")[0] != worst[0].split(" in ")[0]
