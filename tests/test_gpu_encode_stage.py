"""The staging phase of the wave-per-record encode kernel (encode_flow_kernel).  Two parts.  The change map over the staged symbols (build_dmap,
change_bits8: eight symbols a step) is what this file was written for: byte streams under a one-token vocabulary, where a MISSED change bit gives a
wrong token, under a vocabulary of runs a^2 .. a^128, where a SPURIOUS bit inside a run ends a token early, and the C2 records.  The quantiser cases
(levels4 / stage_symbols: thresholds and their neighbours in every byte lane of lane 0's and lane 63's group, large offsets, record shapes) are
regression tests of the staging arithmetic as it stands -- one f64 FMA, float clamp and truncating convert, a group with a sample within 1e-4 of a
step redone from the exact staircase.  Every case compares with the oracle, bit for bit, under plan 2 (16 waves; C2 segments of 3 456 symbols) and
plan 3 (8 waves; 7 040), at batch 1 - 4."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import load_tokenizer
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C2_SEG = {2: 3456, 3: 7040}      # segment lengths the two plans pick for the C2 tokenizer (64 chunks of 54 / 110 symbols)
C2_MARGIN = 208                  # symbols staged past a segment's end (trie depth 194, rounded up to 16)
AB_SEG = {2: 3968, 3: 8064}      # ... and for a trie of two tokens (tests/test_gpu_encode_resolve.py)
BATCH_GROUPS = 5                 # kStageGroups: groups of four samples a lane loads per staging batch; a batch is 4 * 64 * 5 = 1 280 samples


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ecg_byte_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "HIP extension not built -- no fallback exists"
    return torch.device("cuda", 0)


@pytest.fixture(params=[2, 3], ids=["plan-wave", "plan-wave-long-segments"])
def plan(request, dev):
    from ecg_byte_amd.tokenizer import set_encode_plan
    set_encode_plan(request.param)
    yield request.param
    set_encode_plan(0)


@pytest.fixture(scope="module")
def c2(dev):
    from ecg_byte_amd import synth
    from ecg_byte_amd.tokenizer import HipTokenizer
    _, merges, pc = load_tokenizer("c2")
    x = synth.synth_ecg(4, 5000, seed=23)            # (4, 12, 5000)
    return HipTokenizer(merges), O.Trie(merges), pc, x


def _check(tk, trie, pc, x, what=""):
    """x: (B, n) float64 numpy or a CUDA tensor of that shape; every record against the oracle's quantise + encode."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    host = t.cpu().numpy()
    ids, counts = tk.quantize_encode(t, pc)
    ids, counts = ids.cpu().numpy(), counts.cpu().numpy()
    for b in range(host.shape[0]):
        ref = trie.quantize_encode(host[b], pc["percentile_1"], pc["percentile_99"])
        assert counts[b] == ref.size, (what, b, int(counts[b]), ref.size)
        if not np.array_equal(ids[b, : ref.size].astype(np.uint32), ref):
            sym_ref = O.quantize(host[b], pc["percentile_1"], pc["percentile_99"])
            first = int(np.flatnonzero(ids[b, : ref.size].astype(np.uint32) != ref)[0])
            raise AssertionError((what, b, "first differing token", first, "levels of the record", sym_ref[:16].tolist()))


def _thresholds(pc):
    from ecg_byte_amd import _lib
    thr = (C.c_double * 25)()
    _lib.check(_lib.lib().ecgb_quantizer_thresholds(float(pc["percentile_1"]), float(pc["percentile_99"]), thr))
    return np.array(list(thr), dtype=np.float64)


def _edge_values(pc):
    """The samples the fast path may get wrong if its band, its clamp or its rounding were off."""
    p1, p99 = float(pc["percentile_1"]), float(pc["percentile_99"])
    a = p1 - 0.5
    d = ((p99 + 0.5) - (p1 - 0.5)) + 1e-6
    scale = 26.0 / d
    vals = []
    for t in _thresholds(pc):                               # every step of the staircase: itself, +-1, +-2, +-4 ulp
        for ulps in (0, 1, 2, 4):
            up = down = t
            for _ in range(ulps):
                up, down = np.nextafter(up, np.inf), np.nextafter(down, -np.inf)
            vals += [up, down] if ulps else [t]
    for k2 in range(0, 53):                                 # q at 5e-5, 1e-4, 2e-4 either side of every integer and half-integer 0 .. 26
        for off in (5e-5, 1e-4, 2e-4):
            vals += [a + (0.5 * k2 + off) / scale, a + (0.5 * k2 - off) / scale]
    vals += [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e300, -1e300, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308]
    for eps in (1e-12, 1e-9, 1e-6, 1e-3, 0.4 / scale, 1.0 / scale, 7.0 / scale, 40.0 / scale):
        vals += [a - eps, a + d + eps, a + d - eps]         # just below level 0, just above (and below the top of) level 25
    return np.array(vals, dtype=np.float64), a + 12.5 / scale


def _edge_records(vals, background):
    """One edge value per group of four, the other three samples plain: records of 13 blocks of 256 samples (one segment under either plan, three
    staging batches, so every unrolled group of a batch is used); block m holds its value in byte lane j of lane 0's group and of lane 63's."""
    slots = [(v, j) for v in vals for j in range(4)]
    per = 13
    n_rec = -(-len(slots) // per)
    x = np.full((n_rec, per * 256), background, dtype=np.float64)
    for s, (v, j) in enumerate(slots):
        r, m = divmod(s, per)
        x[r, 256 * m + j] = v
        x[r, 256 * m + 252 + j] = v
    return x


def test_quantiser_edges_in_every_byte_lane_and_both_end_lanes(plan, c2):
    tk, trie, pc, _ = c2
    vals, bg = _edge_values(pc)
    x = _edge_records(vals, bg)
    for r in range(0, x.shape[0], 4):                       # batches of 4, the last one smaller
        _check(tk, trie, pc, x[r: r + 4], f"edge records {r}..")
    _check(tk, trie, pc, x[:1], "edge record 0 alone")


def test_every_group_of_a_wave_on_an_edge(plan, c2):
    """All four samples of every group ambiguous at once (a record of nothing but thresholds and their neighbours)."""
    tk, trie, pc, _ = c2
    vals, _ = _edge_values(pc)
    x = np.resize(vals, (3, 2 * 1280 + 36))
    _check(tk, trie, pc, x, "all edges")


@pytest.mark.parametrize("p1, span", [(1.0e9, 1.0), (-3.0e9, 1.0), (7.6e7, 1.0), (7.7e7, 1.0), (2.0e7, 1.0e-3)],
                         ids=["a*scale 1.3e10", "a*scale -3.9e10", "a*scale 9.9e8 (fast)", "a*scale 1.0e9 (exact)", "a*scale 5.2e8, scale 26"])
def test_large_offsets_take_the_exact_staircase(plan, dev, c2, p1, span):
    """|a * scale| >= 1e9: the float arithmetic of the fast path cannot resolve the 1e-4 band, every group takes the staircase; just below the
    bound the fast path runs with the least margin it is allowed."""
    tk, trie, _, _ = c2
    pc = {"percentile_1": p1, "percentile_99": p1 + span}
    rng = np.random.default_rng(5)
    x = (p1 - 0.5) + (span + 1.0) * rng.uniform(-0.2, 1.2, size=(2, 3 * 1280 + 7))      # q from -5 to 31
    thr = _thresholds(pc)
    edges = np.concatenate([thr, np.nextafter(thr, np.inf), np.nextafter(thr, -np.inf)])
    x[0, 5: 5 + edges.size] = edges
    x[1, 1281: 1281 + edges.size] = edges[::-1]
    _check(tk, trie, pc, x, f"p1 {p1}")


def _c2_lengths():
    out = [1, 3, 4, 5, 255, 256, 257, 1281]
    for seg in C2_SEG.values():
        out += [seg - 1, seg, seg + 1, seg + C2_MARGIN + 1]
    return out


@pytest.mark.parametrize("n", _c2_lengths())
def test_record_lengths_at_group_batch_and_segment_edges(plan, c2, n):
    tk, trie, pc, x = c2
    flat = x.reshape(4, -1)
    _check(tk, trie, pc, flat[:3, 100: 100 + n], f"n {n}")
    _check(tk, trie, pc, flat[3:, :n], f"n {n}, one record")


@pytest.mark.parametrize("n", [1283, 4097])
def test_odd_length_and_a_row_pointer_off_by_eight_bytes(plan, c2, n):
    """Rows that the 16-byte loads cannot take: an odd length (every other row unaligned) and a base pointer 8 bytes past a 16-byte boundary."""
    tk, trie, pc, x = c2
    flat = x.reshape(4, -1)
    _check(tk, trie, pc, flat[:4, :n], "odd length")
    buf = torch.from_numpy(np.ascontiguousarray(flat[:2, : n + 1]).reshape(-1)).cuda()
    shifted = buf[1: 1 + 2 * n].view(2, n)                  # same even-or-odd n, base + 8 bytes
    assert shifted.data_ptr() % 16 == 8 and shifted.is_contiguous()
    _check(tk, trie, pc, shifted, "pointer + 8")
    even = torch.from_numpy(np.ascontiguousarray(flat[:2, : n + 2]).reshape(-1)).cuda()
    shifted = even[1: 1 + 2 * (n + 1)].view(2, n + 1)
    assert shifted.data_ptr() % 16 == 8
    _check(tk, trie, pc, shifted, "even length, pointer + 8")


def test_one_full_record(plan, c2):
    tk, trie, pc, x = c2
    _check(tk, trie, pc, x[:1].reshape(1, -1), "12 x 5000")
    _check(tk, trie, pc, x.reshape(4, -1), "4 records of 12 x 5000")


# ---- the change map on byte streams: a vocabulary of the one token 'ab', so a missed bit shows as a wrong or missing token ...
AB = [([97, 98], 256)]
# ... and one of runs, a^2 .. a^128: inside a run the walk follows a node's continuation only while the map says "same symbol", so a spurious bit cuts a token short
RUNS = [([97] * k, 256 + k - 2) for k in range(2, 129)]


def _check_bytes(texts, merges=AB):
    from ecg_byte_amd.tokenizer import HipTokenizer
    tk = HipTokenizer(merges)
    n = len(texts[0])
    assert all(len(t) == n for t in texts)
    t = torch.from_numpy(np.frombuffer(b"".join(texts), dtype=np.uint8).reshape(len(texts), n).copy()).cuda()
    ids, counts = tk.encode_bytes(t)
    ids, counts = ids.cpu().numpy(), counts.cpu().numpy()
    for b, text in enumerate(texts):
        ref = np.asarray(O.encode_text(text, merges), dtype=np.uint32)
        assert counts[b] == ref.size, (n, b, int(counts[b]), ref.size)
        assert np.array_equal(ids[b, : ref.size].astype(np.uint32), ref), (n, b)


def test_a_single_change_at_word_and_segment_edges(plan):
    for k in [31, 32, 33, 63, 64, 65] + [s + e for s in AB_SEG.values() for e in (-1, 0, 1)]:
        _check_bytes([b"a" * k + b"b"])
        _check_bytes([b"a" * k + b"b" + b"a" * 40, b"b" * k + b"a" + b"b" * 40, b"a" * (k + 41)])


def test_strict_alternation_across_word_and_segment_edges(plan):
    for n in (70, AB_SEG[2] + 40, AB_SEG[3] + 40):
        p = (b"ab" * (n // 2 + 1))[:n]
        q = (b"ba" * (n // 2 + 1))[:n]
        _check_bytes([p])
        _check_bytes([p, q, p, q])


def test_constant_streams_of_every_length_to_130(plan):
    for n in range(1, 131):
        _check_bytes([b"a" * n] if n % 3 else [b"a" * n, b"b" * n])


def test_the_only_change_at_a_lane_or_batch_hand_over(plan):
    """The first position of a lane's group, the last position of a staging batch and the first of the next."""
    batch = 4 * 64 * BATCH_GROUPS
    n = 2 * batch + 100
    for p in (1, 4, 252, 256, batch - 1, batch, batch + 1, 2 * batch - 1, 2 * batch):
        _check_bytes([b"a" * p + b"b" * (n - p)])
    _check_bytes([b"a" * p + b"b" * (n - p) for p in (batch - 1, batch, 256, 4)])


@pytest.mark.parametrize("k", [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128])
def test_no_spurious_change_inside_a_run(plan, k):
    """Runs of every phase against the map's 4-, 8- and 32-symbol steps, repeated over several segments; single other bytes between them."""
    unit = b"a" * k + b"b"
    reps = 9000 // len(unit) + 1
    _check_bytes([unit * reps], RUNS)
    _check_bytes([unit * reps, b"b" + (unit * reps)[:-1], b"a" * (len(unit) * reps)], RUNS)
