"""The resolve phase of the wave-per-record encode kernel (encode_flow_kernel): every lane's first chain walk starts up to two
blocks ahead of its own, at the first claimed position of the farthest of those blocks that holds one, and the correction loop
only repairs what is left.  Whatever the first guesses are the result is the sequential parse, so every case compares with the
oracle, bit for bit, under plan 2 (blocks of 64 positions) and plan 3 (blocks of 128), at batch 1 - 4.  (That the guesses are
good is a matter of speed, not of results: the passes-per-segment counter of scripts/dev_prof_encode.py shows it.)"""
import os

import numpy as np
import pytest

from helpers import load_tokenizer, oracle_batch, random_merges
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ecg_byte_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "HIP extension not built -- no fallback exists"
    return torch.device("cuda", 0)


@pytest.fixture(params=[2, 3], ids=["plan-wave", "plan-wave-long-segments"])
def plan(request, dev):
    """Forces the wave-per-record kernel at any batch size: 16 waves with 64-position blocks, 8 waves with 128-position blocks."""
    from ecg_byte_amd.tokenizer import set_encode_plan
    set_encode_plan(request.param)
    yield request.param
    set_encode_plan(0)


@pytest.fixture(scope="module")
def c2():
    _, merges, pc = load_tokenizer("c2")
    from ecg_byte_amd import synth
    x = synth.synth_ecg(3, 5000, seed=11)
    return merges, pc, O.Trie(merges), x


def _check_bytes(merges, texts):
    """texts: equal-length byte strings, one batch; each against lib.rs's restatement."""
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


AB = [([97, 98], 256)]
# block edges (64 / 128 positions), and the segment lengths the two plans pick for a trie this small (62 x 64 = 3 968 and 126 x 64 = 8 064
# symbols), bracketed: S - 1, S, S + 1, 2 S + 1
AB_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 3967, 3968, 3969, 7937, 8063, 8064, 8065, 16129]


@pytest.mark.parametrize("n", AB_LENGTHS)
def test_mis_phased_chunks_at_block_and_segment_edges(plan, n):
    """'ab' over 'babab...' and 'abab...a': a parse that starts at the wrong phase never meets the real chain, so the position the
    lead-in walk starts from is a speculative one in every block."""
    p1 = (b"b" + b"ab" * (n // 2 + 1))[:n]
    p2 = (b"ab" * (n // 2 + 1))[:n]
    for batch in ([p1], [p2], [p1, p2, p1], [p2, p1, p2, p1]):
        _check_bytes(AB, batch)


RUNS = [([97] * k, 256 + k - 2) for k in range(2, 129)] + [([97] * 200, 400)]     # a^2 .. a^128 and a^200: within the kernel's 225-symbol limit


@pytest.mark.parametrize("n", [129, 200, 513, 4001])
def test_blocks_without_a_claimed_position(plan, n):
    """Tokens longer than a block: the left neighbour's block holds no claimed position (the lane keeps its own guess), the chain
    jumps over whole blocks."""
    _check_bytes(RUNS, [b"a" * n])


def test_long_tokens_between_single_bytes_and_a_carry_deep_in_the_next_segment(plan):
    n = 201 * 20
    _check_bytes(RUNS, [(b"a" * 200 + b"b") * 20])
    _check_bytes(RUNS, [(b"a" * 200 + b"b") * 20, (b"a" * 199 + b"bb") * 20, (b"b" + b"a" * 200) * 20, b"a" * n])
    # two and three segments under either plan: the carry of a 200-symbol token lands up to three blocks into the next segment
    _check_bytes(RUNS, [(b"a" * 200 + b"b") * 90, (b"a" * 200) * 90 + b"b" * 90])


@pytest.mark.parametrize("n", [133, 300, 4100])
def test_unmatched_bytes_where_the_lead_in_walks(plan, n):
    """Bytes that occur in no merge (one position each, no length byte) at positions 60 - 70 and 124 - 132, between ordinary tokens:
    the walk towards the own block steps over them one by one, as the walk inside the block does."""
    rng = np.random.default_rng(n)
    merges = random_merges(rng, 120, alphabet=b"abcd", max_len=7)
    spots = list(range(60, 71)) + list(range(124, 133))
    texts = []
    for pick in (spots, spots[::2], [63, 64, 127, 128], [61, 66, 125, 130]):
        buf = bytearray(bytes(rng.choice(np.frombuffer(b"aabbcd", dtype=np.uint8), size=n)))
        for k, p in enumerate(pick):
            buf[p] = b"X~"[k & 1]
        texts.append(bytes(buf))
    _check_bytes(merges, texts[:1])
    _check_bytes(merges, texts)


@pytest.mark.parametrize("samples", [5000, 1, 5, 53])
def test_headline_path_at_small_size(plan, c2, samples):
    """The benchmark's path (float64 records, C2 tokenizer and percentiles) on three records and on their first 1, 5 and 53 samples
    per lead."""
    from ecg_byte_amd.tokenizer import HipTokenizer
    merges, pc, trie, x = c2
    xs = np.ascontiguousarray(x[:, :, :samples])
    tk = HipTokenizer(merges)
    ref = oracle_batch(trie, xs, pc)
    for B in (1, 3):
        ids, counts = tk.quantize_encode(torch.from_numpy(xs[:B]).cuda(), pc)
        ids, counts = ids.cpu().numpy(), counts.cpu().numpy()
        for b in range(B):
            assert counts[b] == ref[b].size, (samples, b)
            assert np.array_equal(ids[b, : counts[b]].astype(np.uint32), ref[b]), (samples, b)
