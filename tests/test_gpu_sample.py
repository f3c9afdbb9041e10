"""GPU tests of the device sampler (csrc/sample.hip, ecgb_sample_bf16): the drawn token against the per-token float64 restatement of the rule (tests/sample_ref.py) for
explicit uniforms and for the Philox path, repeatability, the "nothing drawable" flag, the drawn distribution, and HipCausalLM.generate(device_sampler=True): the
replayed graph equals the eager loop, is captured once and takes each call's seed and nonce.

Tolerance of the explicit-u comparison: device and restatement differ only by float64 `exp` and by the order of float64 sums over <= 65 536 groups (about 1e-11 in
probability), so a case may be left out only when u lies within 1e-9 of a boundary between two kept entries -- at most 1 in 1 000 per configuration."""
import numpy as np
import pytest

import sample_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CONFIGS = lambda n: [(0.6, 50, 0.9), (0.6, 0, 0.9), (1, 0, 1), (0.7, 12, 0.8), (1e-3, 50, 0.9), (100, 5, 1), (1, 1, 1), (1, n, 1), (1, n + 5, 1), (1, 0, 1e-6)]
ROWS = ["n1", "n7", "n8", "n257", "n8191", "n8193", "padded", "neginf", "constant", "zeros", "posinf"]


@pytest.fixture(scope="module")
def ops():
    from ecg_byte_amd import decoder_ops
    return decoder_ops


def _row(kind):
    """(bf16 bits [ld], n) of one test row: bf16-rounded normal logits unless said."""
    rng = np.random.default_rng(ROWS.index(kind))
    n = {"padded": 5003, "neginf": 2049, "constant": 70001, "zeros": 515, "posinf": 1030}.get(kind) or int(kind[1:])
    ld = 5056 if kind == "padded" else n
    x = rng.standard_normal(ld).astype(np.float32)
    if kind == "padded":
        x[n:] = 50.0                                                       # the padded head's columns: never candidates
    elif kind == "neginf":
        x[rng.choice(n, 100, replace=False)] = -np.inf
    elif kind == "constant":
        x[:] = 1.25                                                        # one key holds 70 001 entries: the cuts fall inside the tie group
    elif kind == "zeros":
        x[::3], x[1::6] = 0.0, -0.0
    elif kind == "posinf":
        x[77] = np.inf
    return R.bf16_round(x)[1], n


def _bf16(bits, rows):
    return torch.from_numpy(np.tile(bits.view(np.int16), (rows, 1))).cuda().view(torch.bfloat16)


def _values(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


@pytest.mark.parametrize("kind", ROWS)
def test_explicit_u_against_the_float64_rule(ops, kind):
    """1 007 uniforms per configuration (0 and 1 - 2^-53 among them) in launches of 1, 3 and 17 rows: the token is the restatement's."""
    bits, n = _row(kind)
    xs = {rows: _bf16(bits, rows) for rows in (1, 3, 17)}
    scratch = {rows: ops.sample_scratch(rows, "cuda") for rows in xs}
    rng = np.random.default_rng(100 + ROWS.index(kind))
    for T, K, P in CONFIGS(n):
        row = R.Row(_values(bits), n, T, K, P)
        us = np.concatenate([[0.0, 1.0 - 2.0 ** -53], rng.random(1005)])
        ut = torch.from_numpy(us).cuda()
        got, lo = [], 0
        for rows in [1, 3] + [17] * 59:
            got.append(ops.sample_rows(xs[rows], n, T, K, P, None, 0, scratch[rows], u=ut[lo:lo + rows].contiguous()))
            lo += rows
        assert lo == us.size
        got = torch.cat(got).cpu().numpy()
        for s in scratch.values():
            ops.sample_check(s)
        want, dist = row.draw(us)
        assert got.min() >= 0 and got.max() < n
        off = got != want
        left_out = int((off & (dist < 1e-9)).sum())
        print(f"{kind} T={T} k={K} p={P}: kept {row.ids.size}, differ {int(off.sum())}, left out {left_out}, smallest distance {dist.min():.3g}")
        assert not (off & (dist >= 1e-9)).any(), (kind, T, K, P, us[off][:4], got[off][:4], want[off][:4], dist[off][:4])
        assert left_out <= 1, (kind, T, K, P, left_out)


def test_same_launch_same_tokens(ops):
    bits, n = _row("n8193")
    x, scratch = _bf16(bits, 17), ops.sample_scratch(17, "cuda")
    seed2 = torch.tensor([12345, 678], dtype=torch.int64, device="cuda")
    first = ops.sample_rows(x, n, 0.6, 50, 0.9, seed2, 9, scratch)
    for _ in range(19):
        assert torch.equal(ops.sample_rows(x, n, 0.6, 50, 0.9, seed2, 9, scratch), first)
    assert len(set(first.tolist())) > 1                                    # (rows differ: the row index is part of the counter)


def test_nothing_drawable_raises(ops):
    bits, n = _row("n257")
    x = _bf16(bits, 3).clone()
    x[1, ::2], x[1, 1::2] = float("nan"), float("-inf")
    scratch = ops.sample_scratch(3, "cuda")
    out = ops.sample_rows(x, n, 0.6, 50, 0.9, None, 0, scratch, u=torch.full((3,), 0.5, dtype=torch.float64, device="cuda"))
    assert int(out[1]) == 0 and int(scratch[0]) != 0
    want = R.Row(_values(bits), n, 0.6, 50, 0.9).draw([0.5])[0][0]
    assert int(out[0]) == want and int(out[2]) == want                     # the other rows are drawn as usual
    with pytest.raises(RuntimeError, match="no drawable"):
        ops.sample_check(scratch)
    ops.sample_check(scratch)                                              # cleared by the check
    from ecg_byte_amd._lib import EcgbError
    for bad in (dict(temperature=0.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(n=n + 1)):
        kw = dict(n=n, temperature=1.0, top_k=0, top_p=1.0)
        kw.update(bad)
        with pytest.raises(EcgbError):
            ops.sample_rows(x, kw["n"], kw["temperature"], kw["top_k"], kw["top_p"], None, 0, scratch, u=torch.zeros(3, dtype=torch.float64, device="cuda"))


def test_generator_path_is_philox_of_seed_nonce_row_step(ops):
    """u_dev = NULL: the token is the restatement's for the u the host Philox gives for (seed, nonce, row, step) -- step as an argument and as a device word."""
    bits, n = _row("n8191")
    rows = 17
    x, scratch = _bf16(bits, rows), ops.sample_scratch(rows, "cuda")
    row = R.Row(_values(bits), n, 1.0, 0, 1.0)
    seen = set()
    for seed, nonce, step in [(5, 77, 600), (6, 77, 600), (5, 78, 600), (5, 77, 601), (2 ** 64 - 3, 2 ** 63 + 11, 2 ** 31 - 1)]:
        signed = lambda v: v - 2 ** 64 if v >= 2 ** 63 else v
        seed2 = torch.tensor([signed(seed), signed(nonce)], dtype=torch.int64, device="cuda")
        us = np.array([R.uniform(seed, nonce, r, step) for r in range(rows)])
        want, dist = row.draw(us)
        assert dist.min() > 1e-9
        got = ops.sample_rows(x, n, 1.0, 0, 1.0, seed2, step, scratch)
        assert np.array_equal(got.cpu().numpy(), want), (seed, nonce, step)
        got_dev = ops.sample_rows(x, n, 1.0, 0, 1.0, seed2, torch.tensor([step], dtype=torch.int32, device="cuda"), scratch)
        assert torch.equal(got_dev, got)
        seen.add(tuple(us))
    assert len(seen) == 5                                                  # each of seed, nonce, step changes u (and the row does: 17 different u per launch)
    assert len(set(next(iter(seen)))) == rows


def _load_generate():
    from test_gpu_decoder_model import _load_generate as load
    return load()


def _prompt(zg):
    return torch.from_numpy(zg["input_ids"]).cuda(), torch.from_numpy(zg["attention_mask"]).cuda()


def test_drawn_distribution_on_the_generate_fixture(ops):
    """T 0.7, k 12, p 0.8 on the fixture's first-step logits, 4 000 draws (500 rows x 8 steps of one seed): nothing outside the kept set, max |freq - want| < 0.04
    (the numbers and the tolerance of test_generate_sampling_follows_the_warped_distribution)."""
    zg, m = _load_generate()
    ids, mask = _prompt(zg)
    _, lg = m.generate(input_ids=ids[:1], attention_mask=mask[:1], max_new_tokens=1, pad_token_id=299, return_logits=True)
    x16 = lg[0, 0].to(torch.bfloat16)
    assert torch.equal(x16.float(), lg[0, 0])
    V = x16.numel()
    row = R.Row(x16.float().cpu().numpy().astype(np.float64), V, 0.7, 12, 0.8)
    want = np.zeros(V)
    want[row.ids] = np.diff(np.concatenate([[0.0], row.cum])) / row.cum[-1]
    x, scratch = x16[None].repeat(500, 1).contiguous(), ops.sample_scratch(500, "cuda")
    seed2 = torch.tensor([5, 1], dtype=torch.int64, device="cuda")
    draws = torch.cat([ops.sample_rows(x, V, 0.7, 12, 0.8, seed2, step, scratch) for step in range(8)])
    ops.sample_check(scratch)
    freq = np.bincount(draws.cpu().numpy(), minlength=V) / draws.numel()
    assert freq[want == 0].sum() == 0.0
    print("max |freq - want|", np.abs(freq - want).max(), "kept", row.ids.size)
    assert np.abs(freq - want).max() < 0.04


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def test_generate_top_k_1_is_greedy_and_needs_do_sample():
    zg, m = _load_generate()
    ids, mask = _prompt(zg)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=8, pad_token_id=299)
    greedy = m.generate(**kw)
    for use_graph in (True, False):
        assert torch.equal(m.generate(do_sample=True, top_k=1, device_sampler=True, use_graph=use_graph, **kw), greedy)
    with pytest.raises(ValueError):
        m.generate(device_sampler=True, **kw)


def test_generate_graph_equals_eager_and_is_captured_once():
    zg, m = _load_generate()
    ids, mask = _prompt(zg)
    sam = dict(do_sample=True, temperature=1.5, top_k=50, top_p=0.95, device_sampler=True, pad_token_id=299)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=20, **sam)
    a = m.generate(generator=_gen(7), **kw)                                # the default of this mode: the replayed graph
    assert len(m._gen_graphs) == 1
    assert torch.equal(a, m.generate(generator=_gen(7), use_graph=True, **kw))
    assert torch.equal(a, m.generate(generator=_gen(7), use_graph=False, **kw))
    g = _gen(7)
    assert torch.equal(a, m.generate(generator=g, **kw)) and not torch.equal(a, m.generate(generator=g, **kw))      # successive calls differ: another nonce
    # another prompt length and token count under the same rounded capacity: the same captured step, with this call's seed and nonce
    kw2 = dict(input_ids=ids[:, 3:], attention_mask=mask[:, 3:], max_new_tokens=17, **sam)
    b = m.generate(generator=_gen(8), **kw2)
    assert len(m._gen_graphs) == 1
    assert torch.equal(b, m.generate(generator=_gen(8), use_graph=False, **kw2))
    # the device's default generator, as main's five-seed loop seeds it
    torch.manual_seed(3)
    c = m.generate(**kw)
    torch.manual_seed(3)
    assert torch.equal(c, m.generate(use_graph=False, **kw))
    assert len(m._gen_graphs) == 1
    greedy = m.generate(input_ids=ids, attention_mask=mask, max_new_tokens=20, pad_token_id=299)
    assert len(m._gen_graphs) == 2 and not torch.equal(greedy, a)


def test_generate_seeds_differ_on_a_batch_of_64():
    zg, m = _load_generate()
    ids, mask = _prompt(zg)
    kw = dict(input_ids=ids[:1].repeat(64, 1), attention_mask=mask[:1].repeat(64, 1), max_new_tokens=4, pad_token_id=299, do_sample=True, temperature=1.0, top_k=0,
              top_p=1.0, device_sampler=True)
    a, b = m.generate(generator=_gen(1), **kw), m.generate(generator=_gen(2), **kw)
    assert not torch.equal(a, b)
    assert len({tuple(r.tolist()) for r in a[:, -4:]}) > 1                 # and the rows of one call differ
    assert torch.equal(a, m.generate(generator=_gen(1), **kw))             # re-seeding reproduces the run


def test_generate_eos_ends_and_pads_rows():
    zg, m = _load_generate()
    ids, mask = _prompt(zg)
    S0 = ids.shape[1]
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=16, pad_token_id=299, do_sample=True, temperature=1.0, top_k=4, top_p=1.0, device_sampler=True)
    free = m.generate(generator=_gen(4), **kw)[:, S0:]
    eos = int(torch.bincount(free[:, 1:].reshape(-1)).argmax())             # a token the free run draws often
    out = m.generate(generator=_gen(4), eos_token_id=eos, **kw)
    assert torch.equal(out, m.generate(generator=_gen(4), eos_token_id=eos, use_graph=False, **kw))
    out, ended = out[:, S0:].cpu().numpy(), 0
    for got, want in zip(out, free.cpu().numpy()):
        hits = np.nonzero(want[:got.size] == eos)[0]
        k = int(hits[0]) if hits.size else got.size - 1
        ended += bool(hits.size)
        assert (got[:k + 1] == want[:k + 1]).all() and (got[k + 1:] == 299).all()
    assert ended > 0


def test_default_sampling_path_is_untouched():
    """device_sampler left at None: the torch path's tokens for a fixed seed, on a model that used the sampler before as on one that never did."""
    zg, m = _load_generate()
    _, m2 = _load_generate()
    ids, mask = _prompt(zg)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=10, pad_token_id=299, do_sample=True, temperature=0.7, top_k=12, top_p=0.8)
    m2.generate(generator=_gen(5), device_sampler=True, **kw)
    for extra in (dict(), dict(device_sampler=False)):
        assert torch.equal(m.generate(generator=_gen(5), **kw, **extra), m2.generate(generator=_gen(5), **kw, **extra)), extra
    assert not any(hasattr(st, "seed2") for st in m.__dict__.get("_gen_graphs", {}).values())   # no sampler state on the model that never asked for it
