"""CPU tests around the device sampler (csrc/sample.hip): the generator's block function against Random123's known answers, the CLI flag, and the float64
restatement of the rule (tests/sample_ref.py) against the torch code of HipCausalLM._next_token.  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest

import sample_ref as R


@pytest.fixture(scope="module")
def lib():
    from ecg_byte_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


# Random123 (examples/kat_vectors): philox4x32 10 rounds
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(lib, ctr, key, want):
    out = (C.c_uint32 * 4)()
    assert lib.ecgb_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out) == 0
    assert tuple(out) == want
    assert tuple(R.philox4x32_10(ctr, key)) == want                        # and the restatement the GPU tests feed the rule with
    assert lib.ecgb_philox4x32_10(None, (C.c_uint32 * 2)(*key), out) != 0


def test_uniform_is_53_bits_of_the_first_two_words():
    o = R.philox4x32_10([3, 46, 0x9abcdef0, 0x12345678], [0x55667788, 0x11223344])
    u = R.uniform(0x1122334455667788, 0x123456789abcdef0, 3, 46)
    assert u == ((o[0] << 32 | o[1]) >> 11) / 2.0 ** 53 and 0.0 <= u < 1.0
    others = {R.uniform(0x1122334455667789, 0x123456789abcdef0, 3, 46), R.uniform(0x1122334455667788, 0x123456789abcdef1, 3, 46),
              R.uniform(0x1122334455667788, 0x123456789abcdef0, 4, 46), R.uniform(0x1122334455667788, 0x123456789abcdef0, 3, 47)}
    assert u not in others and len(others) == 4


def test_sample_scratch_bytes(lib):
    assert lib.ecgb_sample_scratch_bytes(1) >= 4 and lib.ecgb_sample_scratch_bytes(17) >= 4


def test_parser_accepts_device_sampler():
    from ecg_byte_amd import main
    assert main.get_args([]).device_sampler is False
    assert main.get_args(["--inference", "--device_sampler"]).device_sampler is True


def test_llm_wrapper_passes_the_flag_on():
    from types import SimpleNamespace
    torch = pytest.importorskip("torch")
    from ecg_byte_amd.llm import LLM
    seen = {}

    class Fake(torch.nn.Module):
        device = torch.device("cpu")

        def generate(self, **kw):
            seen.update(kw)
            return kw["input_ids"]

    tok = SimpleNamespace(pad_token_id=1, eos_token_id=2, batch_decode=lambda ids, **kw: ["x"])
    batch = {"tokenized_signal": torch.zeros((1, 4), dtype=torch.long), "attn_mask": torch.ones((1, 4))}
    LLM(Fake(), SimpleNamespace(device_sampler=True)).generate(batch, tok)
    assert seen["device_sampler"] is True
    LLM(Fake(), SimpleNamespace()).generate(batch, tok)
    assert seen["device_sampler"] is None


def test_rule_edges_in_the_restatement():
    x = np.array([1.0, np.nan, -np.inf, 3.0, 3.0, -0.0, 0.0, 2.0])
    row = R.Row(x, 8, 1.0, 0, 1.0)
    assert row.drawable == 6 and list(row.ids) == [3, 4, 7, 0, 5, 6]         # value descending, id ascending; -0 ties with +0
    assert list(R.Row(x, 8, 1.0, 1, 1.0).ids) == [3, 4]                      # top-k keeps the tie with the k-th value
    assert list(R.Row(x, 8, 1.0, 0, 1e-6).ids) == [3]                        # the first entry always stays
    tok, dist = R.Row(x, 8, 1.0, 2, 1.0).draw([0.0, 0.49, 0.51, 1 - 2.0 ** -53])
    assert list(tok) == [3, 3, 4, 4] and np.allclose(dist, [0.5, 0.01, 0.01, 0.5])
    assert list(R.Row(np.array([1.0, np.inf, 5.0, np.inf]), 4, 0.6, 0, 1.0).ids) == [1, 3]      # +inf: weight 1, the rest 0 and behind the cut
    assert R.Row(np.array([np.nan, -np.inf]), 2, 1.0, 0, 1.0).drawable == 0
    assert list(R.Row(np.array([0.0, 9.0, 50.0]), 2, 1.0, 0, 1.0).ids) == [1, 0]                  # columns past n are not candidates


def test_restatement_keeps_the_set_of_next_token(monkeypatch):
    """The kept set of rules 1-4 = the entries `_next_token`'s torch code leaves a probability, on CPU rows of fp32 logits (no ties).  The torch code works in fp32:
    rows whose top-p cut lies within 1e-4 (probability) of an entry's cumulative weight are left out, at most one in four."""
    torch = pytest.importorskip("torch")
    from ecg_byte_amd.decoder import HipCausalLM
    seen = []
    monkeypatch.setattr(torch, "multinomial", lambda probs, k, generator=None: (seen.append(probs.clone()), torch.zeros((probs.shape[0], 1), dtype=torch.long))[1])
    rng = np.random.default_rng(11)
    used = total = 0
    for T, K, P in [(0.6, 50, 0.9), (0.7, 12, 0.8), (1.0, 0, 0.5), (0.6, 0, 0.9), (1.0, 5, 1.0), (2.0, 400, 0.95)]:
        for _ in range(20):
            x = (2.0 * rng.standard_normal(300)).astype(np.float32)
            row = R.Row(x.astype(np.float64), 300, T, K, P)
            total += 1
            if row.margin < 1e-4:
                continue
            used += 1
            HipCausalLM._next_token(None, torch.from_numpy(x)[None], True, T, K, P, None)
            assert set(np.nonzero(seen.pop()[0].numpy() > 0)[0]) == set(row.ids.tolist()), (T, K, P)
    assert used * 4 >= total * 3, (used, total)
