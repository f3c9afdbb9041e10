"""A decode step's attention at the cache lengths where a batch of its loops begins, ends or is empty.  Every form of it (csrc/attention_decode.hip: one workgroup a
head, keys split over workgroups, RoPE + append + split in one launch; csrc/decode.hip: all heads of a KV group a workgroup) is made of the routines of
csrc/decode_attn.inc: a wave takes 16 keys a batch (16 waves in the one-workgroup kernel, 4 in the split kernels), a thread 8 value rows a batch (1024 / 512 / 256 keys a
batch of the one-workgroup kernel at head_dim 64 / 128 / 256, 256 / 128 / 64 of a split).  Reference: softmax(q.K^T * scale + mask) . V in fp32 with P cast to bf16, as
tests/test_gpu_decoder_ops.py::test_decode_attention_single_and_split_kernels forms it and at its tolerance; between the forms: the same bits."""
import math

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SINGLE_LENGTHS = {64: [1, 15, 16, 17, 255, 256, 257, 1023, 1025], 128: [1, 15, 16, 17, 255, 256, 257], 256: [1, 15, 16, 17, 255, 256, 257, 513]}
# (keys, splits): a split of 1 / 63 / 64 / 65 keys; the newest key alone in the last split (65 = 8 * 8 + 1); more splits than keys; 256 / 257 keys a split
SPLIT_CASES = [(7, 7), (630, 10), (640, 10), (650, 10), (65, 9), (5, 8), (512, 2), (514, 2)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from ecg_byte_amd import decoder_ops
    return decoder_ops


def _inputs(ops, D, Hq, Hkv, B, n):
    """Raw q|k|v of the step, the cache before it, the mask (row 0 left-padded), the RoPE tables; the rotated q|k|v and the cache after the append; the fp32 reference."""
    g = torch.Generator(device="cuda").manual_seed(1000 * D + 10 * n + B)
    cap = n + 11
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda", generator=g).to(torch.bfloat16)
    cache = (torch.randn(B, cap, 2 * Hkv * D, device="cuda", generator=g) * 0.7).to(torch.bfloat16)
    mask = torch.ones(B, cap, device="cuda")                    # ones past the length too: those rows must not be read
    pad = min(3, n - 1)
    mask[0, :pad] = 0
    if n > 40:
        mask[B - 1, 20:24] = 0
    fr = torch.rand(B, D // 2, device="cuda", generator=g) * 50.0
    cos, sin = fr.cos().contiguous(), fr.sin().contiguous()
    q2, c2 = qkv.clone(), cache.clone()
    ops.rope_append_(q2, cos, sin, Hq, Hkv, D, c2, n)
    q = q2[:, :Hq * D].float().view(B, Hq, D)
    k = c2[:, :n, :Hkv * D].float().view(B, n, Hkv, D).repeat_interleave(Hq // Hkv, dim=2)
    v = c2[:, :n, Hkv * D:].float().view(B, n, Hkv, D).repeat_interleave(Hq // Hkv, dim=2)
    s = torch.einsum("bhd,bnhd->bhn", q, k) * D ** -0.5
    s = s.masked_fill(mask[:, None, :n] == 0, float("-inf"))
    p = torch.softmax(s, dim=-1).to(torch.bfloat16).float()
    want = torch.einsum("bhn,bnhd->bhd", p, v).reshape(B, Hq * D)
    return qkv, cache, mask, cos, sin, q2, c2, want


def _close(got, want, what):
    err, bound = (got.float() - want).abs().max().item(), 2e-2 * want.abs().max().item() + 1e-3
    assert err <= bound, (what, err, bound)


def _single(ops, D, Hq, Hkv, B, n, q2, c2, mask, want):
    n_dev = torch.full((1,), n, dtype=torch.int32, device="cuda")
    one = ops.attn_decode(q2, c2, mask, n, Hq, Hkv, D, D ** -0.5)
    _close(one, want, ("attn_decode", n))
    dyn = ops.attn_decode_dyn(q2, c2, mask, n_dev, Hq, Hkv, D, D ** -0.5)
    _close(dyn, want, ("attn_decode_dyn", n))
    assert torch.equal(one, dyn), n


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (2, 2)], ids=["gqa4", "mha"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_one_workgroup_form_at_the_ends_of_its_batches(ops, D, Hq, Hkv, B):
    for n in SINGLE_LENGTHS[D]:
        _, _, mask, _, _, q2, c2, want = _inputs(ops, D, Hq, Hkv, B, n)
        _single(ops, D, Hq, Hkv, B, n, q2, c2, mask, want)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (2, 2)], ids=["gqa4", "mha"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_split_forms_at_the_ends_of_their_batches(ops, D, Hq, Hkv, B):
    scale = 1.0 / math.sqrt(D)
    for n, ns in SPLIT_CASES:
        qkv, cache, mask, cos, sin, q2, c2, want = _inputs(ops, D, Hq, Hkv, B, n)
        cap = cache.shape[1]
        n_dev = torch.full((1,), n, dtype=torch.int32, device="cuda")
        _single(ops, D, Hq, Hkv, B, n, q2, c2, mask, want)
        split = ops.attn_decode_split(q2, c2, mask, n, Hq, Hkv, D, scale, ns)
        _close(split, want, ("attn_decode_split", n, ns))
        own = ops.decode_split_scratch(cap, B, Hq, D, ns, "cuda")
        split_dyn = ops.attn_decode_split(q2, c2, mask, n_dev, Hq, Hkv, D, scale, ns, scratch=own)
        _close(split_dyn, want, ("attn_decode_split_dyn", n, ns))
        assert torch.equal(split_dyn, split), (n, ns)
        # RoPE + append + attention from the raw projection: the split kernels' bits, the appended cache row included
        assert ops.decode_one_ok(B, Hq, D, ns, cap)
        scratch = ops.decode_one_scratch(B, Hq, D, ns, "cuda")
        for kv in (n, n_dev):
            c1 = cache.clone()
            one = ops.attn_decode_one(qkv, cos, sin, c1, mask, kv, Hq, Hkv, D, scale, ns, scratch=scratch)
            _close(one, want, ("attn_decode_one", n, ns))
            assert torch.equal(one, split) and torch.equal(c1, c2), (n, ns)
            # the scratch is back in its empty state: counters zero, statistics "not stored yet"
            assert float(scratch[-2 * B * Hq:].abs().max()) == 0.0 and bool((scratch.view(torch.int32)[: B * Hq * ns * 2] == 0x7FC0DEAD).all()), (n, ns)
        grouped_scratch = ops.decode_attn_scratch(cap, B, Hq, Hkv, D, ns, "cuda")
        for kv in (n, n_dev):
            c1 = cache.clone()
            grouped = ops.decode_attn(qkv.clone(), cos, sin, c1, mask, kv, Hq, Hkv, D, scale, ns, grouped_scratch)
            _close(grouped, want, ("decode_attn", n, ns))
            assert torch.equal(grouped, split) and torch.equal(c1, c2), (n, ns)
