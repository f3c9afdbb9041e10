"""Fused attention with dropout on the probabilities (ecgb_attn_fwd_dropout / ecgb_attn_bwd_dropout, ops.attn_fwd / attn_bwd with drop=(p, seed),
HipGPT2LM.fused_attention_dropout): the mask bit for bit against the numpy rule of tests/dropout_ref.py and against the mask ops.dropout draws on
a materialised [B Hq, S, S] tensor; forward and gradients against float64 with that mask; determinism; p = 0; the GPT-2 block against the fp32
oracle and against the materialised-scores path.

Shapes (unless a test says otherwise): B 2, p 0.25, S in {64, 200, 257} -- one tile; a partial 64-key tile with a partial 128-row block; a last
block of one row -- query / KV heads 3/3 and 4/2, batch row 1 left-padded by 65 keys (at S 64 the whole row: rows without a visible key).

The float64 bound.  e0 is the norm-relative error (whole_rel of tests/test_gpu_attention_fp64.py: || x - ref || / || row magnitudes ||) of the same kernel
family's p = 0 kernels -- the register-staged ones, ecgb_set_attn_fwd_staging(0) -- against the float64 reference without dropout on the same inputs;
e_drop the same quantity of the dropout kernels against the float64 reference with Z = kept / (1 - p) (magnitudes with Z in them).  Required:
    e_drop <= 2 / (1 - p) * e0 + 1e-4
1 / (1 - p): every surviving probability carries its bf16 rounding with 1 / (1 - p) the weight; 2: headroom for the smaller number of terms per row;
1e-4: the additive constant LEAN_VS_ROUND2 of that file uses.  Measured ratios e_drop / e0: EXPERIMENTS.md."""
import math

import numpy as np
import pytest

from dropout_ref import attn_keep

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

P = 0.25
D = 64
SCALE = 1.0 / 8.0
LENGTHS = (64, 200, 257)
HEADS = ((3, 3), (4, 2))
LPAD = 65
B = 2


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from ecg_byte_amd import decoder_ops
    return decoder_ops


def _mask(S):
    m = torch.ones(B, S, device="cuda")
    m[1, : min(LPAD, S)] = 0
    return m


def _visible(mask, S):
    """bool [B, 1, S, S]: key j visible to query i."""
    return torch.tril(torch.ones(S, S, dtype=torch.bool, device="cuda"))[None, None] & (mask[:, None, None, :] != 0)


def _keep(p, seed, Hq, S):
    return torch.from_numpy(attn_keep(p, seed, B, Hq, S)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# the mask, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("S", LENGTHS)
def test_mask_bits_are_the_numpy_rule(ops, S, Hq, Hkv):
    """q = k = 0 and v_j = e_(j mod 64): every visible key weighs 1 / nvis_i, so O[i, c] nvis_i (1 - p) counts the kept visible keys of class c in
    row i (at most 5 at these lengths; the bf16 rounding of O moves the product by less than 0.03).  At S 64 a class is one key: every bit."""
    seed = 1234 + S
    qkv = torch.zeros(B * S, (Hq + 2 * Hkv) * D, dtype=torch.bfloat16, device="cuda")
    x = qkv.view(B, S, Hq + 2 * Hkv, D)
    j = torch.arange(S, device="cuda")
    x[:, j, Hq + Hkv:, j % 64] = 1.0
    mask = _mask(S)
    o, _ = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, SCALE, drop=(P, seed))
    vis = _visible(mask, S)
    nvis = vis.sum(-1).double()                                                          # [B, 1, S]
    got = o.view(B, S, Hq, D).permute(0, 2, 1, 3).double() * nvis[..., None] * (1 - P)   # [B, Hq, S, 64]
    cls = torch.nn.functional.one_hot(j % 64, 64).double()                               # [S, 64]
    want = ((_keep(P, seed, Hq, S) & vis).double() @ cls)                                # kept visible keys per class
    assert float(want.max()) <= 5
    assert float((got - got.round()).abs().max()) < 0.03
    assert torch.equal(got.round(), want), f"{int((got.round() != want).sum())} of {want.numel()} counts differ"
    assert float(want.sum()) > 0 and float(((~_keep(P, seed, Hq, S)) & vis).sum()) > 0   # the test saw kept and dropped keys


@pytest.mark.parametrize("S", LENGTHS)
def test_materialised_path_draws_the_same_mask(ops, S):
    """ops.dropout on an all-ones [B Hq, S, S] tensor keeps exactly the elements tests/dropout_ref.py keeps: the fused kernels (above) and the
    materialised-scores path read one mask from one (p, seed)."""
    Hq, seed = 4, 77
    ones = torch.ones(B * Hq, S, S, dtype=torch.bfloat16, device="cuda")
    d = ops.dropout(ones, P, seed)
    assert torch.equal(d.view(B, Hq, S, S) != 0, _keep(P, seed, Hq, S))
    kept = d[d != 0].float()
    assert bool((kept == float(torch.tensor(1.0 / (1.0 - P)).to(torch.bfloat16))).all())


def test_mask_index_past_32_bits(ops):
    """B 2 x 4 query heads x S 23 233: the flat index of the last heads' elements is past 2^32 (8 S^2 = 4.32e9), of the others past 2^31.  Only the
    last 64 keys are visible (left padding), so the 64 live rows see at most one key per class j mod 64 and every bit of their mask shows:
      forward  q = 0, v_j = e_(j mod 64):                 O[i, c] nvis_i (1 - p) = the bit of (i, the visible key of class c);
      dQ       k_j = e_(j mod 64), dO = ones (dO.v = 1):   dQ[i, c] = scale P_ij (Z_ij - delta_i), delta_i = sum_c O[i, c] -> the same bit;
      dK/dV    dO_i = e_(i mod 64):                        dV[j, c] nvis_i (1 - p) = the bits of (the live row i of class c, j) summed over the two query
                                                            heads of the KV group (the mask index uses the query head)."""
    from dropout_ref import mix32, threshold
    Hq, Hkv, S, seed = 4, 2, 23233, 4242
    G, T = Hq // Hkv, S - 64
    qkv = torch.zeros(B * S, (Hq + 2 * Hkv) * D, dtype=torch.bfloat16, device="cuda")
    x = qkv.view(B, S, Hq + 2 * Hkv, D)
    j = torch.arange(S, device="cuda")
    x[:, j, Hq:, j % 64] = 1.0                                                            # k and v
    mask = torch.ones(B, S, device="cuda")
    mask[:, :T] = 0
    # numpy: keep[b, hq, r, t] for query T + r, key T + t
    b_, h_, r_, t_ = np.meshgrid(np.arange(B), np.arange(Hq), np.arange(64), np.arange(64), indexing="ij")
    idx = ((b_ * Hq + h_).astype(np.uint64) * np.uint64(S) + (T + r_).astype(np.uint64)) * np.uint64(S) + (T + t_).astype(np.uint64)
    assert int(idx[1, 3].min()) > 2 ** 32 and 2 ** 31 < int(idx[0, 3].min()) and int(idx[0, 3].max()) < 2 ** 32
    vis = torch.tril(torch.ones(64, 64, dtype=torch.bool, device="cuda"))
    bits = (torch.from_numpy(mix32(seed, idx) >= threshold(P)).cuda() & vis).double()     # [B, Hq, 64 rows, 64 keys]
    nvis = torch.arange(1, 65, device="cuda").double()                                    # row T + r sees r + 1 keys
    cls = ((T + torch.arange(64, device="cuda")) % 64)                                    # class of key / row T + t
    o, lse = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, SCALE, drop=(P, seed))
    ov = o.view(B, S, Hq, D)
    assert bool((ov[:, :T] == 0).all())                                                   # rows without a visible key
    live = ov[:, T:].permute(0, 2, 1, 3).double()                                         # [B, Hq, 64 rows, 64 classes]
    got = (live * nvis[:, None] * (1 - P))[..., cls]                                      # ... -> [.., key t]
    assert float((got - got.round()).abs().max()) < 0.03 and torch.equal(got.round(), bits)
    # dQ
    do = torch.ones(B * S, Hq * D, dtype=torch.bfloat16, device="cuda")
    d = ops.attn_bwd(qkv, mask, o, do, lse, B, S, Hq, Hkv, D, SCALE, drop=(P, seed)).view(B, S, Hq + 2 * Hkv, D)
    dq = d[:, T:, :Hq].permute(0, 2, 1, 3).double()[..., cls]                             # [B, Hq, rows, key t]
    delta = live.sum(-1, keepdim=True)
    got = (dq / SCALE * nvis[:, None] + delta) * (1 - P) * vis
    assert float((got - got.round()).abs().max()) < 0.1 and torch.equal(got.round(), bits)
    assert bool((d[:, :T, :Hq] == 0).all()) and bool((d[:, :T, Hq:] == 0).all())          # dead rows' dq, masked keys' dk / dv
    # dK / dV
    do = torch.zeros(B, S, Hq, D, dtype=torch.bfloat16, device="cuda")
    do[:, j, :, j % 64] = 1.0
    d = ops.attn_bwd(qkv, mask, o, do.view(B * S, Hq * D), lse, B, S, Hq, Hkv, D, SCALE, drop=(P, seed)).view(B, S, Hq + 2 * Hkv, D)
    dv = d[:, T:, Hq + Hkv:].permute(0, 2, 1, 3).double()[..., cls]                       # [B, Hkv, key t, row r]
    got = dv * nvis[None, :] * (1 - P)
    want = bits.view(B, Hkv, G, 64, 64).sum(2).transpose(-1, -2)                          # both heads of the group; [.., key t, row r]
    assert float((got - got.round()).abs().max()) < 0.06 and torch.equal(got.round(), want)


# ---------------------------------------------------------------------------------------------------------------------
# forward and gradients against float64
# ---------------------------------------------------------------------------------------------------------------------
def attn_drop_ref_fp64(qkv, do, mask, Z, S, Hq, Hkv):
    """attn_ref_fp64 of tests/test_gpu_attention_fp64.py with Z ([B, Hq, S, S] float64, kept / (1 - p)) on the probabilities:
    o = (P o Z) V, dP = (dO V^T) o Z, dS = P o (dP - rowsum(dO o O)), dq = scale dS K, dk = scale dS^T Q, dv = (P o Z)^T dO; the row magnitudes
    (o_scale, a_dq, a_dk, a_dv) of that file's docstring with Z wherever a probability multiplies a value."""
    G = Hq // Hkv
    x = qkv.view(B, S, Hq + 2 * Hkv, D).double()
    dov = do.view(B, S, Hq, D).double()
    vis = _visible(mask, S)[:, 0]                                                         # [B, S, S]
    f64 = dict(dtype=torch.float64, device="cuda")
    R = {k: torch.zeros(B, S, Hq, D, **f64) for k in ("o", "dq")}
    R.update({k: torch.zeros(B, S, Hkv, D, **f64) for k in ("dk", "dv", "a_dk", "a_dv")})
    R["o_scale"], R["a_dq"] = torch.zeros(B, S, Hq, **f64), torch.zeros(B, S, Hq, **f64)
    for b in range(B):
        for hq in range(Hq):
            g = hq // G
            q, k, v, dO, z = x[b, :, hq], x[b, :, Hq + g], x[b, :, Hq + Hkv + g], dov[b, :, hq], Z[b, hq]
            s = (q @ k.T * SCALE).masked_fill(~vis[b], -math.inf)
            Pm = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)                          # rows without a visible key: zeros
            Pz = Pm * z
            o = Pz @ v
            dP = (dO @ v.T) * z
            Di = (dO * o).sum(1, keepdim=True)
            dS = Pm * (dP - Di)
            R["o"][b, :, hq], R["dq"][b, :, hq] = o, SCALE * (dS @ k)
            R["dk"][b, :, g] += SCALE * (dS.T @ q)
            R["dv"][b, :, g] += Pz.T @ dO
            M = (dO.abs() @ v.abs().T) * z
            T = Pm * (M + (Pm * M).sum(1, keepdim=True))
            R["o_scale"][b, :, hq] = (Pz @ v.abs()).norm(dim=1)
            R["a_dq"][b, :, hq] = SCALE * (T @ k.abs()).norm(dim=1)
            R["a_dk"][b, :, g] += SCALE * (T.T @ q.abs())
            R["a_dv"][b, :, g] += Pz.T @ dO.abs()
    R["a_dk"], R["a_dv"] = R["a_dk"].norm(dim=-1), R["a_dv"].norm(dim=-1)
    return R


def _whole(o, d, R, S, Hq, Hkv):
    from test_gpu_attention_fp64 import whole_rel
    x = d.view(B, S, Hq + 2 * Hkv, D)
    return {"o": whole_rel(o.view(B, S, Hq, D), R["o"], R["o_scale"]), "dq": whole_rel(x[:, :, :Hq], R["dq"], R["a_dq"]),
            "dk": whole_rel(x[:, :, Hq:Hq + Hkv], R["dk"], R["a_dk"]), "dv": whole_rel(x[:, :, Hq + Hkv:], R["dv"], R["a_dv"])}


def _seed_with_an_all_dropped_row(S, Hq, mask):
    """The first seed whose mask drops EVERY visible key of some row that has one (numpy alone decides; with p 0.25 the rows with a single
    visible key do it one time in four)."""
    vis = _visible(mask, S)
    for seed in range(500, 600):
        lost = ((_keep(P, seed, Hq, S) & vis).sum(-1) == 0) & (vis.sum(-1) > 0)
        if bool(lost.any()):
            return seed, lost
    raise AssertionError("no seed with an all-dropped row")


@pytest.mark.parametrize("family", ["gauss", "peaked", "flat"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("S", LENGTHS)
def test_forward_and_gradients_against_float64(ops, S, Hq, Hkv, family):
    from test_gpu_attention_fp64 import LEAN_VS_ROUND2, attn_ref_fp64, make_inputs
    qkv, do = make_inputs(family, B, S, Hq, Hkv, D, seed=100 + S + Hq)
    mask = _mask(S)
    seed, lost = _seed_with_an_all_dropped_row(S, Hq, mask)
    # e0: the register-staged kernels without dropout against the plain float64 reference
    try:
        ops.set_attn_fwd_staging(0)
        o0, lse0 = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, SCALE)
        d0 = ops.attn_bwd(qkv, mask, o0, do, lse0, B, S, Hq, Hkv, D, SCALE)
    finally:
        ops.set_attn_fwd_staging(2)
    e0 = _whole(o0, d0, attn_ref_fp64(qkv, do, mask, B, S, Hq, Hkv, D, SCALE), S, Hq, Hkv)
    # e_drop
    keep = _keep(P, seed, Hq, S)
    R = attn_drop_ref_fp64(qkv, do, mask, keep.double() / (1 - P), S, Hq, Hkv)
    o, lse = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, SCALE, drop=(P, seed))
    d = ops.attn_bwd(qkv, mask, o, do, lse, B, S, Hq, Hkv, D, SCALE, drop=(P, seed))
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(d.float()).all())
    assert torch.equal(lse, lse0), "lse is that of the undropped probabilities"
    e = _whole(o, d, R, S, Hq, Hkv)
    a, c = 2.0 / (1.0 - P), LEAN_VS_ROUND2[1]
    print(f"\nS {S} heads {Hq}/{Hkv} {family}: " + "  ".join(f"{n} {e[n]:.3e} / e0 {e0[n]:.3e} = {e[n] / max(e0[n], 1e-300):.2f}" for n in e))
    # rows without a visible key: o = 0 and dq = 0; masked keys: dk = dv = 0; a row whose visible keys are all dropped: o = 0
    ov, x = o.view(B, S, Hq, D), d.view(B, S, Hq + 2 * Hkv, D)
    dead = _visible(mask, S)[:, 0].sum(-1) == 0                                           # [B, S]
    if S == 64:
        assert bool(dead[1].all())
    assert bool((ov[dead] == 0).all()) and bool((x[:, :, :Hq][dead] == 0).all())
    assert bool((x[:, :, Hq:][mask == 0] == 0).all())
    assert bool(lost.any()) and bool((ov.permute(0, 2, 1, 3)[lost] == 0).all())
    for n in ("o", "dq", "dk", "dv"):
        assert e[n] <= a * e0[n] + c, (n, e[n], e0[n], e[n] / max(e0[n], 1e-300))


# ---------------------------------------------------------------------------------------------------------------------
# determinism, p = 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", LENGTHS)
def test_same_bits_twice_and_p_zero_is_the_plain_call(ops, S):
    from test_gpu_attention_fp64 import make_inputs
    Hq, Hkv, seed = 4, 2, 31
    qkv, do = make_inputs("gauss", B, S, Hq, Hkv, D, seed=7)
    mask = _mask(S)
    runs = []
    for _ in range(2):
        o, lse = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, SCALE, drop=(P, seed))
        runs.append((o, lse, ops.attn_bwd(qkv, mask, o, do, lse, B, S, Hq, Hkv, D, SCALE, drop=(P, seed))))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    o2, _ = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, SCALE, drop=(P, seed + 1))
    assert not torch.equal(o2, runs[0][0])                                                # another seed, another mask
    for mode in (2, 0):                                                                   # the default kernels and the register-staged ones
        try:
            ops.set_attn_fwd_staging(mode)
            o, lse = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, SCALE)
            dq = ops.attn_bwd(qkv, mask, o, do, lse, B, S, Hq, Hkv, D, SCALE)
            oz, lsez = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, SCALE, drop=(0.0, seed))
            dz = ops.attn_bwd(qkv, mask, oz, do, lsez, B, S, Hq, Hkv, D, SCALE, drop=(0.0, seed))
        finally:
            ops.set_attn_fwd_staging(2)
        assert torch.equal(o, oz) and torch.equal(lse, lsez) and torch.equal(dq, dz), mode


# ---------------------------------------------------------------------------------------------------------------------
# the GPT-2 block
# ---------------------------------------------------------------------------------------------------------------------
def _tensors(obj):
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, (tuple, list)):
        for t in obj:
            yield from _tensors(t)


def _oracle_loss_and_grads(z, b, keeps, p):
    """The torch restatement of tests/test_gpu_gpt2.py's attention-dropout test: the fp32 block with autograd, the given keep masks per layer."""
    import torch.nn.functional as F
    from oracle import gpt2_ref as G
    params = {k[2:]: torch.from_numpy(z[k]).cuda().requires_grad_(True) for k in z.files if k.startswith("w:")}
    ids, mask, pos = b["input_ids"], b["attention_mask"], b["position_ids"]
    H, nh, Bn, S = 128, 2, 3, 64
    x = params["transformer.wte.weight"][ids] + params["transformer.wpe.weight"][pos]
    vis = torch.tril(torch.ones(S, S, dtype=torch.bool, device="cuda"))[None, None] & (mask[:, None, None, :] != 0)
    for i in range(2):
        pre = f"transformer.h.{i}."
        h = F.layer_norm(x, (H,), params[pre + "ln_1.weight"], params[pre + "ln_1.bias"], 1e-5)
        q, k, v = (h @ params[pre + "attn.c_attn.weight"] + params[pre + "attn.c_attn.bias"]).split(H, dim=2)
        q, k, v = (t.view(Bn, S, nh, D).transpose(1, 2) for t in (q, k, v))
        sc = (q @ k.transpose(-1, -2)) / 8.0
        pr = torch.nan_to_num(torch.softmax(sc.masked_fill(~vis, float("-inf")), -1), nan=0.0)
        pr = pr * keeps[i].float() / (1 - p)
        a = (pr @ v).transpose(1, 2).reshape(Bn, S, H)
        x = x + a @ params[pre + "attn.c_proj.weight"] + params[pre + "attn.c_proj.bias"]
        h = F.layer_norm(x, (H,), params[pre + "ln_2.weight"], params[pre + "ln_2.bias"], 1e-5)
        x = x + G.gelu_new(h @ params[pre + "mlp.c_fc.weight"] + params[pre + "mlp.c_fc.bias"]) @ params[pre + "mlp.c_proj.weight"] + params[pre + "mlp.c_proj.bias"]
    x = F.layer_norm(x, (H,), params["transformer.ln_f.weight"], params["transformer.ln_f.bias"], 1e-5)
    logits = x @ params["transformer.wte.weight"].T
    ref = F.cross_entropy(logits[:, :-1].reshape(-1, 300), b["labels"][:, 1:].reshape(-1), ignore_index=-100)
    ref.backward()
    return ref, {n: t.grad for n, t in params.items()}


def test_gpt2_fused_attention_dropout_against_the_fp32_oracle():
    """The tiny GPT-2 golden (2 layers, 2 heads of 64, B 3, S 64) with attn_pdrop 0.2 and fused_attention_dropout: (p, seed) per layer from
    m._saved, the masks from numpy, the fp32 torch restatement with those masks; loss within 1e-2 relative, every gradient within 4e-2.
    While the state is live: the attention slot holds (lse [B, n_head, S], (p, seed)), and the layer saves nothing of S x S size -- no saved
    tensor has B n_head S S or more elements except the row activations [B S, width] every form of the step keeps (qkv, the MLP's: at this
    tiny S their widths, 384 and 512, exceed n_head S = 128), and none ends in two dims of S."""
    from test_gpu_gpt2 import _batch, _grads_hf, _load
    z, m = _load()
    m.cfg.attn_pdrop = 0.2
    m.fused_attention_dropout = True
    m.train()
    b = _batch(z)
    out = m(**b)
    Bn, nh, S = 3, 2, 64
    keeps, seeds = [], []
    for layer in m._saved[0]:
        lse, (p, seed) = layer[5]
        assert torch.is_tensor(lse) and lse.shape == (Bn, nh, S) and lse.dtype == torch.float32
        assert p == 0.2
        seeds.append(seed)
        for t in _tensors(layer):
            assert t.numel() < Bn * nh * S * S or (t.dim() == 2 and t.shape[0] == Bn * S), tuple(t.shape)
            assert not (t.dim() >= 2 and t.shape[-1] == S and t.shape[-2] == S), tuple(t.shape)
        k = torch.from_numpy(attn_keep(p, seed, Bn, nh, S)).cuda()
        assert abs(1 - k.float().mean().item() - 0.2) < 0.03
        keeps.append(k)
    assert seeds[0] != seeds[1]
    out.loss.backward()
    ref, want = _oracle_loss_and_grads(z, b, keeps, 0.2)
    assert abs(out.loss.item() - ref.item()) <= 1e-2 * ref.item(), (out.loss.item(), ref.item())
    for name, g in _grads_hf(m).items():
        rel = ((g - want[name]).norm() / want[name].norm().clamp_min(1e-12)).item()
        assert rel < 4e-2, (name, rel)


def test_gpt2_fused_attention_dropout_against_the_materialised_path():
    """Two models from one seed on one batch, the flag on and off: the same seeds, hence the same masks; loss within 1e-2 relative and every
    gradient within 4e-2 of each other.  Two runs with the flag on: the same bits -- loss, gradients, weights after one optimizer step."""
    from test_gpu_gpt2 import _batch, _grads_hf, _load

    def step(fused):
        z, m = _load()
        m.cfg.attn_pdrop = 0.2
        m.fused_attention_dropout = fused
        m.train()
        opt = m.make_optimizer()
        out = m(**_batch(z))
        slots = [layer[5] for layer in m._saved[0]]
        out.loss.backward()
        grads = {n: g.clone() for n, g in _grads_hf(m).items()}
        opt.step_and_update_lr()
        return out.loss.detach().clone(), grads, {n: p.data.clone() for n, p in m.named_parameters()}, slots

    l1, g1, w1, s1 = step(True)
    l0, g0, _, s0 = step(False)
    assert [s[1] for s in s1] == [s[1] for s in s0]                                       # (p, seed) per layer
    assert all(torch.is_tensor(s[0]) for s in s1) and all(isinstance(s[0], tuple) for s in s0)
    assert abs(l1.item() - l0.item()) <= 1e-2 * abs(l0.item()), (l1.item(), l0.item())
    for name in g0:
        rel = ((g1[name] - g0[name]).norm() / g0[name].norm().clamp_min(1e-12)).item()
        assert rel < 4e-2, (name, rel)
    l2, g2, w2, _ = step(True)
    assert torch.equal(l1, l2)
    for name in g1:
        assert torch.equal(g1[name], g2[name]), name
    for name in w1:
        assert torch.equal(w1[name], w2[name]), name
