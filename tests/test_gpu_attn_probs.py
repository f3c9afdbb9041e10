"""GPU tests of output_attentions: ecgb_attn_probs (ops.attn_probs) against an fp64 softmax of the same bf16 q and k, its two
output forms against each other, HipCausalLM's attentions against the vendored transformers' eager attentions
(tests/golden/make_decoder_golden_attn.py), the unchanged loss / logits, the interpret shape, and the interp_analysis CLI."""
import json
import math
import os
import pickle

import numpy as np
import pytest

from helpers import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _qkv(B, S, Hq, Hkv, D, seed, std=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = (torch.randn(B * S, (Hq + 2 * Hkv) * D, generator=g) * std).to(torch.bfloat16).cuda()
    mask = torch.ones(B, S)
    if B > 1:
        mask[1, : (S // 3 + 1) if S > 1 else 0] = 0          # ragged left pad
    if B > 2:
        mask[2] = 0                                          # fully padded row
    return qkv, mask.cuda()


def _lse(qkv, mask, B, S, Hq, Hkv, D, scale):
    from ecg_byte_amd import decoder_ops as ops
    # the round-2 forward (scores times scale * log2 e in fp32) at head_dim 64: the lean kernel rounds its pre-scaled q operand to bf16,
    # an error of the lse (half an ulp of q) that is not the probability kernel's to measure
    if D == 64:
        ops.set_attn_fwd_staging(1)
    try:
        _, lse = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, scale)
    finally:
        ops.set_attn_fwd_staging(2)
    return lse


def _ref_probs(qkv, mask, b, S, Hq, Hkv, D, scale):
    """fp64 softmax of batch row b: [Hq, S, S]; rows with no visible key = 1/S."""
    x = qkv.view(-1, S, (Hq + 2 * Hkv) * D)[b].double()
    q = x[:, : Hq * D].view(S, Hq, D).transpose(0, 1)
    k = x[:, Hq * D: (Hq + Hkv) * D].view(S, Hkv, D).transpose(0, 1).repeat_interleave(Hq // Hkv, 0)
    s = torch.matmul(q, k.transpose(1, 2)) * scale
    vis = torch.tril(torch.ones(S, S, dtype=torch.bool, device=qkv.device)) & (mask[b] != 0)[None, :]
    s = s.masked_fill(~vis, -math.inf)
    empty = ~vis.any(1)
    p = torch.softmax(s.masked_fill(empty[:, None], 0.0), -1)
    p[:, empty] = 1.0 / S
    return p, vis, empty


SHAPES = [  # (D, Hq, Hkv, S)
    (64, 2, 2, 1), (64, 4, 1, 33), (64, 2, 2, 130), (64, 32, 8, 1024), (64, 4, 1, 2050),
    (128, 2, 2, 64), (128, 4, 1, 130), (128, 8, 1, 33),
    (256, 2, 2, 1), (256, 4, 1, 130), (256, 8, 1, 2048),
]


@pytest.mark.parametrize("D,Hq,Hkv,S", SHAPES, ids=[f"d{d}-{a}x{b}-s{s}" for d, a, b, s in SHAPES])
def test_probs_vs_fp64_softmax(D, Hq, Hkv, S):
    from ecg_byte_amd import decoder_ops as ops
    B, scale, w = 3, 1.0 / math.sqrt(D), 0.37
    qkv, mask = _qkv(B, S, Hq, Hkv, D, seed=D + S + Hq)
    lse = _lse(qkv, mask, B, S, Hq, Hkv, D, scale)
    probs = torch.empty((B, Hq, S, S), dtype=torch.bfloat16, device="cuda")
    psum = torch.empty((B, S, S), dtype=torch.float32, device="cuda")
    ops.attn_probs(qkv, mask, lse, B, S, Hq, Hkv, D, scale, probs=probs, psum=psum, weight=w)
    torch.cuda.synchronize()
    inv = torch.tensor(1.0 / S, dtype=torch.bfloat16).item()
    for b in range(B):
        ref, vis, empty = _ref_probs(qkv, mask, b, S, Hq, Hkv, D, scale)
        got = probs[b].double()
        full = vis[None].expand_as(ref) & ~empty[None, :, None]
        r = ref[full]
        ulp = torch.exp2(torch.floor(torch.log2(r.clamp_min(2.0 ** -126))) - 7).clamp_min(2.0 ** -126)
        err = (got[full] - r).abs()
        assert bool((err <= ulp).all()), f"b{b}: worst {float((err / ulp).max()):.3f} ulp"
        hidden = ~vis[None].expand_as(ref) & ~empty[None, :, None]
        assert bool((got[hidden] == 0).all()), f"b{b}: a key that is not visible has nonzero probability"
        if bool(empty.any()):
            assert bool((got[:, empty, :] == inv).all()), f"b{b}: rows with no visible key are not bf16(1/S)"
        want = w * ref.sum(0)
        assert bool(((psum[b].double() - want).abs() <= 2e-4 * want.abs() + 1e-7).all()), f"b{b}: sum form"


def test_two_forms_deterministic_and_composable():
    from ecg_byte_amd import decoder_ops as ops
    B, S, Hq, Hkv, D = 3, 130, 4, 1, 128
    scale = 1.0 / math.sqrt(D)
    qkv, mask = _qkv(B, S, Hq, Hkv, D, seed=7)
    _, lse = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, scale)

    def run(probs=True, psum=True, weight=1.0, out=None, accumulate=False):
        p = torch.full((B, Hq, S, S), 7.0, dtype=torch.bfloat16, device="cuda") if probs else None
        s = out if out is not None else (torch.full((B, S, S), 5.0, device="cuda") if psum else None)
        ops.attn_probs(qkv, mask, lse, B, S, Hq, Hkv, D, scale, probs=p, psum=s, weight=weight, accumulate=accumulate)
        return p, s

    p1, s1 = run()
    p2, s2 = run()
    pa, _ = run(psum=False)
    _, sa = run(probs=False)
    assert torch.equal(p1, p2) and torch.equal(s1, s2), "two launches differ"
    assert torch.equal(p1, pa) and torch.equal(s1, sa), "a form launched alone differs from the same form launched with the other"
    w1, w2 = 0.25, 0.625
    outs = []
    for _ in range(2):
        acc = torch.full((B, S, S), 3.0, device="cuda")
        run(probs=False, weight=w1, out=acc)
        run(probs=False, weight=w2, out=acc, accumulate=True)
        outs.append(acc)
    assert torch.equal(outs[0], outs[1])
    want = (w1 + w2) * s1.double()
    assert bool(((outs[0].double() - want).abs() <= 4 * 2.0 ** -24 * want.abs() + 1e-30).all())


def test_bad_arguments_are_status_codes():
    from ecg_byte_amd import _lib
    from ecg_byte_amd import decoder_ops as ops
    B, S, Hq, Hkv, D = 1, 64, 2, 1, 64
    qkv, mask = _qkv(B, S, Hq, Hkv, D, seed=1)
    _, lse = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, 0.125)
    L, QKV = _lib.lib(), qkv.shape[1]
    p = torch.empty((B, Hq, S, S), dtype=torch.bfloat16, device="cuda")
    args = lambda **kw: dict(dict(q=ops._off(qkv, 0), ldq=QKV, k=ops._off(qkv, Hq * D), ldk=QKV, mask=ops._p(mask), lse=ops._p(lse), p=ops._p(p), ps=None,
                                  w=1.0, acc=0, B=B, S=S, Hq=Hq, Hkv=Hkv, D=D, sc=0.125, st=ops._st()), **kw)
    call = lambda a: L.ecgb_attn_probs(*a.values())
    assert call(args()) == 0
    assert call(args(p=None)) == -1                      # neither output
    assert call(args(lse=None)) == -1
    assert call(args(Hkv=3)) == -1                       # Hq % Hkv
    assert call(args(S=0)) == -1
    assert call(args(D=96)) == -3
    assert call(args(ldq=QKV - 4)) == -3
    torch.cuda.synchronize()


# ---- the model against the vendored transformers ------------------------------------------------------------------------------------------
def _tiny(name):
    from ecg_byte_amd.decoder import DecoderConfig, HipCausalLM
    z = np.load(os.path.join(GOLDEN, f"decoder_{name}_tiny.npz"))
    if name == "llama":
        cfg = DecoderConfig(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                            num_key_value_heads=1, rms_norm_eps=1e-5, rope_theta=500000.0, pad_token_id=299,
                            rope_scaling={"factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                          "original_max_position_embeddings": 32, "rope_type": "llama3"})
    else:
        cfg = DecoderConfig(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                            num_key_value_heads=1, head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0, rope_scaling=None, pad_token_id=299,
                            model_type="gemma")
    m = HipCausalLM(cfg)
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")})
    m.eval()
    batch = dict(input_ids=torch.from_numpy(z["input_ids"]).cuda(), attention_mask=torch.from_numpy(z["attention_mask"]).cuda(),
                 position_ids=torch.from_numpy(z["position_ids"]).cuda())
    return m, batch, torch.from_numpy(z["labels"]).cuda()


@pytest.mark.parametrize("name", ["llama", "gemma"])
def test_model_attentions_vs_vendored_transformers(name):
    g = np.load(os.path.join(GOLDEN, "decoder_attn_tiny.npz"))
    m, batch, _ = _tiny(name)
    L = m.cfg.num_hidden_layers
    with torch.no_grad():
        full = m(**batch, output_attentions=True).attentions
        mean = m(**batch, output_attentions="mean").attentions
    assert isinstance(full, tuple) and len(full) == L
    ref = [torch.from_numpy(g[f"{name}/fp32/{i}"]).cuda() for i in range(L)]
    for i in range(L):
        assert full[i].dtype == torch.bfloat16 and full[i].shape == ref[i].shape
        err = (full[i].float() - ref[i]).abs().max().item()
        assert err <= 2 * float(g[f"{name}/bf16_err/{i}"]) + 2 ** -9, (i, err)
    assert isinstance(mean, tuple) and len(mean) == 1 and mean[0].dtype == torch.float32 and mean[0].shape == (ref[0].shape[0], 1) + ref[0].shape[2:]
    err = (mean[0][:, 0] - torch.stack(ref).mean(dim=(0, 2))).abs().max().item()
    assert err <= 2 * float(g[f"{name}/bf16_err/mean"]) + 2 ** -9, err
    # the reference interpreter's reduction returns the map unchanged from the 1-tuple
    assert torch.equal(torch.stack(mean).mean(dim=(0, 2))[0], mean[0][0, 0])


def test_loss_and_logits_unchanged_and_grad_path():
    m, batch, labels = _tiny("llama")
    with torch.no_grad():
        losses = [m(**batch, labels=labels, output_attentions=oa) for oa in (False, True, "mean")]
        logits = [m(**batch, output_attentions=oa) for oa in (False, True, "mean")]
    assert losses[0].attentions is None and logits[0].attentions is None
    assert all(torch.equal(o.loss, losses[0].loss) for o in losses) and losses[1].attentions is not None
    assert all(torch.equal(o.logits, logits[0].logits) for o in logits) and logits[2].attentions is not None
    m.train()
    out = m(**batch, labels=labels, output_attentions=True)
    assert out.attentions is None
    out.loss.backward()


def test_head_dim_outside_fused_set_raises_only_when_asked():
    from ecg_byte_amd.decoder import DecoderConfig, HipCausalLM
    cfg = DecoderConfig(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                        num_key_value_heads=1, head_dim=192, rms_norm_eps=1e-5, rope_theta=10000.0, rope_scaling=None, pad_token_id=299)
    m = HipCausalLM(cfg).eval()
    assert not m.fused_attention
    ids = torch.randint(0, 299, (2, 64), device="cuda")
    with torch.no_grad():
        assert m(input_ids=ids).attentions is None
        for oa in (True, "mean"):
            with pytest.raises(NotImplementedError):
                m(input_ids=ids, output_attentions=oa)


def test_interpret_shape_llama_1b_dims():
    """Llama-3.2-1B attention dims (32 / 8 heads, head_dim 64), two random layers, batch 1 at the interpret shape S = 2050 with a left pad."""
    from ecg_byte_amd.decoder import DecoderConfig, HipCausalLM
    cfg = DecoderConfig(vocab_size=1024, hidden_size=2048, intermediate_size=8192, num_hidden_layers=2, num_attention_heads=32,
                        num_key_value_heads=8, rms_norm_eps=1e-5, rope_theta=500000.0, rope_scaling=None, pad_token_id=1023)
    m = HipCausalLM(cfg).eval()
    S, pad = 2050, 70
    ids = torch.randint(0, 1023, (1, S), device="cuda")
    mask = torch.ones(1, S, device="cuda")
    mask[0, :pad] = 0
    ids[0, :pad] = 1023
    pos = (torch.cumsum(mask, 1) - 1).clamp(min=0).long()
    with torch.no_grad():
        mean = m(input_ids=ids, attention_mask=mask, position_ids=pos, output_attentions="mean").attentions[0][0, 0]
        full = m(input_ids=ids, attention_mask=mask, position_ids=pos, output_attentions=True).attentions
        want = torch.stack(full).float().mean((0, 2))[0]
    rows = mean[pad:].double().sum(-1)
    # 5e-4, not 1e-4: at head_dim 64 the lean forward forms its lse from q * scale * log2 e rounded to bf16 (half an ulp of q), the probabilities here
    # from the exact bf16 q -- rows with few visible keys sum to 1 within ~2e-4 (measured 1.8e-4 at this shape)
    assert float((rows - 1).abs().max()) <= 5e-4
    assert bool(((mean - want).abs() <= 2.0 ** -8 * want.abs() + 1e-7).all())
    assert bool((mean[:pad] == mean[0, 0]).all()) and abs(float(mean[0, 0]) - 1.0 / S) < 1e-7


# ---- the interp_analysis CLI ------------------------------------------------------------------------------------------------------------
REPORTS = ["sinus rhythm normal ecg", "atrial fibrillation with rapid ventricular response", "left bundle branch block"]
QUESTION = "Could you please help me explain my ECG ?"


def test_interp_analysis_end_to_end(tmp_path):
    pytest.importorskip("transformers")
    from helpers import load_tokenizer
    from test_gpu_pipeline import _write_model_dir
    from ecg_byte_amd import file_utils as F
    from ecg_byte_amd import interp_analysis as IA
    from ecg_byte_amd import main as M
    from ecg_byte_amd import synth
    vocab, merges, pc = load_tokenizer("c1")
    data = tmp_path / "data"
    x = synth.synth_ecg(3, 100, seed=9)
    for sub in ("ecg", "text"):
        os.makedirs(data / "ptb_500" / sub / "test")
    for i in range(3):
        np.save(data / "ptb_500" / "ecg" / "test" / f"ecg_{i}_0.npy", x[i])
        (data / "ptb_500" / "text" / "test" / f"text_{i}_0.json").write_text(json.dumps(REPORTS[i]))
    F.save_percentiles(tmp_path / "percentiles.npy", pc["percentile_1"], pc["percentile_99"])
    with open(data / "tokenizer_c1.pkl", "wb") as f:
        pickle.dump((vocab, merges), f)
    model_dir = str(tmp_path / "tiny-llama")
    _write_model_dir(model_dir, QUESTION.split() + " ".join(REPORTS).split())
    argv = ["--device", "cuda:0", "--model", model_dir, "--dataset", "ptb_500", "--tokenizer_check", "tokenizer_c1", "--batch_size=1",
            "--percentiles", str(tmp_path / "percentiles.npy"), "--pad_to_max", "1024", "--num_merges", "1000", "--bins=100", "--peft",
            "--interpret", "--data_root", str(data), "--runs_root", str(tmp_path / "runs"), "--checkpoint", "ck", "--workers", "1"]
    args = IA.get_args(argv)
    model, _ = M.build_model_and_tokenizer(args, vocab, torch.device("cuda:0"))
    os.makedirs(tmp_path / "runs" / "0" / "ck")
    torch.save({"model": model.state_dict(), "epoch": 0}, tmp_path / "runs" / "0" / "ck" / "best_model.pth")
    out = IA.main(argv)
    path = tmp_path / "runs" / "0" / "ck" / "interpret_ptb_500.npz"
    assert path.exists()
    z = np.load(path)
    n = len(out["signal"]["attentions"])
    assert n >= 1
    for comp in ("signal", "question", "answer"):
        for k in range(n):
            seq, att = z[f"{comp}/sequences/{k}"], z[f"{comp}/attentions/{k}"]
            assert att.shape == seq.shape and np.isfinite(att).all() and (att >= 0).all(), (comp, k)
    assert len(z["signal/signal/0"].item()) == 12 * 100
