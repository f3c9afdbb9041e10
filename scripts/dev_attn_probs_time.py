"""Dev-only: ecgb_attn_probs (output_attentions) at the interpret shape (1 x 2050, 32 / 8 heads of 64), the Gemma-2B head layout (1 x 2048, 8 / 1 heads of 256)
and the C3 shape (32 x 1024, sum form only), HIP events, interleaved rounds; then the eval forward of a Llama-3.2-1B-dims model (two layers) at the interpret
shape with output_attentions False against "mean".
Usage: dev_attn_probs_time.py [rounds]"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ecg_byte_amd import decoder_ops as ops


def timed(fn, reps=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SHAPES = [((1, 2050, 32, 8, 64), ("full", "sum")), ((1, 2048, 8, 1, 256), ("full", "sum")), ((32, 1024, 32, 8, 64), ("sum",))]
torch.manual_seed(0)
cases = []
for (B, S, Hq, Hkv, D), forms in SHAPES:
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device="cuda").to(torch.bfloat16)
    mask = torch.ones(B, S, device="cuda")
    mask[0, :70] = 0                                                   # a left pad
    scale = 1 / math.sqrt(D)
    _, lse = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, scale)
    for form in forms:
        probs = torch.empty((B, Hq, S, S), dtype=torch.bfloat16, device="cuda") if form == "full" else None
        psum = torch.empty((B, S, S), dtype=torch.float32, device="cuda") if form == "sum" else None
        fn = (lambda qkv=qkv, mask=mask, lse=lse, B=B, S=S, Hq=Hq, Hkv=Hkv, D=D, scale=scale, probs=probs, psum=psum:
              ops.attn_probs(qkv, mask, lse, B, S, Hq, Hkv, D, scale, probs=probs, psum=psum, weight=0.5, accumulate=True))
        written = B * Hq * S * S * 2 if form == "full" else B * S * S * 4
        flops = 2 * B * Hq * D * S * S / 2                            # q.k over the causal half
        cases.append(((B, S, Hq, Hkv, D), form, fn, written, flops, []))
for _ in range(rounds):
    for c in cases:
        c[5].append(timed(c[2]))
for shape, form, _, written, flops, ts in cases:
    t = min(ts) * 1e-3
    print(f"B,S,Hq,Hkv,D={shape} {form:4s}: {t * 1e6:8.1f} us (median {sorted(ts)[len(ts) // 2] * 1e3:.1f})   wrote {written / 1e6:7.1f} MB  "
          f"{written / t / 1e12:5.2f} TB/s   {flops / t / 1e12:6.1f} TFLOP/s", flush=True)

# eval forward at the interpret shape, output_attentions False vs "mean"
from ecg_byte_amd.decoder import DecoderConfig, HipCausalLM
cfg = DecoderConfig(vocab_size=1024, hidden_size=2048, intermediate_size=8192, num_hidden_layers=2, num_attention_heads=32, num_key_value_heads=8,
                    rms_norm_eps=1e-5, rope_theta=500000.0, rope_scaling=None, pad_token_id=1023)
m = HipCausalLM(cfg).eval()
S = 2050
ids = torch.randint(0, 1023, (1, S), device="cuda")
mask = torch.ones(1, S, device="cuda")
mask[0, :70] = 0
labels = ids.clone()
res = {False: [], "mean": []}
with torch.no_grad():
    for _ in range(rounds):
        for oa in res:
            res[oa].append(timed(lambda oa=oa: m(input_ids=ids, attention_mask=mask, labels=labels, output_attentions=oa), reps=10))
f, a = min(res[False]), min(res["mean"])
print(f"eval forward (2 layers, Llama-3.2-1B dims, 1 x {S}): output_attentions False {f:.3f} ms, 'mean' {a:.3f} ms (+{100 * (a - f) / f:.1f} %)", flush=True)
