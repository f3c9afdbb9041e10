"""Dev-only: one GPT-2-small layer's attention with dropout on the probabilities, forward + backward, at C1's shape (B 4 x S 1024 x 12 heads of 64,
p 0.1; SHAPE=B,S,H and P_DROP= for another): the materialised-scores path (HipCausalLM._attn_materialised: head-batched GEMMs, softmax kernel, ops.dropout,
seven S x S passes in the backward) against the fused kernels with the dropout inside (ops.attn_fwd / attn_bwd with drop=(p, seed)), in one process, HIP events,
interleaved rounds; beside them the p = 0 kernels of the same family (register-staged, ecgb_set_attn_fwd_staging 0) and the default lean kernels.
Then the peak memory of a two-layer GPT-2-small training step (forward + backward) both ways.  Both paths draw the same masks: their outputs are compared.
Usage: dev_attn_dropout_ab.py [rounds [reps]]"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ecg_byte_amd import decoder_ops as ops
from ecg_byte_amd.gpt2 import GPT2Config, HipGPT2LM

B, S, H = [int(v) for v in os.environ.get("SHAPE", "4,1024,12").split(",")]
D, p, seed = 64, float(os.environ.get("P_DROP", "0.1")), 12345
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
scale = 1 / math.sqrt(D)


def timed(fn):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


torch.manual_seed(0)
m = HipGPT2LM(GPT2Config(vocab_size=512, n_positions=S, n_embd=H * D, n_layer=1, n_head=H))      # the owner of _attn_materialised (cfg, qkv width)
qkv = torch.randn(B * S, 3 * H * D, device="cuda").to(torch.bfloat16)
do = torch.randn(B * S, H * D, device="cuda").to(torch.bfloat16)
mask = torch.ones(B, S, device="cuda")
for b in range(B): mask[b, : (37 * b) % (S // 2)] = 0
drop = (p, seed)


def staged(mode, fn):
    def run():
        ops.set_attn_fwd_staging(mode)
        try: return fn()
        finally: ops.set_attn_fwd_staging(2)
    return run


def fused_pair(dr):
    o, l = ops.attn_fwd(qkv, mask, B, S, H, H, D, scale, drop=dr)
    return (lambda: ops.attn_fwd(qkv, mask, B, S, H, H, D, scale, drop=dr)), (lambda: ops.attn_bwd(qkv, mask, o, do, l, B, S, H, H, D, scale, drop=dr)), o


ao_m, PP = m._attn_materialised(qkv, mask, B, S, drop=drop)
fwd_f, bwd_f, o_f = fused_pair(drop)
ops.set_attn_fwd_staging(0)
fwd_0, bwd_0, _ = fused_pair(None)                               # o / lse of the register-staged p = 0 forward
ops.set_attn_fwd_staging(2)
fwd_l, bwd_l, _ = fused_pair(None)
variants = {
    "materialised, p %.2f" % p: (lambda: m._attn_materialised(qkv, mask, B, S, drop=drop), lambda: m._attn_materialised_bwd(qkv, do, PP, B, S, drop=drop)),
    "fused dropout, p %.2f" % p: (fwd_f, bwd_f),
    "register-staged, p 0": (staged(0, fwd_0), staged(0, bwd_0)),
    "lean (default), p 0": (fwd_l, bwd_l),
}
# the same masks: the two paths' outputs agree to the bf16 roundings of the materialised P
d_m, d_f = m._attn_materialised_bwd(qkv, do, PP, B, S, drop=drop), bwd_f()
rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()
print(f"B {B} S {S} heads {H} x {D}, p {p}: fused against materialised  o {rel(o_f, ao_m):.2e}  d_qkv {rel(d_f, d_m):.2e}", flush=True)
del d_m, d_f
res = {k: ([], []) for k in variants}
for _ in range(rounds):
    for k, (f, b) in variants.items():
        res[k][0].append(timed(f)); res[k][1].append(timed(b))
print(f"{'':28s} {'fwd ms':>8s} {'bwd ms':>8s} {'fwd+bwd':>8s}   (min of {rounds} rounds x {reps} calls; medians in brackets)")
for k, (fs, bs) in res.items():
    f, b = min(fs), min(bs)
    print(f"{k:28s} {f:8.3f} {b:8.3f} {f + b:8.3f}   [{sorted(fs)[rounds // 2]:.3f} {sorted(bs)[rounds // 2]:.3f}]", flush=True)
del m, PP, ao_m, o_f


def step_peak(fused):
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    cfg = GPT2Config(vocab_size=4099, n_positions=S, n_embd=H * D, n_layer=2, n_head=H, attn_pdrop=p)
    mm = HipGPT2LM(cfg, seed=5)
    mm.fused_attention_dropout = fused
    mm.train()
    g = torch.Generator(device="cuda").manual_seed(3)
    ids = torch.randint(0, 4098, (B, S), device="cuda", generator=g)
    labels = torch.full((B, S), -100, device="cuda"); labels[:, -50:] = ids[:, -50:]
    pos = (torch.cumsum(mask, 1) - 1).clamp(min=0).long()
    for _ in range(2):                                            # the second step: buffers of the first are warm
        torch.cuda.synchronize(); base = torch.cuda.memory_allocated(); torch.cuda.reset_peak_memory_stats()
        out = mm(input_ids=ids, attention_mask=mask, labels=labels, position_ids=pos)
        out.loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
    return out.loss.item(), base / 2 ** 20, peak / 2 ** 20


for fused in (False, True):
    loss, base, peak = step_peak(fused)
    print(f"two-layer step, {'fused dropout' if fused else 'materialised '}: loss {loss:.4f}  allocated before {base:.0f} MiB  peak {peak:.0f} MiB  (step's own {peak - base:.0f} MiB)", flush=True)
