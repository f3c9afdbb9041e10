"""Dev: a batched decode step at Llama-3.2-1B dims (LoRA r16 unmerged, 1024-token prompts, graph replay) with the 9..64-row kernels (HipCausalLM.decode_rows) on and
off, timed with device events in ONE process, the arms alternated and the off arm run twice (its spread is the yardstick for a difference):
    python scripts/dev_generate_batch_time.py [sites|steps|all] [B ...]
sites: the six projections of a step at M = 32 (and 9, 64), ops.gemm_nt_rows / gemm_nt_rows_glu against ops.gemm_nt / gemm_nt + glu_fwd: us a launch, weight bytes per us.
steps: ms per decode step = (generate(128 new) - generate(32 new)) / 96 -- both calls replay the same captured step and share the prefill -- tokens/s = B / step, and the
step's weight bytes (every projection, the adapters, the tied head once) over its time as a share of 8 TB/s."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from ecg_byte_amd import decoder_ops as ops
from ecg_byte_amd.decoder import DecoderConfig, HipCausalLM

what = sys.argv[1] if len(sys.argv) > 1 else "all"
Bs = [int(a) for a in sys.argv[2:]] or [1, 8, 9, 16, 32, 64]
V = 128256 + 256 + 3500 + 3


def timed(fn, reps=20, windows=3):
    for _ in range(3):
        fn()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)           # us
    return out


def bf(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).to(torch.bfloat16)


if what in ("sites", "all"):
    sites = [("q|k|v", 3072, 2048, False), ("o", 2048, 2048, False), ("gate|up + GLU", 2 * 8192, 2048, True), ("down", 2048, 8192, False),
             ("adapter t", 64, 2048, False), ("adapter t (down)", 64, 8192, False), ("tied head", 132096, 2048, False)]
    for M in (32, 9, 64):
        for name, N, K, glu in sites:
            a, b = bf(M, K), bf(N, K, scale=K ** -0.5)
            a2, b2 = (bf(M, 64), bf(N, 64, scale=0.1)) if N > 64 else (None, None)
            if glu:
                new = lambda: ops.gemm_nt_rows_glu(a, b, a2=a2, b2=b2)
                old = lambda: ops.glu_fwd(ops.gemm_nt(a, b, a2=a2, b2=b2))
            else:
                new = lambda: ops.gemm_nt_rows(a, b, a2=a2, b2=b2)
                old = lambda: ops.gemm_nt(a, b, a2=a2, b2=b2)
            t_old, t_new, t_old2 = timed(old), timed(new), timed(old)
            wbytes = 2 * N * (K + (64 if a2 is not None else 0))
            fmt = lambda ts: " / ".join(f"{t:.1f}" for t in ts)
            print(f"M {M} {name} [{N} x {K}]: rows kernel {fmt(t_new)} us ({wbytes / min(t_new) / 1e6:.2f} TB/s of weights), tile kernels {fmt(t_old)} | {fmt(t_old2)} us "
                  f"({wbytes / min(t_old + t_old2) / 1e6:.2f} TB/s)", flush=True)

if what in ("steps", "all"):
    m = HipCausalLM(DecoderConfig.llama_3_2_1b(vocab_size=V, pad_token_id=V - 1))
    m.enable_lora(16, 32, 0.05)
    for n_, p_ in m.named_parameters():
        if n_.endswith(".B"):
            p_.data.normal_(0, 0.01)
    m.eval()
    wbytes = sum(w.numel() * 2 for ws in (m.wqkv, m.wo, m.wgu, m.wdown) for w in ws) + m.embed.numel() * 2
    wbytes += sum(s.A.numel() * 2 + s.B.numel() * 2 for layer in m.lora for s in layer.values())
    print(f"weight bytes a step: {wbytes / 1e9:.3f} GB", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)

    def gen_ms(p, pm, new):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        seq = m.generate(input_ids=p, attention_mask=pm, max_new_tokens=new, pad_token_id=V - 1, use_graph=True)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1), seq

    for B in Bs:
        p = torch.randint(1000, 100000, (B, 1024), device="cuda", generator=g)
        pm = torch.ones_like(p, dtype=torch.float32)
        res = []
        for arm, on in (("rows", True), ("tile", False), ("tile again", False), ("rows again", True)):
            m.decode_rows = on
            gen_ms(p, pm, 128)                                   # captures (first time) and warms
            steps = []
            for _ in range(2):
                t_long, seq = gen_ms(p, pm, 128)
                t_short, _ = gen_ms(p, pm, 32)
                steps.append((t_long - t_short) / 96)
            res.append((arm, min(steps), max(steps)))
        print(f"B {B}: " + "; ".join(f"{arm} {lo:.3f}-{hi:.3f} ms a step ({B / lo * 1e3:.0f} tokens/s, {wbytes / lo / 1e6 / 8000:.3f} of 8 TB/s)" for arm, lo, hi in res), flush=True)
        m.__dict__.pop("_gen_graphs", None)                      # the captured steps own their KV caches
        torch.cuda.empty_cache()
