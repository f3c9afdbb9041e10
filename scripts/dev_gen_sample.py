"""Dev-only: sampling generate at Llama-3.2-1B dims with LoRA r16, a 600-token prompt + 128 new tokens, T 0.6 / top_k 50 / top_p 0.9, one process on one GPU:
tokens/s of greedy replayed, torch sampling in the eager loop (the default without the flag), torch sampling with use_graph=True (captured per call) and the device
sampler (replayed graph, captured once), and the sampler kernel's own time from device events at the head's width.  Best of three calls each."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ecg_byte_amd import decoder_ops as ops
from ecg_byte_amd.decoder import DecoderConfig, HipCausalLM
V = 128256 + 256 + 4000 + 3
m = HipCausalLM(DecoderConfig.llama_3_2_1b(vocab_size=V, pad_token_id=V - 1))
m.enable_lora(16, 32, 0.05)
for n_, p_ in m.named_parameters():
    if n_.endswith(".B"):
        p_.data.normal_(0, 0.01)
m.eval()
g = torch.Generator(device="cuda").manual_seed(0)
p = torch.randint(1000, 100000, (1, 600), device="cuda", generator=g)
pm = torch.ones_like(p, dtype=torch.float32)
sam = dict(do_sample=True, temperature=0.6, top_k=50, top_p=0.9)
print("GPU:", torch.cuda.get_device_name(0), "| host:", os.uname().nodename)
for name, kw in (("greedy, replayed graph", dict()), ("torch sampling, eager loop", sam), ("torch sampling, use_graph=True (captured per call)", dict(use_graph=True, **sam)),
                 ("device sampler, replayed graph", dict(device_sampler=True, **sam))):
    best = None
    for it in range(4):                                           # (the first call captures where a graph is kept)
        torch.manual_seed(it)
        torch.cuda.synchronize(); t = time.perf_counter()
        seq = m.generate(input_ids=p, attention_mask=pm, max_new_tokens=128, pad_token_id=V - 1, **kw)
        torch.cuda.synchronize(); dt = time.perf_counter() - t
        best = dt if best is None or it == 1 else min(best, dt)   # best of calls 1..3
    print(f"{name}: {1e3 * best:.0f} ms ({128 / best:.1f} tokens/s)")
# the kernel alone: one row of the head's width (random logits of the spread a trained head gives), then the greedy choice for comparison
x = (3.0 * torch.randn((1, m.embed.shape[0]), device="cuda", generator=g)).to(torch.bfloat16)
seed2, scratch = torch.tensor([1, 2], dtype=torch.int64, device="cuda"), ops.sample_scratch(1, "cuda")
for name, fn in (("sample_rows (T 0.6, k 50, p 0.9)", lambda s: ops.sample_rows(x, V, 0.6, 50, 0.9, seed2, s, scratch)),
                 ("sample_rows (T 1, k off, p 1)", lambda s: ops.sample_rows(x, V, 1.0, 0, 1.0, seed2, s, scratch)), ("argmax_rows", lambda s: ops.argmax_rows(x, V))):
    for s in range(5):
        fn(s)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for s in range(200):
        fn(s)
    ev[1].record()
    torch.cuda.synchronize()
    print(f"{name}: {1e3 * ev[0].elapsed_time(ev[1]) / 200:.1f} us per launch (n {V}, 200 launches back to back)")
ops.sample_check(scratch)
