"""Dev: the detokenise launches at the C2 shape -- records of 12 x 5000, the C2 tokenizer, ids from the real encode -- timed with device events: the three
payloads, the histogram, the encode of the same batch beside them, and the host path they replace (decode_text + reverse_normalize_all per record).
    python scripts/dev_detokenize_time.py [records=4096] [host_records=64]
Algorithmic bytes of a payload = 4 T (ids read) + payload written (+ 8 per symbol when the original is read back for the error); shares are of 8 TB/s."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np, torch
from helpers import load_tokenizer
from ecg_byte_amd import synth, _lib
from ecg_byte_amd import tokenizer_utils as tu
from ecg_byte_amd.tokenizer import HipTokenizer, _ptr, _stream_ptr

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
H = int(sys.argv[2]) if len(sys.argv) > 2 else 64
vocab, merges, pc = load_tokenizer("c2")
tk = HipTokenizer(merges)
x = synth.synth_ecg(min(B, 4096), 5000, seed=0)
xd = torch.from_numpy(x).cuda()
if B > 4096:
    xd = xd.repeat((B + 4095) // 4096, 1, 1)[:B].contiguous()
n = 60000
ids = torch.empty((B, n), dtype=torch.int32, device="cuda"); counts = torch.empty((B,), dtype=torch.int32, device="cuda")
tk.quantize_encode(xd, pc, ids_stride=n, out=(ids, counts))
T = int(counts.sum().item())
S = B * n
out8 = torch.empty((B, n), dtype=torch.uint8, device="cuda")
out32 = torch.empty((B, n), dtype=torch.float32, device="cuda")
out64 = torch.empty((B, n), dtype=torch.float64, device="cuda")
values = torch.rand((B, n), dtype=torch.float32, device="cuda")
n_sym = torch.empty((B,), dtype=torch.int32, device="cuda"); flags = torch.empty_like(n_sym); mism = torch.empty_like(n_sym)
diff = torch.empty((B,), dtype=torch.float64, device="cuda")
hist = torch.empty((256 + len(merges),), dtype=torch.int64, device="cuda"); over = torch.empty((), dtype=torch.int64, device="cuda")
L, h, p1, p99 = _lib.lib(), tk._h, float(pc["percentile_1"]), float(pc["percentile_99"])
legs = {
    "encode (quantise + encode, for scale)": (lambda: tk.quantize_encode(xd, pc, ids_stride=n, out=(ids, counts)), 8 * S + 4 * T),
    "bytes": (lambda: L.ecgb_detokenize_hip(h, _ptr(ids), n, _ptr(counts), B, _ptr(out8), n, _ptr(n_sym), _ptr(flags), _stream_ptr()), 4 * T + S),
    "values f32": (lambda: L.ecgb_detokenize_values_f32_hip(h, _ptr(ids), n, _ptr(counts), B, _ptr(values), _ptr(out32), n, _ptr(n_sym), _ptr(flags),
                                                              _stream_ptr()), 8 * T + 4 * S),
    "signal f64": (lambda: L.ecgb_detokenize_signal_f64_hip(h, _ptr(ids), n, _ptr(counts), B, p1, p99, _ptr(out64), n, _ptr(n_sym), _ptr(flags), None, 0,
                                                              None, None, _stream_ptr()), 4 * T + 8 * S),
    "signal f64 + error against the original": (lambda: L.ecgb_detokenize_signal_f64_hip(h, _ptr(ids), n, _ptr(counts), B, p1, p99, _ptr(out64), n, _ptr(n_sym),
                                                                                           _ptr(flags), _ptr(xd), n, _ptr(diff), _ptr(mism), _stream_ptr()),
                                                4 * T + 16 * S),
    "histogram": (lambda: L.ecgb_token_histogram_hip(_ptr(ids), n, _ptr(counts), B, _ptr(hist), hist.numel(), _ptr(over), _stream_ptr()), 4 * T),
}
print(f"{B} records of 12 x 5000: {S} symbols, {T} tokens ({S / T:.2f} symbols a token)", flush=True)
for name, (fn, alg) in legs.items():
    for _ in range(3):
        rc = fn()
        assert rc is None or rc == 0 or isinstance(rc, tuple), rc
    reps = 20
    best = 1e30
    for _ in range(3):                                         # three windows of 20 launches: the spread is printed with the figure
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        best = min(best, ms)
        print(f"  {name}: {ms:.4f} ms per launch, {alg / 1e6:.1f} MB algorithmic, {alg / ms / 1e6 / 8000:.3f} of 8 TB/s", flush=True)
assert int(n_sym.min()) == n and int(flags.max()) == 0 and int(mism.max()) == 0 and int(hist.sum()) == T
# the host path: what train_tokenizer's self-check does per record
ids_h, counts_h = ids[:H].cpu().numpy(), counts[:H].cpu().numpy()
t0 = time.perf_counter()
for b in range(H):
    text = tu.decode_text([int(v) for v in ids_h[b, : counts_h[b]]], vocab)
    tu.reverse_normalize_all(np.array(list(text)).reshape(12, 5000), pc)
dt = time.perf_counter() - t0
print(f"host path (decode_text + reverse_normalize_all): {dt / H * 1e3:.2f} ms a record over {H} records = {dt / H * B:.1f} s for {B}", flush=True)
