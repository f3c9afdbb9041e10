"""The attention host layer without a GPU: which kernels a call launches, with what grid, block and dynamic LDS (ecgb_attn_launch_plan), against
tests/golden/attn_plan_parent.json -- what the commit BEFORE the plan existed launched for the same arguments, recorded through its real entry points with
the launch helpers logging instead of launching.  Operands are addresses inside one host buffer and are never read.  Refused calls: the recorded return
code and message, under the called entry point's own name.  Also: every required pointer refused when null."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_plan_parent.json")
ENTRIES = ("ecgb_attn_fwd", "ecgb_attn_bwd", "ecgb_attn_bwd_rope", "ecgb_attn_fwd_dropout", "ecgb_attn_bwd_dropout")   # ecgb_attn_launch_plan's `entry`
FWD, BWD, ROPE, FWD_DROP, BWD_DROP = range(5)
STAGINGS = (0, 1, 2, 2 | 0x100, 2 | 0x200, 2 | 0x400, 2 | 0x700)
SEQS = (1, 64, 127, 128, 129, 1000, 2048)
LIMIT = {64: 28608, 128: 24576, 256: 8192}       # the last accepted length of each head dim
OPERANDS = ("q", "k", "v", "mask", "o", "do", "lse", "delta", "dq", "dk", "dv", "cos", "sin")


def case(entry, D, S, Hq=4, Hkv=2, B=2, staging=2, waves=4, pass_p=0, p=0.0, ld=None, mis=None, scratch="full"):
    """ld: row strides that differ from the fused buffer's (q / k / v / dq / dk / dv: (Hq + 2 Hkv) D, o: Hq D); mis: bytes added to an operand's address;
    scratch: none | small (16 bytes short of the slabs) | slabs | full (what ecgb_attn_bwd_scratch_bytes asks for) | odd (full, 8 bytes off alignment)."""
    return dict(entry=entry, D=D, S=S, Hq=Hq, Hkv=Hkv, B=B, staging=staging, waves=waves, pass_p=pass_p, p=p, ld=ld or {}, mis=mis or {}, scratch=scratch)


def key(c):
    extra = "".join(f" ld{k}={v}" for k, v in sorted(c["ld"].items())) + "".join(f" {k}+{v}" for k, v in sorted(c["mis"].items()))
    return (f"{ENTRIES[c['entry']][5:]} D{c['D']} S{c['S']} B{c['B']} Hq{c['Hq']} Hkv{c['Hkv']} st{c['staging']:#x} w{c['waves']} pp{c['pass_p']} "
            f"p{c['p']} scr:{c['scratch']}{extra}")


def cases():
    out = []
    both = (FWD, BWD)
    # every (staging, lean waves, group size, length) at head_dim 64; the staging's low bits and pass_p at 256; a thinner grid at 128
    for e in both:
        for S in SEQS:
            for G in (1, 2, 4, 8):
                out += [case(e, 64, S, Hq=8, Hkv=8 // G, staging=st, waves=w) for st in STAGINGS for w in (4, 8)]
                out += [case(e, 256, S, Hq=8, Hkv=8 // G, staging=st, pass_p=pp) for st in (0, 1, 2) for pp in (0, 1)]
            out += [case(e, 128, S, Hq=8, Hkv=8 // G, staging=st) for st in (0, 2) for G in (1, 4)]
    # the last accepted and the first refused length
    for e in both:
        for D, last in LIMIT.items():
            for S in (last, last + 1):
                out += [case(e, D, S, B=1, Hq=2, Hkv=1, staging=st, waves=w) for st in (0, 1, 2) for w in ((4, 8) if D == 64 else (4,))]
    # Gemma-like: the query heads of the one KV head split over workgroups, fp32 slabs and the ordered reduction behind them
    for S in (2048, 200):
        for st in (0, 2):
            for pp in (0, 1):
                out += [case(BWD, 256, S, B=1, Hq=8, Hkv=1, staging=st, pass_p=pp, scratch=scr) for scr in ("none", "small", "slabs", "full", "odd")]
        out.append(case(FWD, 256, S, B=1, Hq=8, Hkv=1))
    # head_dim 256: each operand of the LDS-DMA predicate made ineligible in turn (k, v: forward and dQ; q, dO: dK / dV)
    for e in both:
        for op in ("q", "k", "v") + (("do",) if e == BWD else ()):
            ldname = "o" if op == "do" else op
            for pp in (0, 1):
                out.append(case(e, 256, 200, pass_p=pp, mis={op: 2}))
                out.append(case(e, 256, 200, pass_p=pp, ld={ldname: 4 * 256 + 4}))            # & 7 set: the entry points refuse it
                out.append(case(e, 256, 200, pass_p=pp, ld={ldname: 1 << 25}))                 # 64 rows past 32 bits
                out.append(case(e, 256, 200, pass_p=pp, ld={ldname: (1 << 25) - 8}))           # the last stride inside them
    # dropout: the register-staged family whatever the staging; p == 0 is the plain call; its refusals
    for e in (FWD_DROP, BWD_DROP):
        for S in (1, 129, 1000):
            for G in (1, 4):
                out += [case(e, 64, S, Hq=8, Hkv=8 // G, staging=st, waves=w, p=0.25) for st in (0, 1, 2) for w in (4, 8)]
        out += [case(e, D, 129, p=0.0, staging=st) for D in (64, 128, 256) for st in (0, 2)]
        out += [case(e, D, 129, p=0.25) for D in (32, 128, 256)]
        out += [case(e, 64, 129, p=p) for p in (1.0, -0.1, 1.5)]
        out += [case(e, 64, 28609, p=0.25), case(e, 64, 28608, p=0.25, B=1, Hq=2, Hkv=1), case(e, 64, 129, p=0.25, ld={"q": 8 * 64 + 4})]
    out += [case(BWD_DROP, 64, 129, p=0.25, ld={"dk": 8 * 64 + 2})]
    # the RoPE form: head_dim 64 on the lean kernels with 16-byte aligned gradient rows, and nothing else
    for S in (1, 129, 2048):
        out += [case(ROPE, 64, S, Hq=8, Hkv=8 // G, waves=w) for G in (1, 4) for w in (4, 8)]
    out += [case(ROPE, 64, 129, staging=st) for st in STAGINGS]
    out += [case(ROPE, D, 129) for D in (32, 128, 256)]
    out += [case(ROPE, 64, 129, ld={"dq": 8 * 64 + 4}), case(ROPE, 64, 129, ld={"dk": 8 * 64 + 4}), case(ROPE, 64, 129, ld={"dv": 8 * 64 + 4}),
            case(ROPE, 64, 129, ld={"dv": 8 * 64 + 2}), case(ROPE, 64, 129, ld={"k": 8 * 64 + 4}), case(ROPE, 64, 28609), case(ROPE, 64, 129, Hq=3)]
    out += [case(ROPE, 64, 129, mis={op: 8}) for op in ("dq", "dk", "dv", "cos", "sin")]
    # strides: rows off 8 elements, gradient rows off 4 (and on 4 but off 8: taken, with narrower stores), misaligned operands at head_dim 64
    for e in both:
        for D in (64, 256):
            out += [case(e, D, 129, ld={n: 8 * D + 4}) for n in ("q", "k", "v", "o")]
            out += [case(e, D, 129, mis={n: 2}) for n in ("q", "k", "v", "o")]
    for D in (64, 128, 256):
        out += [case(BWD, D, 129, ld={n: 8 * D + 2}) for n in ("dq", "dk", "dv")]
        out += [case(BWD, D, 129, ld={n: 8 * D + 4}) for n in ("dq", "dk", "dv")]
    # shapes
    for e in both:
        out += [case(e, 64, 129, B=0), case(e, 64, 0), case(e, 64, 129, Hq=0, Hkv=0), case(e, 64, 129, Hq=4, Hkv=3), case(e, 32, 129), case(e, 96, 129),
                case(e, 64, 129, B=64, Hq=32, Hkv=8), case(e, 256, 129, B=64, Hq=8, Hkv=1), case(e, 128, 300, B=3, Hq=6, Hkv=3)]
    seen = set()
    return [c for c in out if not (key(c) in seen or seen.add(key(c)))]


def set_switches(lib, c):
    assert lib.ecgb_set_attn_fwd_staging(c["staging"]) == 0 and lib.ecgb_set_attn_lean_waves(c["waves"]) == 0 and lib.ecgb_set_attn_d256_pass_p(c["pass_p"]) == 0


def reset_switches(lib):
    lib.ecgb_set_attn_fwd_staging(2), lib.ecgb_set_attn_lean_waves(4), lib.ecgb_set_attn_d256_pass_p(0)


def operands(lib, c, base):
    """(addresses by operand name, strides by name, scratch address or None, scratch bytes) of a case; the switches must be set"""
    addr = {n: base + 256 * i + c["mis"].get(n, 0) for i, n in enumerate(OPERANDS)}
    fused = (c["Hq"] + 2 * c["Hkv"]) * c["D"]
    ld = {n: fused for n in ("q", "k", "v", "dq", "dk", "dv")}
    ld["o"] = c["Hq"] * c["D"]
    ld.update(c["ld"])
    shape = (c["B"], c["S"], c["Hq"], c["Hkv"], c["D"])
    full = lib.ecgb_attn_bwd_scratch_bytes(*shape)
    lib.ecgb_set_attn_d256_pass_p(0)
    slabs = lib.ecgb_attn_bwd_scratch_bytes(*shape)
    lib.ecgb_set_attn_d256_pass_p(c["pass_p"])
    nbytes = {"none": 0, "small": max(slabs - 16, 0), "slabs": slabs, "full": full, "odd": full}[c["scratch"]]
    scratch = None if c["scratch"] == "none" or nbytes == 0 else base + 4096 + (8 if c["scratch"] == "odd" else 0)
    return addr, ld, scratch, nbytes


def plan(lib, c, base):
    """-> [return code, message or "", ["kernel grid block lds", ...], [lean_hw_log2, head_splits, byte offset of pbuf in the scratch or -1]]"""
    set_switches(lib, c)
    a, ld, scratch, nbytes = operands(lib, c, base)
    n, gbl, aset, names = C.c_int(-1), (C.c_int * 12)(), (C.c_longlong * 3)(), C.create_string_buffer(512)
    rc = lib.ecgb_attn_launch_plan(c["entry"], c["p"], a["q"], ld["q"], a["k"], ld["k"], a["v"], ld["v"], a["do"], ld["o"], a["dq"], ld["dq"], a["dk"], ld["dk"],
                                   a["dv"], ld["dv"], a["cos"], a["sin"], c["B"], c["S"], c["Hq"], c["Hkv"], c["D"], scratch, nbytes, C.byref(n), gbl, aset, names, len(names))
    if rc:
        return [rc, (lib.ecgb_last_error() or b"").decode(), [], []]
    kern = names.value.decode().split("\n")
    assert len(kern) == n.value, (kern, n.value)
    return [0, "", [f"{kern[i]} {gbl[3 * i]} {gbl[3 * i + 1]} {gbl[3 * i + 2]}" for i in range(n.value)], list(aset)]


@pytest.fixture(scope="module")
def lib():
    from ecg_byte_amd import _lib
    L = _lib.lib()
    yield L
    reset_switches(L)


@pytest.fixture(scope="module")
def base():
    buf = (C.c_uint8 * 8192)()
    yield (C.addressof(buf) + 63) & ~63


def test_sweep_reaches_every_branch():
    golden = json.load(open(GOLDEN))
    cs = cases()
    assert sorted(golden) == sorted(key(c) for c in cs), "tests/golden/attn_plan_parent.json was recorded for another sweep"
    kernels = {line.rsplit(" ", 3)[0] for g in golden.values() for line in g[2]}
    want = {"attn_fwd_lean_kernel", "attn_fwd_kernel<64, dma>", "attn_fwd_kernel<64>", "attn_fwd_kernel<128>", "attn_fwd_d256_kernel", "attn_fwd_kernel<256>",
            "attn_fwd_kernel<64, dropout>", "attn_bwd_dq_lean_kernel", "attn_bwd_dq_dma_kernel", "attn_bwd_dq_kernel<64>", "attn_bwd_dq_kernel<128>",
            "attn_bwd_dq_kernel<256>", "attn_bwd_dq_d256_kernel", "attn_bwd_dq_kernel<64, dropout>", "attn_bwd_dkv_lean_kernel", "attn_bwd_dkv_dma_kernel",
            "attn_bwd_dkv_kernel<64>", "attn_bwd_dkv_kernel<128>", "attn_bwd_dkv_kernel<64, dropout>", "attn_bwd_dkv_pair_kernel<256>",
            "attn_bwd_dkv_pair_d256_kernel", "attn_bwd_dk_d256_kernel", "attn_bwd_dv_d256_kernel", "attn_dkv_reduce_kernel<256>"}
    assert kernels == want, (sorted(kernels - want), sorted(want - kernels))
    assert {g[0] for g in golden.values()} == {0, -1, -3}
    assert {g[3][1] for g in golden.values() if g[0] == 0} >= {0, 1, 2, 4} and any(g[0] == 0 and g[3][2] >= 0 for g in golden.values())


def test_plan_equals_parent(lib, base):
    golden = json.load(open(GOLDEN))
    bad = []
    for c in cases():
        k = key(c)
        want, got = golden[k], plan(lib, c, base)
        who = ENTRIES[c["entry"]]
        if want[0]:
            # the parent's code and text; the name in front is the called entry point's (the parent said ecgb_attn_bwd for ecgb_attn_bwd_rope's shared checks
            # and the plain names for the dropout entry points at p == 0)
            ok = got[0] == want[0] and got[1].startswith(who + ": ") and got[1].split(": ", 1)[1] == want[1].split(": ", 1)[1]
        else:
            ok = got == want
        if not ok:
            bad.append((k, want, got))
    reset_switches(lib)
    assert not bad, f"{len(bad)} of {len(golden)} differ; the first: {bad[:5]}"


def test_accepted_lengths(lib, base):
    for D, last in LIMIT.items():
        for e in (FWD, BWD):
            for st in STAGINGS:
                for w in (4, 8):
                    assert plan(lib, case(e, D, last, B=1, Hq=2, Hkv=1, staging=st, waves=w), base)[0] == 0, (D, e, st, w)
                    got = plan(lib, case(e, D, last + 1, B=1, Hq=2, Hkv=1, staging=st, waves=w), base)
                    assert got[0] == -3 and got[1].startswith(ENTRIES[e] + ": sequence too long"), (D, e, st, w, got)
    reset_switches(lib)


def test_null_pointers_are_refused(lib, base):
    """each required pointer null in turn: ECGB_ERR_INVALID under the called name, before anything else (the other arguments are unusable too: head_dim 32,
    p = 2, unaligned gradients -- whatever the entry point would say about them comes later)"""
    a = [base + 256 * i for i in range(13)]
    q, k, v, mask, o, do, lse, delta, dq, dk, dv, cos, sin = range(13)
    B, S, Hq, Hkv, D, ld = 2, 64, 4, 2, 32, 8 * 32
    calls = {
        "ecgb_attn_fwd": ((q, k, v, mask, o, lse), lambda x: lib.ecgb_attn_fwd(x[q], ld, x[k], ld, x[v], ld, x[mask], x[o], ld, x[lse], B, S, Hq, Hkv, D, 0.125, None)),
        "ecgb_attn_fwd_dropout": ((q, k, v, mask, o, lse), lambda x: lib.ecgb_attn_fwd_dropout(x[q], ld, x[k], ld, x[v], ld, x[mask], x[o], ld, x[lse], B, S, Hq, Hkv, D,
                                                                                                0.125, 2.0, 7, None)),
        "ecgb_attn_bwd": ((q, k, v, mask, o, do, lse, delta, dq, dk, dv),
                          lambda x: lib.ecgb_attn_bwd(x[q], ld, x[k], ld, x[v], ld, x[mask], x[o], x[do], ld, x[lse], x[delta], x[dq], ld + 2, x[dk], ld, x[dv], ld,
                                                      B, S, Hq, Hkv, D, 0.125, None, 0, None)),
        "ecgb_attn_bwd_dropout": ((q, k, v, mask, o, do, lse, delta, dq, dk, dv),
                                  lambda x: lib.ecgb_attn_bwd_dropout(x[q], ld, x[k], ld, x[v], ld, x[mask], x[o], x[do], ld, x[lse], x[delta], x[dq], ld + 2, x[dk], ld,
                                                                      x[dv], ld, B, S, Hq, Hkv, D, 0.125, None, 0, 2.0, 7, None)),
        "ecgb_attn_bwd_rope": ((q, k, v, mask, o, do, lse, delta, dq, dk, dv, cos, sin),
                               lambda x: lib.ecgb_attn_bwd_rope(x[q], ld, x[k], ld, x[v], ld, x[mask], x[o], x[do], ld, x[lse], x[delta], x[dq], ld + 2, x[dk], ld,
                                                                x[dv], ld, x[cos], x[sin], B, S, Hq, Hkv, D, 0.125, None, 0, None)),
    }
    for name, (required, call) in calls.items():
        rc = call(a)
        assert rc in (-1, -3) and (lib.ecgb_last_error() or b"").decode().startswith(name + ":"), name      # (nothing null: refused for the rest)
        for i in required:
            x = list(a)
            x[i] = None
            rc, msg = call(x), (lib.ecgb_last_error() or b"").decode()
            assert rc == -1 and msg.startswith(name + ":") and "null" in msg.lower(), (name, OPERANDS[i], rc, msg)
