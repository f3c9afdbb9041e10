"""CPU model of the resolve phase of encode_flow_kernel: which position should a lane's first chain walk start from?

The claim-merge parse is simulated as in scripts/archive/sim_claim.py (64 lanes in lockstep, one trie step or one emission per
trip, chunk starts at equal numbers of runs); its claim set and token lengths then go through the kernel's correction loop --
lane c owns positions [PW c, PW c + PW), walks the length pointers from a first entry, and every pass replaces the entries that
differ from the left neighbour's exit -- for each rule that picks the first entry:

    own        the first claimed position of the lane's own block (the kernel before the lead-in walk)
    last-1     follow from the LAST claimed position of block c - 1
    lead L     follow from the first claimed position of the farthest of blocks c - L .. c - 1 that holds one (own if none does)

Prints, per record, the correction passes per segment and the number of wrong first entries: blocks whose first entry differs
from the entry the loop ends with (lane 0 starts at the carry and never counts; a block the chain jumps over counts when its
guess is not the position the chain passes it at).  Usage: sim_resolve_entry.py [LEAD ...]
(default 1 2); SEG and PW from the environment (3456 and 64: the bench plan)."""
import importlib.util
import json
import os
import pickle
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

spec = importlib.util.spec_from_file_location("synth", os.path.join(ROOT, "ecg_byte_amd", "synth.py"))
synth = importlib.util.module_from_spec(spec)
spec.loader.exec_module(synth)
G = os.path.join(ROOT, "tests", "golden")
vocab, merges = pickle.load(open(os.path.join(G, "tokenizer_c2.pkl"), "rb"))
pct = json.load(open(os.path.join(G, "percentiles_c2.json")))

children, token = [dict()], [None]


def insert(bs, tid):
    n = 0
    for b in bs:
        nx = children[n].get(b)
        if nx is None:
            nx = len(children)
            children.append({})
            token.append(None)
            children[n][b] = nx
        n = nx
    token[n] = tid


for b in range(256):
    insert([b], b)
for bs, tid in merges:
    insert(bs, tid)


def parse_segment(sym, sb, se, carry, lanes_n=64):
    """The claim-merge parse of positions [sb, se): returns the claimed positions and position -> next token start."""
    n = len(sym)
    rs = [p for p in range(sb, se) if p == sb or sym[p] != sym[p - 1]]
    starts = sorted(set([sb] + [rs[(k * len(rs)) // lanes_n] for k in range(1, lanes_n)]))
    tasks = [max(s, carry) for s in starts]
    tasks = [t for i, t in enumerate(tasks) if i == 0 or t != tasks[i - 1]]
    claimed, nxt, lanes, trips = set(), {}, [], 0
    for r in tasks:
        if r < se and r not in claimed:
            claimed.add(r)
            lanes.append([r, r, 0, r])
    while lanes:
        trips += 1
        alive = []
        for st in lanes:
            r, j, node, best = st
            if node != 0 and token[node] is not None:
                best = j
            if j - r >= 2 and sym[j - 1] == sym[j - 2] and j < n and sym[j] == sym[j - 1] and sym[j] in children[node]:
                c, m = sym[j], 0                                             # a run: up to 32 symbols in one trip
                while j < n and sym[j] == c and c in children[node] and m < 32:
                    if m > 0 and token[node] is not None:
                        best = j
                    node = children[node][c]
                    j += 1
                    m += 1
                alive.append([r, j, node, best])
            elif j < n and sym[j] in children[node]:
                alive.append([r, j + 1, children[node][sym[j]], best])
            else:
                r2 = r + max(best - r, 1)
                nxt[r] = r2
                if r2 < se and r2 not in claimed:
                    claimed.add(r2)
                    alive.append([r2, r2, 0, r2])
        lanes = alive
    return claimed, nxt, trips


def resolve(claimed, nxt, sb, se, carry, PW, rule):
    """The kernel's correction loop; returns (passes, wrong first entries, carry out)."""
    n_blk = (se - sb + PW - 1) // PW
    blocks = [sorted(p for p in claimed if sb + PW * c <= p < min(sb + PW * c + PW, se)) for c in range(n_blk)]

    def follow(p, end):
        while p < end:
            p = nxt.get(p, p + 1)       # (a position nobody claimed holds no length: one step, as in the kernel)
        return p

    entry = []
    for c in range(n_blk):
        s_blk, e_blk = sb + PW * c, min(sb + PW * c + PW, se)
        own = max(blocks[c][0] if blocks[c] else e_blk, s_blk)
        if c == 0:
            entry.append(max(carry, s_blk))
        elif rule == "own":
            entry.append(own)
        elif rule == "last-1":
            entry.append(follow(blocks[c - 1][-1], s_blk) if blocks[c - 1] else own)
        else:
            src = next((blocks[c - d][0] for d in range(rule, 0, -1) if c >= d and blocks[c - d]), None)
            entry.append(follow(src, s_blk) if src is not None else own)
    first = list(entry)
    exits = [follow(entry[c], min(sb + PW * c + PW, se)) for c in range(n_blk)]
    passes = 0
    while True:
        want = [max(carry, sb)] + exits[:-1]
        changed = [c for c in range(n_blk) if want[c] != entry[c]]
        if not changed:
            break
        passes += 1
        for c in changed:
            entry[c] = want[c]
            exits[c] = follow(entry[c], min(sb + PW * c + PW, se))
    return passes, sum(1 for c in range(n_blk) if first[c] != entry[c]), exits[-1]


def main():
    leads = [int(a) for a in sys.argv[1:]] or [1, 2]
    SEG, PW = int(os.environ.get("SEG", "3456")), int(os.environ.get("PW", "64"))
    rules = ["own", "last-1"] + leads
    sig = synth.synth_ecg(2, 5000, seed=0, fs=500)
    for rec in range(2):
        s = O.quantize(sig[rec], pct["percentile_1"], pct["percentile_99"])
        sym = (np.asarray(s).reshape(-1).astype(np.int64) + 97).tolist()
        stats = {r: [0, 0] for r in rules}
        carry, n_seg, n_blocks, trips = 0, 0, 0, 0
        for sb in range(0, len(sym), SEG):
            se = min(sb + SEG, len(sym))
            claimed, nxt, t = parse_segment(sym, sb, se, carry)
            trips += t
            outs = set()
            for r in rules:
                p, w, out = resolve(claimed, nxt, sb, se, carry, PW, r)
                stats[r][0] += p
                stats[r][1] += w
                outs.add(out)
            assert len(outs) == 1, "every rule ends at the same fixed point"
            carry = outs.pop()
            n_seg += 1
            n_blocks += (se - sb + PW - 1) // PW
        print(f"record {rec}: {n_seg} segments of {SEG}, {n_blocks} blocks of {PW}, {trips} parse trips")
        for r in rules:
            name = r if isinstance(r, str) else f"lead {r}"
            print(f"  {name:8s} {stats[r][0] / n_seg:5.2f} passes / segment, {stats[r][1]:4d} wrong first entries")


if __name__ == "__main__":
    main()
