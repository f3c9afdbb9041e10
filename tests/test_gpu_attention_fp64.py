"""The softmax kernels against float64 at the inputs where they go wrong: peaked scores, attention sinks, scores that rise tile after tile
past the overflow of exp2, flat rows, large values; masks with holes, whole masked tiles past key 4 096, right padding, fully padded rows,
non-1 mask values; sequences up to the longest ecgb_attn_fwd takes; every head_dim-64 kernel form and the grouped-query layouts the lean
launch packs differently.

Reference: the same bf16 inputs in float64 on the device, a chunk of query rows at a time (S = 28 672 fits), with the analytic backward
(dP = dO V^T, dS = P o (dP - rowsum(dO o O)), dq = scale dS K, dk = scale dS^T Q, dv = P^T dO).  Errors are taken PER (row, head) and the
worst row is held to its bound, so one wrong 64-row tile of a long sequence cannot hide in a whole-tensor norm.

Bounds (BOUND_* below; "2 ln2 delta" stands for its exact form 2^(2 delta) - 1, which the code uses: large delta is not first order).  u = 2^-8 is bf16's unit roundoff (8 significant bits).  delta_i (log2 units) bounds the error of row i's scores as a kernel forms them:
    delta_i = (k_op * u + D * 2^-24) * max_j sum_d |q_id k_jd| * scale * log2(e)
k_op = 0 for kernels that multiply bf16 q and k exactly (fp32 accumulation over D terms: the 2^-24 term); k_op = 1 for the lean head_dim-64
kernels, whose register operand is pre-scaled by scale * log2(e) and rounded to bf16 (half an ulp of every element: a score error that
grows with |score|); the backward sees the forward's error in lse and its own in the scores, so its term is doubled.
  o:    per row, || o - o_ref || / || P |V| ||: the rounding of P to bf16 (u), of the output (u), the fp32 row sum against the bf16 P
        the products use (u), and a probability off by exp(+-2 ln2 delta) -> 3u + 2 ln2 delta.  The denominator P|V| is the size the roundings
        scale with (it is >= |o|, = |o| when every v of the row points one way).
  lse:  |lse - lse_ref| <= delta + log2(1 + 28 672 * 2^-24) (the fp32 sum of at most 28 672 exponentials) <= delta + 2^-8.
  grad: per row, || g - g_ref || / || A_g ||, A_g the row's magnitude -- the same sums over absolute values, which every rounding scales
        with and which does not vanish where the exact gradient cancels (a row whose only visible key is itself has dq = 0 exactly):
            A_dq,i = scale sum_j T_ij |k_j|,  A_dk,j = scale sum_i T_ij |q_i|,  A_dv,j = sum_i p_ij |dO_i|,
            T_ij = p_ij (M_ij + sum_l p_il M_il),  M_ij = |dO_i|.|v_j|  (>= |dP_ij|, and sum_l p_il M_il >= |rowsum(dO o O)_i|).
        dS_ij = p_ij (dP_ij - D_i) is off by at most T_ij times: u (dS to bf16) + 3u + 2 ln2 delta (D_i from the bf16 O: the o bound)
        + 2 ln2 delta (p from the forward's lse and the backward's own scores); plus u for the bf16 output -> 5u + 4 ln2 delta
        (dv = P^T dO: u + 2 ln2 delta for P, u for the output, within it).
Every form is held to these bounds with k_op = 0 against the reference of ITS OWN score operands (attn_ref_fp64's ops_: the lean kernels'
bf16 pre-scaled q or k emulated bit for bit), so a lean kernel at peaked, sink or rising scores is checked as tightly as the others.  Its
distance from the operation itself -- the pre-scale rounding, which grows with |score| (o up to ~15x the round-2 kernels' error at +-40
nats) -- is held besides to the k_op = 1 bounds, and at the families whose scores stay within a few nats (LEAN_TIGHT_FAMILIES), where that
rounding is not the dominant error, to 1.5x the round-2 kernels' whole-tensor error plus 1e-4.
Below 2^-126 the hardware exp2 flushes to zero (and bf16 has no more normal numbers): probabilities carry that absolute floor."""
import math

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U = 2.0 ** -8                                                          # bf16: 8 significant bits, round to nearest
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
FP32 = 2.0 ** -24

EXPM1 = lambda delta: torch.expm1(LN2 * delta)                         # noqa: E731  2^delta - 1: a probability off by delta log2 units
BOUND_O = lambda delta: 3 * U + EXPM1(2 * delta)                       # noqa: E731  per-row relative, denominator || P |V| ||
BOUND_LSE = lambda delta: delta + 2.0 ** -8                            # noqa: E731  absolute, log2 units
BOUND_GRAD = lambda delta: 5 * U + 2 * EXPM1(2 * delta)                # noqa: E731  per-row relative, denominator || A_g ||
LEAN_VS_ROUND2 = (1.5, 1e-4)                                           # a lean form's error <= 1.5 x the round-2 kernels' + 1e-4
LEAN_TIGHT_FAMILIES = ("gauss", "flat", "big-v")
TINY = 2.0 ** -126                                                     # fp32 / bf16 smallest normal: exp2 flushes below it
PROBS_ABS = 1e-2                                                       # attn_probs: every probability within 1e-2 absolute (exact-score lse)

MEASURED = {}                                                          # (test id / form, quantity) -> (worst error, bound)


def _record(key, err, bound):
    MEASURED[key] = (float(err), float(bound))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from ecg_byte_amd import decoder_ops
    yield decoder_ops
    # the measured worst errors against their bounds (shown with -s); the ones with less than 2x headroom marked
    for (tag, qty), (e, b) in sorted(MEASURED.items()):
        print(f"{tag:70s} {qty:14s} {e:.3e} / {b:.3e}{'  <2x' if e > b / 2 else ''}")


# ---------------------------------------------------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def fam_gauss(B, S, Hq, Hkv, D, seed):
    """gauss: q, k, v and dO all N(0, 1) -- the inputs every comparison used before."""
    g = _gen(seed)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device="cuda", generator=g)
    do = torch.randn(B * S, Hq * D, device="cuda", generator=g)
    return qkv, do


def fam_peaked(B, S, Hq, Hkv, D, seed):
    """peaked: q and k N(0, 3.5^2): the scaled score q.k / sqrt(D) has a standard deviation of 12.25 nats, so a row of a few dozen keys
    spans +-40 nats (checked on the reference) and its softmax is nearly one-hot, as in the rows of a pretrained model."""
    qkv, do = fam_gauss(B, S, Hq, Hkv, D, seed)
    qkv[:, : (Hq + Hkv) * D] *= 3.5
    return qkv, do


def _control(qkv, B, S, Hq, Hkv, D, kscore):
    """Plant scores: q dims 0 and 1 = 1 for every query head, k dims 0 / 1 of key j = kscore(j) split as (low, high) parts so that both are
    exact in bf16 (q.k = kscore(j) exactly); the other dims keep their small noise."""
    x = qkv.view(B, S, Hq + 2 * Hkv, D)
    x[:, :, :Hq, :2] = 1.0
    j = torch.arange(S, device="cuda")
    lo, hi = kscore(j)
    x[:, :, Hq:Hq + Hkv, 0] = lo[None, :, None].float()
    x[:, :, Hq:Hq + Hkv, 1] = hi[None, :, None].float()


def _pow2_at_least(x):
    return 2.0 ** math.ceil(math.log2(x))


def fam_rising(B, S, Hq, Hkv, D, seed, step_log2=12):
    """rising: key j scores kappa * (j // 64) above noise of N(0, 0.25) per q and k element, kappa a power of two with
    kappa * scale >= step_log2 * ln 2 nats: every query sees each successive 64-key tile at least step_log2 log2 units above the one
    before (with step_log2 = 130 the tile's exp2 overflows on the lean forward's fast path)."""
    qkv, do = fam_gauss(B, S, Hq, Hkv, D, seed)
    qkv[:, : (Hq + Hkv) * D] *= 0.5
    kappa = _pow2_at_least(step_log2 * LN2 * math.sqrt(D))
    _control(qkv, B, S, Hq, Hkv, D, lambda j: (kappa * ((j // 64) % 256), kappa * 256 * ((j // 64) // 256)))
    return qkv, do


def fam_rising_big(B, S, Hq, Hkv, D, seed):
    """rising-big: rising with jumps of more than 128 log2 units from tile to tile."""
    return fam_rising(B, S, Hq, Hkv, D, seed, step_log2=130)


def _sink(B, S, Hq, Hkv, D, seed, where):
    qkv, do = fam_gauss(B, S, Hq, Hkv, D, seed)
    qkv[:, : (Hq + Hkv) * D] *= 0.5
    c = 25.0 * math.sqrt(D)                                            # q.k = c: 25 nats after the scale
    hi = _pow2_at_least(c)
    _control(qkv, B, S, Hq, Hkv, D, lambda j: (torch.where(where(j), torch.full_like(j, int(hi)), torch.zeros_like(j)),
                                                 torch.where(where(j), torch.full_like(j, int(c - hi)), torch.zeros_like(j))))
    return qkv, do


def fam_sink_first(B, S, Hq, Hkv, D, seed):
    """sink-first: key 0 scores 25 nats above the rest (q.k = 25 sqrt(D) on two planted dims), the attention sink of a pretrained model;
    q and k otherwise N(0, 0.25)."""
    return _sink(B, S, Hq, Hkv, D, seed, lambda j: j == 0)


def fam_sink_last(B, S, Hq, Hkv, D, seed):
    """sink-last: every query's LAST visible key -- the key at its own position -- scores about 25 nats above the rest: q_i and k_i both
    alpha * u_i for a random unit vector u_i shared by the query heads of a group, alpha^2 / sqrt(D) = 25, so q_i.k_i scores 25 nats and
    q_i.k_j (j != i) 25 u_i.u_j = N(0, 25^2 / D) nats; v and dO N(0, 1).  The running maximum has to move up at the row's very end."""
    qkv, do = fam_gauss(B, S, Hq, Hkv, D, seed)
    u = torch.randn(B, S, 1, D, device="cuda", generator=_gen(seed + 1))
    u = u / u.norm(dim=-1, keepdim=True) * math.sqrt(25.0 * math.sqrt(D))
    x = qkv.view(B, S, Hq + 2 * Hkv, D)
    x[:, :, : Hq + Hkv] = u + 0.05 * x[:, :, : Hq + Hkv]
    return qkv, do


def fam_flat(B, S, Hq, Hkv, D, seed):
    """flat: q = 0, so every visible key scores 0 and lse = log2(number of visible keys) exactly; o is the mean of the visible v."""
    qkv, do = fam_gauss(B, S, Hq, Hkv, D, seed)
    qkv[:, : Hq * D] = 0.0
    return qkv, do


def fam_big_v(B, S, Hq, Hkv, D, seed):
    """big-v: v and dO N(0, 100^2): values and gradients far from 1 (the bf16 P and dS must not lose them)."""
    qkv, do = fam_gauss(B, S, Hq, Hkv, D, seed)
    qkv[:, (Hq + Hkv) * D:] *= 100.0
    return qkv, do * 100.0


FAMILIES = {"gauss": fam_gauss, "peaked": fam_peaked, "rising": fam_rising, "rising-big": fam_rising_big, "sink-first": fam_sink_first,
            "sink-last": fam_sink_last, "flat": fam_flat, "big-v": fam_big_v}


def make_inputs(family, B, S, Hq, Hkv, D, seed):
    qkv, do = FAMILIES[family](B, S, Hq, Hkv, D, seed)
    return qkv.to(torch.bfloat16).contiguous(), do.to(torch.bfloat16).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# masks (float [B, S]; key j visible to query i iff j <= i and mask[b, j] != 0)
# ---------------------------------------------------------------------------------------------------------------------
def make_mask(name, B, S):
    m = torch.ones(B, S, device="cuda")
    if name == "none":
        pass
    elif name.startswith("left"):                                      # left pad: keys [0, n) masked ("lefthalf": longer than S / 2)
        n = S // 2 + 37 if name == "lefthalf" else int(name[4:])
        m[:, : min(n, S)] = 0
        if B > 1:
            m[1:, : min(n + 1, S)] = 0                                 # a ragged second row
    elif name == "hole":                                               # one masked key inside an otherwise visible tile
        m[:, (64 + 17) if S > 100 else S // 2] = 0
    elif name == "tilehole":                                           # whole 64-key tiles masked between visible ones; tile 64 (keys 4 096..4 159) too
        m[:, 64:128] = 0
        if S > 4160 + 64:
            m[:, 4096:4160] = 0
    elif name == "alternate":                                          # every other key
        m[:, 1::2] = 0
    elif name == "trailing":                                           # right padding
        m[:, S - max(1, S // 3):] = 0
    elif name == "rowpad":                                             # batch row 1 fully padded, row 0 a short left pad
        m[0, : min(5, S - 1)] = 0
        m[1:] = 0
    elif name == "half":                                               # 0.5 is visible under the contract; a left pad of zeros beside it
        m[:] = 0.5
        m[:, : min(7, S - 1)] = 0
    else:
        raise ValueError(name)
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def _prescaled(t, scale):
    """The lean kernels' pre-scaled operand: bf16(t * fp32(scale * log2 e)), the fp32 product rounded to nearest even as the kernels do it."""
    c32 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    return (t.float() * c32).to(torch.bfloat16).double()


def attn_ref_fp64(qkv, do, mask, B, S, Hq, Hkv, D, scale, ops_=("exact", "exact", "exact"), rows_per_chunk=None):
    """softmax(q k^T * scale + mask) v in float64 and its analytic gradients.  ops_ = the score operands of (forward, dQ, dK / dV): "exact"
    scores q.k * scale * log2 e from the bf16 q and k (the round-2 and register-staged kernels, head_dim 128 / 256), or "lean": the forward and
    dQ form q~.k, dK / dV q.k~ with x~ = bf16(x * scale * log2 e) (the lean head_dim-64 kernels).  lse is the forward's; the backward's
    probabilities are exp2(its own scores - lse) -- what the kernels compute, so a lean form is held to the same tight bounds as the others.
    The default is the operation itself.  Returns a dict: o / dq [B, S, Hq, D], dk / dv [B, S, Hkv, D], lse [B, Hq, S] (log2 units, +inf for
    a row with no visible key), o_scale [B, S, Hq] (|| P |V| ||), a_dq [B, S, Hq] / a_dk, a_dv [B, S, Hkv] (|| A_g ||, module docstring),
    mag [B, S, Hq] (max over visible keys of sum_d |q_d k_d| * scale * log2 e: what delta() scales) and mag_k [B, S, Hkv] (its max over
    the rows that see key j), live [B, S, Hq], smin / smax (scaled scores of visible pairs, nats)."""
    G = Hq // Hkv
    x = qkv.view(B, S, Hq + 2 * Hkv, D)
    dov = do.view(B, S, Hq, D)
    f64 = dict(dtype=torch.float64, device="cuda")
    out = {k: torch.zeros(B, S, Hq, D, **f64) for k in ("o", "dq")}
    out["a_dq"] = torch.zeros(B, S, Hq, **f64)
    out.update({k: torch.zeros(B, S, Hkv, D, **f64) for k in ("dk", "dv", "a_dk", "a_dv")})
    out["lse"] = torch.empty(B, Hq, S, **f64)
    out["o_scale"] = torch.zeros(B, S, Hq, **f64)
    out["mag"] = torch.zeros(B, S, Hq, **f64)
    smin, smax = math.inf, -math.inf
    C = rows_per_chunk or max(64, min(S, (1 << 24) // S))
    c2 = scale * LOG2E
    f_op, q_op, k_op = ops_
    for b in range(B):
        vis_key = mask[b] != 0
        for g in range(Hkv):
            k = x[b, :, Hq + g].double()
            v = x[b, :, Hq + Hkv + g].double()
            kt = _prescaled(x[b, :, Hq + g], scale)
            ka, va = k.abs(), v.abs()
            a_dk, a_dv = torch.zeros(S, D, **f64), torch.zeros(S, D, **f64)
            for hq in range(g * G, (g + 1) * G):
                q = x[b, :, hq].double()
                qt = _prescaled(x[b, :, hq], scale)
                dO = dov[b, :, hq].double()
                for r0 in range(0, S, C):
                    r1 = min(S, r0 + C)
                    qi = torch.arange(r0, r1, device="cuda")
                    vis = (torch.arange(r1, device="cuda")[None, :] <= qi[:, None]) & vis_key[None, :r1]
                    sE = (q[r0:r1] @ k[:r1].T) * c2                           # log2 units
                    if bool(vis.any()):
                        smin, smax = min(smin, float(sE[vis].min()) * LN2), max(smax, float(sE[vis].max()) * LN2)
                    sQ = qt[r0:r1] @ k[:r1].T if "lean" in (f_op, q_op) else sE
                    sK = q[r0:r1] @ kt[:r1].T if k_op == "lean" else sE
                    sF = (sQ if f_op == "lean" else sE).masked_fill(~vis, -math.inf)
                    mx = sF.amax(1, keepdim=True)
                    live = torch.isfinite(mx)
                    mx0 = torch.where(live, mx, torch.zeros_like(mx))
                    l = torch.exp2(sF - mx0).sum(1, keepdim=True)
                    lse = torch.where(live, mx0 + torch.log2(torch.where(live, l, torch.ones_like(l))), torch.full_like(l, math.inf))
                    P = torch.exp2(sF - lse).masked_fill(~vis, 0.0)
                    Pq = torch.exp2((sQ if q_op == "lean" else sE) - lse).masked_fill(~vis, 0.0)
                    Pk = torch.exp2(sK - lse).masked_fill(~vis, 0.0)
                    out["lse"][b, hq, r0:r1] = lse[:, 0]
                    o = P @ v[:r1]
                    out["o"][b, r0:r1, hq] = o
                    out["o_scale"][b, r0:r1, hq] = (P @ va[:r1]).norm(dim=1)
                    out["mag"][b, r0:r1, hq] = ((q[r0:r1].abs() @ ka[:r1].T) * c2).masked_fill(~vis, 0.0).amax(1)
                    dP = dO[r0:r1] @ v[:r1].T
                    Di = (dO[r0:r1] * o).sum(1, keepdim=True)
                    out["dq"][b, r0:r1, hq] = scale * ((Pq * (dP - Di)) @ k[:r1])
                    dSk = Pk * (dP - Di)
                    out["dk"][b, :r1, g] += scale * (dSk.T @ q[r0:r1])
                    out["dv"][b, :r1, g] += Pk.T @ dO[r0:r1]
                    M = dO[r0:r1].abs() @ va[:r1].T
                    Tq = Pq * (M + (Pq * M).sum(1, keepdim=True))
                    Tk = Pk * (M + (Pk * M).sum(1, keepdim=True))
                    out["a_dq"][b, r0:r1, hq] = scale * (Tq @ ka[:r1]).norm(dim=1)
                    a_dk[:r1] += scale * (Tk.T @ q[r0:r1].abs())
                    a_dv[:r1] += Pk.T @ dO[r0:r1].abs()
                    del sE, sQ, sK, sF, P, Pq, Pk, dP, dSk, M, Tq, Tk
            out["a_dk"][b, :, g], out["a_dv"][b, :, g] = a_dk, a_dv
    out["a_dk"], out["a_dv"] = out["a_dk"].norm(dim=-1), out["a_dv"].norm(dim=-1)
    out["live"] = torch.isfinite(out["lse"]).permute(0, 2, 1)
    m = out["mag"].view(B, S, Hkv, G).amax(3)                                 # per key: the worst row of the group that sees it (rows >= j)
    out["mag_k"] = torch.flip(torch.cummax(torch.flip(m, [1]), 1).values, [1])
    out["smin"], out["smax"] = smin, smax
    return out


# ---------------------------------------------------------------------------------------------------------------------
# per-row errors
# ---------------------------------------------------------------------------------------------------------------------
def delta(mag, D, k_op):
    """The score-error bound of the module docstring (log2 units) for a kernel with k_op bf16-rounded pre-scaled operands."""
    return (k_op * U + D * FP32) * mag


def whole_rel(x, ref, mag):
    """|| x - ref || / || mag || over the whole tensor (mag: the rows' magnitudes, as per row), float64."""
    return float((x.double() - ref).norm() / mag.norm().clamp_min(1e-300))


def row_rel(x, ref, denom):
    """|| x - ref || over the last dim / denom, float64."""
    return (x.double() - ref).norm(dim=-1) / denom


def check_forward(o, lse, R, B, S, Hq, D, k_op, tag):
    """o [B*S, Hq*D] bf16, lse [B, Hq, S] against the reference; returns the worst per-row errors (o, lse)."""
    o = o.view(B, S, Hq, D)
    live = R["live"]
    assert bool(torch.isfinite(o.float()).all()), f"{tag}: non-finite o"
    assert bool((~torch.isnan(lse)).all()) and bool((lse != -math.inf).all()), f"{tag}: NaN / -inf lse"
    # rows with no visible key: o exactly 0, lse +inf
    dead = ~live
    if bool(dead.any()):
        assert bool((o[dead] == 0).all()), f"{tag}: a row with no visible key has o != 0"
        assert bool((lse.permute(0, 2, 1)[dead] == math.inf).all()), f"{tag}: a row with no visible key has lse != +inf"
    assert bool(torch.isfinite(lse.permute(0, 2, 1)[live]).all()), f"{tag}: a live row has a non-finite lse"
    dl = delta(R["mag"], D, k_op)
    eo = row_rel(o[live], R["o"][live], R["o_scale"][live].clamp_min(1e-300))
    bo = BOUND_O(dl[live])
    el = (lse.permute(0, 2, 1)[live].double() - R["lse"].permute(0, 2, 1)[live]).abs()
    bl = BOUND_LSE(dl[live])
    i, j = int(torch.argmax(eo / bo)), int(torch.argmax(el / bl))
    _record((tag, "o"), eo[i], bo[i])
    _record((tag, "lse"), el[j], bl[j])
    assert bool((eo <= bo).all()), f"{tag}: o row error {float(eo[i]):.3e} > bound {float(bo[i]):.3e}"
    assert bool((el <= bl).all()), f"{tag}: lse error {float(el[j]):.3e} > bound {float(bl[j]):.3e} (log2)"
    return float(eo.max()), float(el.max())


def check_backward(d, R, mask, B, S, Hq, Hkv, D, k_op, tag):
    """d_qkv [B*S, (Hq + 2 Hkv) D]; returns the worst per-row errors of dq, dk, dv."""
    assert bool(torch.isfinite(d.float()).all()), f"{tag}: non-finite gradient"
    x = d.view(B, S, Hq + 2 * Hkv, D)
    dq, dk, dv = x[:, :, :Hq], x[:, :, Hq:Hq + Hkv], x[:, :, Hq + Hkv:]
    dead = ~R["live"]
    if bool(dead.any()):
        assert bool((dq[dead] == 0).all()), f"{tag}: a row with no visible key has dq != 0"
    unseen = (mask == 0)[:, :, None].expand(B, S, Hkv)                 # keys no query sees
    if bool(unseen.any()):
        assert bool((dk[unseen] == 0).all()) and bool((dv[unseen] == 0).all()), f"{tag}: a masked key has a nonzero dk / dv"
    dq_dl = delta(R["mag"], D, k_op)
    dkv_dl = delta(R["mag_k"], D, k_op)                                # a key: the worst of the rows that see it
    worst = []
    for name, got, ref, dl in (("dq", dq, R["dq"], dq_dl), ("dk", dk, R["dk"], dkv_dl), ("dv", dv, R["dv"], dkv_dl)):
        e = row_rel(got, ref, R["a_" + name].clamp_min(1e-300))
        bnd = BOUND_GRAD(dl)
        i = int(torch.argmax((e / bnd).reshape(-1)))
        _record((tag, name), e.reshape(-1)[i], bnd.reshape(-1)[i])
        assert bool((e <= bnd).all()), f"{tag}: {name} row error {float(e.reshape(-1)[i]):.3e} > bound {float(bnd.reshape(-1)[i]):.3e}"
        worst.append(float(e.max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# fused attention: the cases
# ---------------------------------------------------------------------------------------------------------------------
# (B, S, Hq, Hkv, family, mask).  Head_dim 64: every S of the issue's list, G in {1, 2, 3, 4, 6, 8, 16}.
D64_CASES = [
    (2, 1, 2, 2, "gauss", "rowpad"),
    (2, 2, 4, 2, "sink-last", "rowpad"),
    (2, 63, 3, 1, "peaked", "hole"),
    (1, 64, 4, 1, "sink-first", "none"),
    (2, 65, 8, 1, "sink-last", "left63"),
    (1, 127, 16, 1, "flat", "alternate"),
    (2, 128, 6, 1, "big-v", "left64"),
    (2, 129, 4, 2, "rising", "left65"),
    (2, 1000, 8, 2, "peaked", "left128"),
    (2, 1000, 4, 1, "gauss", "trailing"),
    (2, 1000, 8, 1, "rising", "half"),
    (2, 1000, 3, 1, "rising-big", "none"),
    (1, 4095, 2, 2, "peaked", "lefthalf"),
    (1, 4096, 8, 1, "rising", "tilehole"),
    (1, 4097, 3, 1, "sink-first", "hole"),
    (1, 4160, 16, 1, "peaked", "alternate"),
    (1, 6000, 4, 2, "peaked", "tilehole"),
    (1, 6000, 2, 1, "flat", "trailing"),
    (1, 6000, 8, 1, "rising", "tilehole"),
    (1, 28608, 1, 1, "peaked", "tilehole"),
    (1, 28608, 2, 1, "sink-first", "alternate"),
]
D128_CASES = [
    (2, 1, 4, 1, "gauss", "rowpad"),
    (1, 64, 4, 1, "sink-first", "hole"),
    (2, 129, 8, 1, "peaked", "alternate"),
    (1, 1000, 4, 1, "rising", "left65"),
    (2, 2048, 8, 1, "big-v", "rowpad"),
    (1, 4160, 4, 1, "peaked", "tilehole"),
    (1, 4160, 1, 1, "flat", "trailing"),
    (1, 4160, 8, 1, "sink-last", "half"),
]
D256_CASES = [
    (2, 1, 2, 2, "gauss", "rowpad"),
    (2, 63, 2, 1, "sink-last", "hole"),
    (1, 64, 8, 1, "peaked", "none"),
    (2, 65, 1, 1, "flat", "left64"),
    (2, 129, 2, 1, "big-v", "alternate"),
    (1, 449, 8, 1, "rising", "left65"),
    (2, 1000, 2, 1, "sink-first", "trailing"),
    (1, 2048, 8, 1, "peaked", "half"),
    (1, 4096, 2, 2, "rising-big", "tilehole"),
    (1, 6000, 8, 1, "peaked", "tilehole"),
    (1, 8128, 2, 1, "sink-last", "tilehole"),                          # the longest the LDS-DMA forms take (8 192 runs register-staged)
    (1, 8192, 2, 1, "peaked", "lefthalf"),
    (1, 8192, 1, 1, "sink-first", "hole"),
]

# forms: name -> (head_dim, staging mode, lean waves, d256 pass_p, score operands of (forward, dQ, dK / dV): attn_ref_fp64's ops_)
EX3, LEAN3 = ("exact",) * 3, ("lean",) * 3
FORMS = {
    "lean": (64, 2, 4, False, LEAN3),
    "lean-w8": (64, 2, 8, False, LEAN3),
    "round2": (64, 1, 4, False, EX3),
    "regs": (64, 0, 4, False, EX3),
    "mix-0x100": (64, 2 | 0x100, 4, False, ("exact", "lean", "lean")),  # forward on mode 1, dQ and dK / dV lean
    "mix-0x200": (64, 2 | 0x200, 4, False, ("lean", "exact", "lean")),  # dQ on mode 1
    "mix-0x400": (64, 2 | 0x400, 4, False, ("lean", "lean", "exact")),  # dK / dV on mode 1
    "d128": (128, 2, 4, False, EX3),
    "d256": (256, 2, 4, False, EX3),
    "d256-pass-p": (256, 2, 4, True, EX3),
    "d256-regs": (256, 0, 4, False, EX3),
}
FORMS_OF = {64: ["round2", "regs", "lean", "lean-w8", "mix-0x100", "mix-0x200", "mix-0x400"], 128: ["d128"], 256: ["d256", "d256-pass-p", "d256-regs"]}
ADVERSARIAL = {64: (1, 4096, 8, 1, "rising", "tilehole"), 128: (2, 129, 8, 1, "peaked", "alternate"), 256: (1, 4096, 2, 2, "rising-big", "tilehole")}


def _set_form(ops, form):
    _, mode, waves, pass_p, _ = FORMS[form]
    ops.set_attn_fwd_staging(mode)
    ops.set_attn_lean_waves(waves)
    ops.set_attn_d256_pass_p(pass_p)


def _restore(ops):
    ops.set_attn_fwd_staging(2)
    ops.set_attn_lean_waves(4)
    ops.set_attn_d256_pass_p(False)


def _cases(D, cases):
    return [pytest.param(D, *c, id=f"d{D}-B{c[0]}-S{c[1]}-G{c[2] // c[3]}x{c[3]}-{c[4]}-{c[5]}") for c in cases]


@pytest.mark.parametrize("D,B,S,Hq,Hkv,family,mask_name", _cases(64, D64_CASES) + _cases(128, D128_CASES) + _cases(256, D256_CASES))
def test_fused_attention_against_float64(ops, request, D, B, S, Hq, Hkv, family, mask_name):
    """ecgb_attn_fwd / ecgb_attn_bwd in every form of the head dim, row by row (module docstring), against the float64 reference of the form's
    own score operands with the tight bounds (k_op = 0), and -- lean forms -- against the operation itself with the pre-scale term (k_op = 1)
    and at the gauss / flat / big-v families within 1.5x of the round-2 kernels' error; rows with no visible key give o = 0, lse = +inf,
    dq = 0; masked keys get dk = dv = 0."""
    scale = 1.0 / math.sqrt(D)
    seed = 1000 + 7 * S + D + Hq
    qkv, do = make_inputs(family, B, S, Hq, Hkv, D, seed)
    mask = make_mask(mask_name, B, S)
    R = attn_ref_fp64(qkv, do, mask, B, S, Hq, Hkv, D, scale)
    if family == "peaked" and S >= 64:
        assert R["smax"] >= 40 and R["smin"] <= -40, (R["smin"], R["smax"])
    if family == "flat":                                               # the reference itself: lse = log2(keys visible to the row)
        nvis = torch.cumsum((mask != 0).double(), 1)
        want = torch.where(nvis > 0, torch.log2(nvis.clamp_min(1)), torch.full_like(nvis, math.inf))
        got = R["lse"][:, 0]
        assert torch.equal(torch.isinf(got), torch.isinf(want)) and bool(((got - want)[~torch.isinf(want)].abs() < 1e-9).all())
    tid = request.node.callspec.id
    refs = {EX3: R}
    round2 = None
    try:
        for form in FORMS_OF[D]:
            ops_ = FORMS[form][4]
            if ops_ not in refs:
                refs[ops_] = attn_ref_fp64(qkv, do, mask, B, S, Hq, Hkv, D, scale, ops_)
            _set_form(ops, form)
            o, lse = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, scale)
            check_forward(o, lse, refs[ops_], B, S, Hq, D, 0, f"{tid}/{form}")
            d = ops.attn_bwd(qkv, mask, o, do, lse, B, S, Hq, Hkv, D, scale)
            check_backward(d, refs[ops_], mask, B, S, Hq, Hkv, D, 0, f"{tid}/{form}")
            if ops_ != EX3:                                            # the distance from the operation itself: the pre-scale term
                check_forward(o, lse, R, B, S, Hq, D, int(ops_[0] == "lean"), f"{tid}/{form}/vs-op")
                check_backward(d, R, mask, B, S, Hq, Hkv, D, 1, f"{tid}/{form}/vs-op")
            x = d.view(B, S, Hq + 2 * Hkv, D)
            whole = [whole_rel(o.view(B, S, Hq, D), R["o"], R["o_scale"])] + \
                    [whole_rel(g, R[n], R["a_" + n]) for g, n in ((x[:, :, :Hq], "dq"), (x[:, :, Hq:Hq + Hkv], "dk"), (x[:, :, Hq + Hkv:], "dv"))]
            if form == "round2":
                round2 = whole
            elif D == 64 and form != "regs":
                a, c = LEAN_VS_ROUND2
                for name, e, e2 in zip(("o", "dq", "dk", "dv"), whole, round2):
                    _record((f"{tid}/{form}", name + "-vs-round2"), e, a * e2 + c)
                    if family in LEAN_TIGHT_FAMILIES:
                        assert e <= a * e2 + c, (form, name, e, e2)
            if (B, S, Hq, Hkv, family, mask_name) == ADVERSARIAL[D]:
                o2, lse2 = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, scale)
                assert torch.equal(o, o2) and torch.equal(lse, lse2), form
                assert torch.equal(d, ops.attn_bwd(qkv, mask, o, do, lse, B, S, Hq, Hkv, D, scale)), form
    finally:
        _restore(ops)


@pytest.mark.parametrize("D,S", [(64, 28608), (128, 24576), (256, 8192)])
def test_first_refused_length_raises(ops, D, S):
    """check_args takes up to 28 608 keys at head_dim 64, 24 576 at 128 and 8 192 at 256 (the row's key mask beside the tile buffers in LDS,
    at 64 also the lean kernels' tile flags); one key more is ECGB_ERR_UNSUPPORTED before any launch, forward and backward, in every form."""
    from ecg_byte_amd import _lib
    Hq = Hkv = 1
    try:
        for form in FORMS_OF[D]:
            _set_form(ops, form)
            for n, ok in ((S, True), (S + 1, False)):
                qkv = torch.zeros(n, 3 * D, dtype=torch.bfloat16, device="cuda")
                mask = torch.ones(1, n, device="cuda")
                z, lse0 = torch.zeros(n, D, dtype=torch.bfloat16, device="cuda"), torch.zeros(1, 1, n, device="cuda")
                if ok:
                    o, lse = ops.attn_fwd(qkv, mask, 1, n, Hq, Hkv, D, 0.125)
                    d = ops.attn_bwd(qkv, mask, o, z, lse, 1, n, Hq, Hkv, D, 0.125)
                    torch.cuda.synchronize()
                    assert float(lse[0, 0, -1]) == pytest.approx(math.log2(n), abs=1e-3), form     # q = 0: lse = log2(visible keys)
                    assert bool((d == 0).all()), form
                else:
                    for call in (lambda: ops.attn_fwd(qkv, mask, 1, n, Hq, Hkv, D, 0.125),
                                 lambda: ops.attn_bwd(qkv, mask, z, z, lse0, 1, n, Hq, Hkv, D, 0.125)):
                        with pytest.raises(_lib.EcgbError) as ei:
                            call()
                        assert ei.value.code == -3, form
    finally:
        _restore(ops)


# ---------------------------------------------------------------------------------------------------------------------
# attn_probs
# ---------------------------------------------------------------------------------------------------------------------
PROBS_CASES = [  # (D, B, S, Hq, Hkv, family, mask, lse form)
    (64, 2, 300, 4, 1, "peaked", "hole", "lean"),
    (64, 2, 300, 4, 1, "peaked", "hole", "round2"),
    (64, 2, 1000, 8, 2, "sink-first", "rowpad", "lean"),
    (64, 1, 700, 2, 2, "peaked", "alternate", "lean"),
    (64, 2, 200, 2, 1, "gauss", "left65", "lean"),
    (64, 2, 1000, 4, 1, "rising", "hole", "lean"),
    (64, 1, 4096, 2, 1, "rising", "tilehole", "lean"),
    (128, 2, 257, 4, 1, "peaked", "alternate", "d128"),
    (256, 2, 300, 2, 1, "peaked", "rowpad", "d256"),
    (256, 1, 600, 8, 1, "sink-last", "hole", "d256"),
]


@pytest.mark.parametrize("D,B,S,Hq,Hkv,family,mask_name,form", PROBS_CASES, ids=[f"d{c[0]}-S{c[2]}-{c[5]}-{c[6]}-{c[7]}" for c in PROBS_CASES])
def test_attn_probs_against_float64(ops, request, D, B, S, Hq, Hkv, family, mask_name, form):
    """ecgb_attn_probs (full and sum forms) after the forward a model runs (at head_dim 64 the DEFAULT lean forward), with the lse
    decoder_ops.probs_lse hands over for it, as HipCausalLM does: every probability within 1e-2 absolute of the float64 softmax and within
    2u of it (its bf16 rounding, the fp32 work of both kernels) plus the scores' fp32 error; each row of either form sums to 1 within the
    sum of those bounds; hidden keys exactly 0; rows with no visible key bf16(1/S).  (The lean forward's own lse is not one of the exact
    scores attn_probs forms: at peaked scores it gave probabilities off by 0.1, at rising ones by factors.)"""
    scale = 1.0 / math.sqrt(D)
    qkv, _ = make_inputs(family, B, S, Hq, Hkv, D, 500 + S + D)
    mask = make_mask(mask_name, B, S)
    try:
        _set_form(ops, form)
        _, lse = ops.attn_fwd(qkv, mask, B, S, Hq, Hkv, D, scale)
        lse = ops.probs_lse(qkv, mask, lse, B, S, Hq, Hkv, D, scale)
    finally:
        _restore(ops)
    probs = torch.empty((B, Hq, S, S), dtype=torch.bfloat16, device="cuda")
    psum = torch.empty((B, S, S), dtype=torch.float32, device="cuda")
    ops.attn_probs(qkv, mask, lse, B, S, Hq, Hkv, D, scale, probs=probs, psum=psum, weight=1.0)
    torch.cuda.synchronize()
    x = qkv.view(B, S, Hq + 2 * Hkv, D).double()
    tid = request.node.callspec.id
    worst_abs, worst_sum, srel = 0.0, 0.0, 0.0
    for b in range(B):
        q = x[b, :, :Hq].transpose(0, 1)
        k = x[b, :, Hq:Hq + Hkv].transpose(0, 1).repeat_interleave(Hq // Hkv, 0)
        s = q @ k.transpose(1, 2) * scale
        vis = torch.tril(torch.ones(S, S, dtype=torch.bool, device="cuda")) & (mask[b] != 0)[None, :]
        empty = ~vis.any(1)
        ref = torch.softmax(s.masked_fill(~vis, -math.inf).masked_fill(empty[:, None], 0.0), -1)
        ref[:, empty] = 1.0 / S
        mag = ((q.abs() @ k.abs().transpose(1, 2)) * scale * LOG2E).masked_fill(~vis, 0.0).amax(2)       # [Hq, S]
        dl = delta(mag, D, 0)                                          # the fp32 scores of the forward's lse and of the probs kernel
        # |p - p_ref| <= p_ref (u + (2^(|d lse| + |d s|) - 1)) + u p_ref for the fp32 work of both kernels (exp2 approximations, the order of
        # the MFMA sums, the lse's row sum), above the flush of exp2 at 2^-126
        rel = (2 * U + EXPM1(2 * dl))[:, :, None]
        got = probs[b].double()
        full = (vis & ~empty[:, None])[None].expand_as(ref)
        err = (got - ref).abs()
        worst_abs = max(worst_abs, float(err[full].max()) if bool(full.any()) else 0.0)
        assert bool((err[full] <= PROBS_ABS).all()), f"{tid}: probability off by {float(err[full].max()):.3e} > {PROBS_ABS}"
        bound = (ref * rel + TINY).expand_as(ref)
        assert bool((err[full] <= bound[full]).all()), f"{tid}: worst {float((err[full] / bound[full]).max()):.2f} x the bound"
        assert bool((got[(~vis & ~empty[:, None])[None].expand_as(got)] == 0).all()), f"{tid}: a hidden key is nonzero"
        if bool(empty.any()):
            assert bool((got[:, empty] == torch.tensor(1.0 / S, dtype=torch.bfloat16).double().item()).all())
        rowsum = psum[b].double() / Hq
        want_sum = ref.sum(0) / Hq
        es = (rowsum - want_sum).abs()
        assert bool((es <= want_sum * (rel.amax(0)) + 1e-6).all()), f"{tid}: sum form off by {float(es.max()):.3e}"
        live = ~empty
        if not bool(live.any()):
            continue
        bsum = torch.where(full, bound, torch.zeros_like(bound)).sum(-1)[:, live]      # |sum_j p_ij - 1| <= sum_j (the bound of p_ij)
        esum = (got.sum(-1)[:, live] - 1).abs()
        fsum = (psum[b].double().sum(-1)[live] / Hq - 1).abs()
        worst_sum = max(worst_sum, float(esum.max()), float(fsum.max()))
        srel = max(srel, float(bsum.max()))
        assert bool((esum <= bsum).all()), f"{tid}: a row of the full form sums to 1 within {float(esum.max()):.3e} only"
        assert bool((fsum <= bsum.mean(0)).all()), f"{tid}: a row of the sum form sums to 1 within {float(fsum.max()):.3e} only"
    _record((tid, "probs-abs"), worst_abs, PROBS_ABS)
    _record((tid, "rowsum-1"), worst_sum, srel)


# ---------------------------------------------------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------------------------------------------------
def _decode_inputs(family, B, cap, n, Hq, Hkv, D, seed):
    g = _gen(seed)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda", generator=g)
    cache = torch.randn(B, cap, 2 * Hkv * D, device="cuda", generator=g)
    if family == "peaked":
        qkv[:, : Hq * D] *= 3.5
        cache[:, :, : Hkv * D] *= 3.5
    else:                                                              # sink-first / sink-last: one key 25 nats above the rest
        qkv[:, : Hq * D] *= 0.5
        cache[:, :, : Hkv * D] *= 0.5
        j = 0 if family == "sink-first" else n - 1
        c = 25.0 * math.sqrt(D)
        qv = qkv[:, : Hq * D].view(B, Hq, D)
        qv[:, :, :2] = 1.0
        kc = cache[:, :, : Hkv * D].view(B, cap, Hkv, D)
        kc[:, :, :, :2] = 0.0
        hi = _pow2_at_least(c)
        kc[:, j, :, 0], kc[:, j, :, 1] = hi, c - hi
    return qkv.to(torch.bfloat16), cache.to(torch.bfloat16)


def _decode_ref(q, cache, mask, n, Hq, Hkv, D, scale, k_op):
    """q [B, Hq, D] float64 (already rotated where the kernel rotates); returns o [B, Hq, D], || P |V| || [B, Hq], delta [B, Hq]."""
    B = q.shape[0]
    G = Hq // Hkv
    k = cache[:, :n, : Hkv * D].double().view(B, n, Hkv, D).repeat_interleave(G, 2)
    v = cache[:, :n, Hkv * D:].double().view(B, n, Hkv, D).repeat_interleave(G, 2)
    s = torch.einsum("bhd,bnhd->bhn", q, k) * scale
    vis = (mask[:, None, :n] != 0)
    s = s.masked_fill(~vis, -math.inf)
    p = torch.softmax(s, -1)
    o = torch.einsum("bhn,bnhd->bhd", p, v)
    osc = torch.einsum("bhn,bnhd->bhd", p, v.abs()).norm(dim=-1)
    mag = (torch.einsum("bhd,bnhd->bhn", q.abs(), k.abs()) * scale * LOG2E).masked_fill(~vis, 0.0).amax(-1)
    return o, osc, (k_op * U + D * FP32) * mag


DECODE_CASES = [  # (D, B, Hq, Hkv, n, cap, family, mask)
    (64, 2, 4, 1, 1, 64, "peaked", "none"),
    (64, 1, 8, 1, 2, 64, "sink-last", "none"),
    (64, 2, 8, 8, 63, 128, "peaked", "hole"),
    (64, 1, 4, 1, 64, 128, "sink-first", "alternate"),
    (64, 2, 8, 1, 65, 128, "sink-last", "hole"),
    (64, 1, 32, 8, 511, 640, "peaked", "hole"),
    (64, 1, 32, 8, 512, 640, "sink-first", "split"),
    (64, 1, 8, 1, 2048, 2048, "peaked", "split"),
    (64, 1, 8, 2, 2049, 2176, "sink-last", "hole"),
    (128, 2, 4, 1, 63, 64, "peaked", "hole"),
    (128, 1, 8, 1, 700, 768, "sink-first", "split"),
    (128, 2, 4, 4, 1301, 1408, "peaked", "alternate"),
    (256, 1, 8, 1, 1, 64, "sink-first", "none"),
    (256, 1, 8, 1, 65, 128, "peaked", "hole"),
    (256, 1, 8, 1, 729, 768, "sink-last", "split"),
    (256, 2, 4, 1, 1024, 1024, "peaked", "alternate"),
]


def _decode_mask(name, B, cap, n, ns):
    m = torch.ones(B, cap, device="cuda")
    m[:, n:] = 0
    if name == "hole":
        m[:, n // 2] = 0
        m[0, : min(3, n - 1)] = 0
    elif name == "alternate":
        m[:, : n - 1: 2] = 0                                           # (the newest key stays visible)
    elif name == "split":                                              # every key of the second split masked
        chunk = -(-n // ns)
        m[:, chunk: min(2 * chunk, n - 1)] = 0
    return m


@pytest.mark.parametrize("D,B,Hq,Hkv,n,cap,family,mask_name", DECODE_CASES, ids=[f"d{c[0]}-B{c[1]}-G{c[2] // c[3]}x{c[3]}-n{c[4]}-{c[6]}-{c[7]}" for c in DECODE_CASES])
def test_decode_attention_against_float64(ops, request, D, B, Hq, Hkv, n, cap, family, mask_name):
    """attn_decode, attn_decode_split (host and device length) and attn_decode_one (RoPE + append + attention; the same RoPE in the reference)
    against float64 per (sequence, head), with the forward's o bound; lengths where decode_splits changes; a split whose keys are all masked."""
    scale = 1.0 / math.sqrt(D)
    ns_default = ops.decode_splits(cap, B, Hq)
    ns = max(2, min(ns_default if ns_default > 1 else 4, n))
    qkv, cache = _decode_inputs(family, B, cap, n, Hq, Hkv, D, 900 + n + D)
    mask = _decode_mask(mask_name, B, cap, n, ns)
    q = qkv[:, : Hq * D].double().view(B, Hq, D)
    o_ref, osc, dl = _decode_ref(q, cache, mask, n, Hq, Hkv, D, scale, 0)
    tid = request.node.callspec.id

    def check(got, form, ref, scale_row, dl):
        got = got.view(B, Hq, D)
        assert bool(torch.isfinite(got.float()).all()), form
        e = row_rel(got, ref, scale_row.clamp_min(1e-300))
        bnd = BOUND_O(dl)
        i = int(torch.argmax((e / bnd).reshape(-1)))
        _record((tid, form), e.reshape(-1)[i], bnd.reshape(-1)[i])
        assert bool((e <= bnd).all()), f"{tid}/{form}: row error {float(e.reshape(-1)[i]):.3e} > {float(bnd.reshape(-1)[i]):.3e}"

    n_dev = torch.full((1,), n, dtype=torch.int32, device="cuda")
    check(ops.attn_decode(qkv, cache, mask, n, Hq, Hkv, D, scale), "single", o_ref, osc, dl)
    check(ops.attn_decode_dyn(qkv, cache, mask, n_dev, Hq, Hkv, D, scale), "single-dyn", o_ref, osc, dl)
    check(ops.attn_decode_split(qkv, cache, mask, n, Hq, Hkv, D, scale, ns), "split", o_ref, osc, dl)
    check(ops.attn_decode_split(qkv, cache, mask, n_dev, Hq, Hkv, D, scale, ns), "split-dyn", o_ref, osc, dl)
    if ops.decode_one_ok(B, Hq, D, ns, cap):
        # the new token's raw q | k | v: the kernel rotates q and k (rotate_half, fp32 tables) and writes k, v to cache row n - 1
        pos = torch.arange(B, device="cuda").double() + n - 1
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, device="cuda").double() / D))
        fr = pos[:, None] * inv[None]
        cos, sin = fr.cos().float().contiguous(), fr.sin().float().contiguous()
        c, s_ = cos.double()[:, None, :], sin.double()[:, None, :]

        def rot(t):
            t1, t2 = t[..., : D // 2], t[..., D // 2:]
            return torch.cat([t1 * c - t2 * s_, t2 * c + t1 * s_], -1)
        raw = qkv.clone()
        raw[:, Hq * D:] = cache[:, n - 1]                               # the new token's k | v: what cache row n - 1 holds before the launch
        c1 = cache.clone()
        c1[:, n - 1, : Hkv * D] = rot(raw[:, Hq * D: (Hq + Hkv) * D].double().view(B, Hkv, D)).reshape(B, Hkv * D).to(torch.bfloat16)
        # k_op 4: the rotated q and k rounded to bf16, the rotation's two products each (module docstring's delta)
        o1, osc1, dl1 = _decode_ref(rot(raw[:, : Hq * D].double().view(B, Hq, D)), c1, mask, n, Hq, Hkv, D, scale, 4)
        got = ops.attn_decode_one(raw, cos, sin, cache.clone(), mask, n, Hq, Hkv, D, scale, ns)
        check(got, "one", o1, osc1, dl1)


# ---------------------------------------------------------------------------------------------------------------------
# materialised softmax
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,mask_name", [(136, "hole"), (304, "rowpad"), (256, "alternate"), (520, "trailing")])
def test_materialised_softmax_against_float64(ops, S, mask_name):
    """ecgb_softmax_causal_fwd on peaked bf16 scores (std 12 nats after the scale) with holes and fully masked rows, and ecgb_softmax_bwd
    on its own P: per row, fp64 softmax within bf16's rounding (2u of each probability: bf16 and the fp32 work; exp flushes below 2^-126), pad rows exactly 0;
    dS = scale P (dP - rowsum(P dP)) per row within 2u of its magnitude scale || P (|dP| + rowsum(P |dP|)) || (the bf16 result; the fp32
    row sum)."""
    B, Hh, scale = 2, 3, 0.125
    g = _gen(S)
    scores = (torch.randn(B * Hh, S, S, device="cuda", generator=g) * 98.0).to(torch.bfloat16)
    mask = make_mask(mask_name, B, S)
    p = ops.softmax_causal_fwd_(scores.clone(), mask, Hh, scale)
    vis = torch.tril(torch.ones(S, S, device="cuda", dtype=torch.bool))[None] & (mask.repeat_interleave(Hh, 0)[:, None, :] != 0)
    sf = scores.double() * scale
    assert float(sf.masked_fill(~vis, 0).max()) >= 40 and float(sf.masked_fill(~vis, 0).min()) <= -40
    empty = ~vis.any(-1)
    ref = torch.softmax(sf.masked_fill(~vis, -math.inf).masked_fill(empty[..., None], 0.0), -1).masked_fill(empty[..., None], 0.0)
    err = (p.double() - ref).abs()
    assert bool((p[empty] == 0).all()) and bool((p[~vis & ~empty[..., None]] == 0).all())
    assert bool((err <= ref * 2 * U + TINY).all()), float((err / (ref * 2 * U + TINY)).max())
    dp = (torch.randn(B * Hh, S, S, device="cuda", generator=g) * 3).to(torch.bfloat16)
    pd = p.double()
    want = scale * pd * (dp.double() - (pd * dp.double()).sum(-1, keepdim=True))
    got = ops.softmax_bwd_(p, dp.clone(), scale).double()
    mag = scale * (pd * (dp.double().abs() + (pd * dp.double().abs()).sum(-1, keepdim=True))).norm(dim=-1)   # the row's magnitude
    e = (got - want).norm(dim=-1) / mag.clamp_min(1e-300)
    _record((f"softmax-S{S}-{mask_name}", "dS"), e.max(), 2 * U)
    assert bool((e <= 2 * U).all()), float(e.max())
    assert bool((got[empty] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_registers", [True, False], ids=["registers", "three-sweeps"])
@pytest.mark.parametrize("V,ld", [(50257, 50264), (132515, 132520)])
def test_cross_entropy_against_float64(ops, in_registers, V, ld):
    """ecgb_ce_fwd_bwd, both kernels, against float64: labels 30-60 nats above every other logit (loss ~ V e^-45, the label's gradient p - 1
    cancels to ~-V e^-45), the label in the last vocabulary column, all-equal logits (loss = ln V), an ignored row.  Loss within
    2^-22 (1 + |lse|) absolute (fp32 sums of the exponentials and the final subtraction); each gradient element within
    2u |g_ref| + 2^-23 * inv_count (bf16 result; p - 1 formed in fp32)."""
    g = _gen(V)
    rows = 12
    logits = torch.randn(rows, ld, device="cuda", generator=g)
    labels = torch.randint(0, V, (rows,), device="cuda", generator=g)
    labels[0] = V - 1
    labels[1] = V - 1
    for r in range(0, 8):
        logits[r, labels[r]] = logits[r, :V].max() + 30 + 4 * r
    logits[8] = 1.5                                                    # all equal
    logits[9, :V] = -3.0
    labels[10] = -100                                                  # ignored
    logits = logits.to(torch.bfloat16)
    logits[:, V:] = 0
    inv = ops.count_labels(labels, V)
    ref_logits = logits[:, :V].double()
    lse = torch.logsumexp(ref_logits, -1)
    live = labels >= 0
    tgt = ref_logits.gather(1, labels.clamp_min(0)[:, None])[:, 0]
    loss_ref = torch.where(live, lse - tgt, torch.zeros_like(lse))
    grad_ref = (torch.softmax(ref_logits, -1) - torch.nn.functional.one_hot(labels.clamp_min(0), V).double()) * float(inv)
    grad_ref[~live] = 0
    ops.set_ce_in_registers(in_registers)
    try:
        work = logits.clone()
        sum_loss = torch.zeros(1, device="cuda")
        row_loss = ops.ce_fwd_bwd_(work, labels, inv, sum_loss, V)
        torch.cuda.synchronize()
    finally:
        ops.set_ce_in_registers(True)
    el = (row_loss.double() - loss_ref).abs()
    bl = 2.0 ** -22 * (1 + lse.abs())
    _record((f"ce-V{V}-{'reg' if in_registers else 'sweep'}", "loss"), el.max(), bl.min())
    assert bool((el <= bl).all()), (el.tolist(), loss_ref.tolist())
    assert abs(float(row_loss[8]) - math.log(V)) <= 2.0 ** -20 * math.log(V)
    eg = (work[:, :V].double() - grad_ref).abs()
    bg = 2 * U * grad_ref.abs() + 2.0 ** -23 * float(inv)
    assert bool((eg <= bg).all()), float((eg / bg).max())
    assert bool((work[:, V:] == 0).all()) and bool((work[10] == 0).all())
