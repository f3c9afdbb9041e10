"""The sampling rule of ecgb_sample_bf16 (include/ecgbyte_decoder.h, rules 1-6) restated per token in float64 numpy: no keys, no counts, no groups -- every
drawable entry on its own, ordered by value descending then id ascending, cumulative sums, searchsorted.  Also Philox4x32-10 and the uniform the kernel makes of it."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Random123's philox4x32_10: ten rounds, the key bumped between them."""
    c, k = [int(v) & MASK for v in ctr], [int(v) & MASK for v in key]
    for r in range(10):
        if r:
            k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
    return c


def uniform(seed, nonce, row, step):
    """u of (seed, nonce, row, step): key = (seed lo, seed hi), counter = (row, step, nonce lo, nonce hi), 53 bits of out0:out1."""
    seed, nonce = int(seed) & (2 ** 64 - 1), int(nonce) & (2 ** 64 - 1)
    o = philox4x32_10([row, step, nonce & MASK, nonce >> 32], [seed & MASK, seed >> 32])
    return float(((o[0] << 32 | o[1]) >> 11) * 2.0 ** -53)


class Row:
    """One row after rules 1-4: `ids` the kept entries in order, `cum` their inclusive cumulative weights (float64), `drawable` how many entries rule 1 left,
    `margin` how far, in probability units, the nearest entry's "weight before it" is from the top-p threshold."""

    def __init__(self, x, n, temperature, top_k, top_p):
        x = np.asarray(x, dtype=np.float64)[:n].copy()
        x[x == 0] = 0.0                                                    # -0 is +0
        ids = np.nonzero(~np.isnan(x) & (x != -np.inf))[0]
        self.drawable = ids.size
        self.ids, self.cum = ids[:0], np.zeros(0)
        if ids.size == 0:
            return
        v = x[ids]
        order = np.lexsort((ids, -v))                                      # value descending, then id ascending
        ids, v = ids[order], v[order]
        if 0 < top_k < n and top_k < v.size:
            keep = v >= v[top_k - 1]                                       # ties with the k-th largest stay
            ids, v = ids[keep], v[keep]
        T = np.float64(np.float32(temperature))
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            w = np.where(v == v[0], 1.0, np.exp((v - v[0]) / T))           # (+inf on top: inf - inf never reaches the exp)
        cum = np.cumsum(w)
        before = np.concatenate([[0.0], cum[:-1]])
        keep = before < np.float64(np.float32(top_p)) * cum[-1]
        keep[0] = True
        self.margin = float(np.abs(before[1:] - np.float64(np.float32(top_p)) * cum[-1]).min() / cum[-1]) if before.size > 1 else np.inf     # of the top-p cut
        m = int(np.argmin(keep)) if not keep.all() else keep.size          # `before` never decreases: the kept entries are a prefix
        self.ids, self.cum = ids[:m], cum[:m]

    def draw(self, u):
        """(tokens, distances) for an array of u in [0, 1): the first kept entry whose inclusive cumulative weight is > u Z', clamped to the last; and |u - boundary|
        to the nearest boundary between two kept entries, in probability units (inf when one entry is kept)."""
        u = np.atleast_1d(np.asarray(u, dtype=np.float64))
        zp = self.cum[-1]
        i = np.minimum(np.searchsorted(self.cum, u * zp, side="right"), self.cum.size - 1)
        if self.cum.size == 1:
            return self.ids[i], np.full(u.shape, np.inf)
        b = self.cum[:-1] / zp
        j = np.clip(np.searchsorted(b, u), 1, b.size - 1) if b.size > 1 else np.zeros(u.shape, dtype=np.int64)
        dist = np.minimum(np.abs(u - b[j]), np.abs(u - b[np.maximum(j - 1, 0)]))
        return self.ids[i], dist


def bf16_round(x):
    """float32 values rounded to bf16 (nearest even), as float32; and their 16 bits."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint32)
    r = np.where(nan, 0x7FC0, r).astype(np.uint32)
    return (r << 16).view(np.float32), r.astype(np.uint16)
