"""Numpy restatement of the on-device sampler (csrc/sample.hip) for the sampling tests: Philox4x32-10, the uniform of
(seed, step, row), and the reference's sampling rules (base.py:214-252) in float64 with an explicit tie order."""
import numpy as np

PLAIN, TOPK, TOPP, GUMBEL = 0, 1, 2, 3
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: (..., 4) uint32-valued, key: (..., 2) -> (..., 4) uint64 arrays holding the 32-bit output words."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i] for i in range(4)]
    k0 = np.asarray(key, dtype=np.uint64)[..., 0].copy()
    k1 = np.asarray(key, dtype=np.uint64)[..., 1].copy()
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & np.uint64(_MASK), (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & np.uint64(_MASK)]
        k0 = (k0 + np.uint64(_W0)) & np.uint64(_MASK)
        k1 = (k1 + np.uint64(_W1)) & np.uint64(_MASK)
    return np.stack(c, axis=-1)


def uniform(seed, step, rows):
    """u in (0, 1] of rows `rows` (array) at `step`: counter (step, row, 0, 0), key (seed lo, seed hi)."""
    rows = np.asarray(rows, dtype=np.uint64)
    z = np.zeros_like(rows)
    ctr = np.stack([np.full_like(rows, step), rows, z, z], axis=-1)
    key = np.stack([np.full_like(rows, seed & _MASK), np.full_like(rows, (seed >> 32) & _MASK)], axis=-1)
    x0 = philox4x32_10(ctr, key)[..., 0]
    return (((x0 >> np.uint64(8)) + np.uint64(1)).astype(np.float64)) * 2.0 ** -24


def rank_order(x):
    """Indices of x by value descending, the lower index first among equal values."""
    return np.lexsort((np.arange(x.shape[0]), -x))


def distribution(logit, method, k=0, p=0.0, temp=1.0, set_tol=0.0):
    """One row: (weights w (float64, 0 outside the kept set), stored value per word, kept-set ambiguous flag).
    The word is drawn with probability w / sum(w); stored[w] is the sampled_logprob the reference keeps."""
    x = np.asarray(logit, dtype=np.float64)
    m = x.max()
    lse = np.log(np.exp(x - m).sum())
    lp = x - m - lse
    amb = False
    if method == PLAIN:
        return np.exp((x - m) / temp), lp / temp, amb
    if method == GUMBEL:
        return np.exp(x - m), lp, amb
    order = rank_order(x)
    kept = np.zeros(x.shape[0], dtype=bool)
    if method == TOPK:
        kept[order[:k]] = True
        return np.where(kept, np.exp((x - m) / temp), 0.0), lp / temp, amb
    q = np.exp(x - m)
    q = q / q.sum()
    c = np.cumsum(q[order])
    keep_sorted = np.concatenate([[True], c[:-1] < p])
    kept[order[keep_sorted]] = True
    if set_tol > 0:
        amb = bool(np.min(np.abs(c[:-1] - p)) < set_tol)
    w = np.where(kept, q, 0.0)
    with np.errstate(divide="ignore"):
        stored = np.log(w / w.sum())
    return w, stored, amb


def draw(w, u, tol):
    """Inverse CDF in index order: the first i with cumsum(w)[i] >= u * sum(w).  Returns (word, acceptable words): when
    u * total lies within tol * total of a CDF boundary the neighbouring kept word across it is acceptable too."""
    cdf = np.cumsum(w)
    total = cdf[-1]
    goal = u * total
    i = int(np.searchsorted(cdf, goal, side="left"))
    i = min(i, w.shape[0] - 1)
    ok = {i}
    nz = np.flatnonzero(w > 0)
    pos = int(np.searchsorted(nz, i))
    if pos > 0 and abs(cdf[nz[pos - 1]] - goal) < tol * total:   # near the lower edge of i's interval
        ok.add(int(nz[pos - 1]))
    if pos + 1 < nz.shape[0] and abs(cdf[i] - goal) < tol * total:   # near the upper edge
        ok.add(int(nz[pos + 1]))
    return i, ok


def sample_rows(logits, method, k=0, p=0.0, temp=1.0, seed=0, step=0, rows=None, tol=1e-6):
    """The sampler on rows of logits: (words, stored logprobs, acceptable-word sets, ambiguous flags).  rows: the row
    indices of the Philox counter (default 0..R-1)."""
    logits = np.asarray(logits)
    R = logits.shape[0]
    rows = np.arange(R) if rows is None else np.asarray(rows)
    us = uniform(seed, step, rows)
    words, stored, oks, amb = [], [], [], []
    for r in range(R):
        w, st, set_amb = distribution(logits[r], method, k, p, temp, set_tol=tol)
        i, ok = draw(w, us[r], tol)
        if set_amb:   # the kept set itself is within rounding of changing: any word of the larger set is acceptable
            w2, _, _ = distribution(logits[r], method, k, p + tol, temp)
            ok = set(int(v) for v in np.flatnonzero(w2 > 0))
        words.append(i)
        stored.append(st[i])
        oks.append(ok)
        amb.append(len(ok) > 1)
    return np.array(words), np.array(stored), oks, np.array(amb)
