"""float64 numpy restatement of the IVFPQ refine stage (amdrec_ivfpq_rerank behind FAISSIndex(index_type='IVFPQ',
refine=...)): the checker given the kept rows and the candidates the code scan produced.

* refine: per query the k best candidates by sum_i (q_i - x_i)^2 in float64, ties -> lower position; candidates whose row
  is marked non-finite (or whose distance is not finite) come after every finite one at +inf, by position; unfilled
  candidates (-1) last as (+inf, -1)
* bf16_round: fp32 -> the bf16 value (round to nearest even) widened back to fp32: what a refine='bf16' index keeps
* dist_bound: how far the fp32 kernel's distance may lie from the float64 one
* check_rerank: positions equal up to swaps of near-tied neighbours / a near-tied k-th boundary, distances within the bound
* small numpy trainers (spherical k-means, per-sub-space k-means) so that the recall property can be stated without a GPU
"""
import numpy as np

from tests import ivfpq_oracle

U = 2.0 ** -24


def bf16_round(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).reshape(np.shape(x))


def dist_bound(d64, dim):
    """|d_fp32 - d_64| <= (dim + 3) u d_64 + 2^-126: one rounding in each difference (2 u relative in its square), one in each
    square, at most dim in the summation (any order), first order in u."""
    return (dim + 3) * U * np.abs(np.asarray(d64, dtype=np.float64)) + 2.0 ** -126


def distances(rows, finite, q, pos):
    """float64 distances of one query to rows[pos]; +inf where the row is non-finite or the distance is."""
    x = np.asarray(rows)[pos].astype(np.float64)
    with np.errstate(all="ignore"):
        d = ((np.asarray(q, dtype=np.float64)[None, :] - x) ** 2).sum(1)
    bad = ~np.isfinite(d)
    if finite is not None:
        bad |= ~np.asarray(finite, dtype=bool)[pos]
    return np.where(bad, np.inf, d)


def refine(rows, finite, xq, cand_pos, k):
    cand_pos = np.asarray(cand_pos)
    nq = cand_pos.shape[0]
    D = np.full((nq, k), np.inf)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        pos = cand_pos[q][cand_pos[q] >= 0]
        if pos.size == 0:
            continue
        d = distances(rows, finite, xq[q], pos)
        order = np.lexsort((pos, d))[:k]                 # +inf sorts after every finite distance, then by position
        D[q, :order.size] = d[order]
        I[q, :order.size] = pos[order]
    return D, I


def check_rerank(rows, finite, xq, cand_pos, k, got_pos, got_dist, dim):
    """The kernel's (positions, distances) against the float64 re-rank of the same candidates.  A slot may differ from the
    oracle's only as one of two rank neighbours, or the k-th slot and an outside candidate, whose float64 distances differ
    by less than dist_bound (of the larger of the two).  -> (excused slots, all slots, largest err / bound)."""
    cand_pos, got_pos, got_dist = np.asarray(cand_pos), np.asarray(got_pos), np.asarray(got_dist)
    kc = cand_pos.shape[1]
    fD, fI = refine(rows, finite, xq, cand_pos, kc)      # the full order of the candidates
    excused, worst = 0, 0.0
    for q in range(cand_pos.shape[0]):
        rD, rI, gI, gD = fD[q, :k], fI[q, :k], got_pos[q], got_dist[q].astype(np.float64)
        d_of = dict(zip(fI[q].tolist(), fD[q].tolist()))
        assert np.array_equal(np.isfinite(gD), np.isfinite(rD)), q
        assert ((gI >= 0) == (rI >= 0)).all(), q
        assert (gD[~np.isfinite(gD)] > 0).all()
        g64 = np.array([d_of.get(p, np.inf) if p >= 0 else np.inf for p in gI.tolist()])   # float64 distance of what it returned
        assert all(p in d_of for p in gI[gI >= 0].tolist()), q                              # only candidates come back
        fin = np.isfinite(rD)
        err = np.abs(gD[fin] - g64[fin])
        bound = dist_bound(g64[fin], dim)
        assert (err <= bound).all(), (q, float((err / bound).max()))
        if fin.any():
            worst = max(worst, float((err / bound).max()))
            assert (np.diff(gD[fin]) >= 0).all(), q
        i = 0
        while i < k:
            if gI[i] == rI[i]:
                i += 1
                continue
            tie = lambda a, b: abs(a - b) < float(dist_bound(max(a, b), dim))   # noqa: E731
            if i + 1 < k and gI[i] == rI[i + 1] and gI[i + 1] == rI[i] and tie(rD[i], rD[i + 1]):
                excused += 2
                i += 2
            elif i == k - 1 and gI[i] >= 0 and np.isfinite(rD[i]) and tie(d_of[int(gI[i])], rD[i]):
                excused += 1
                i += 1
            else:
                raise AssertionError(f"query {q} slot {i}: position {gI[i]} (d64 {g64[i]!r}) where the oracle has {rI[i]} "
                                     f"(d64 {rD[i]!r})")
    return excused, cand_pos.shape[0] * k, worst


def perturbed_order(fD, fI, k, scale, dim, rng):
    """The k best of each query's fully ordered candidates (refine(..., k = kc)) after every finite float64 distance has
    moved by a uniform draw from +-scale x dist_bound: what a kernel whose error is that share of the bound may return.
    -> (positions [nq, k], perturbed distances [nq, k])."""
    fin = np.isfinite(fD)
    P = np.where(fin, fD + rng.uniform(-scale, scale, fD.shape) * dist_bound(np.where(fin, fD, 0.0), dim), np.inf)
    gI = np.empty((fD.shape[0], k), np.int64)
    gD = np.empty((fD.shape[0], k))
    for q in range(fD.shape[0]):
        o = np.lexsort((fI[q], P[q]))[:k]
        gI[q], gD[q] = fI[q][o], P[q][o]
    return gI, gD


def order_differences(fD, fI, gI, k, dim):
    """Slots of gI that differ from the oracle's order, split by the rule of check_rerank.
    -> (slots excused as near-tie neighbour swaps / k-th boundary, slots the rule refuses, largest |d64 of the returned
    candidate - d64 of the oracle's candidate| / dist_bound over all differing slots)."""
    excused = refused = 0
    worst = 0.0
    for q in range(fD.shape[0]):
        d_of = dict(zip(fI[q].tolist(), fD[q].tolist()))
        rD, rI = fD[q, :k], fI[q, :k]
        tie = lambda a, b: abs(a - b) < float(dist_bound(max(a, b), dim))   # noqa: E731
        i = 0
        while i < k:
            if gI[q, i] == rI[i]:
                i += 1
                continue
            worst = max(worst, abs(d_of[int(gI[q, i])] - rD[i]) / float(dist_bound(rD[i], dim)))
            if i + 1 < k and gI[q, i] == rI[i + 1] and gI[q, i + 1] == rI[i] and tie(rD[i], rD[i + 1]):
                excused += 2
                i += 2
            elif i == k - 1 and tie(d_of[int(gI[q, i])], rD[i]):
                excused += 1
                i += 1
            else:
                refused += 1
                i += 1
    return excused, refused, worst


# ---- numpy trainers for the CPU statement of the recall property --------------------------------------------------------
def _lloyd(x, k, niter, rng, spherical):
    c = x[rng.choice(x.shape[0], k, replace=False)].copy()
    for _ in range(niter):
        if spherical:
            a = (x @ c.T).argmax(1)
        else:
            a = ((x * x).sum(1)[:, None] - 2 * x @ c.T + (c * c).sum(1)[None, :]).argmin(1)
        for j in np.unique(a):
            mu = x[a == j].mean(0)
            c[j] = mu / max(np.linalg.norm(mu), 1e-30) if spherical else mu
    return c


def train_state(xb, nlist, m, seed=0, niter=6, pq_train=8192):
    """-> (centroids, assign, codebooks, codes): a small float64 IVFPQ build (max-inner-product coarse quantizer, L2 product
    quantizer of the residuals), codes from ivfpq_oracle.encode."""
    rng = np.random.default_rng(seed)
    x = np.asarray(xb, dtype=np.float64)
    cent = _lloyd(x, nlist, niter, rng, True)
    assign = (x @ cent.T).argmax(1)
    res = x - cent[assign]
    d = x.shape[1]
    dsub = d // m
    sample = res[rng.choice(x.shape[0], min(pq_train, x.shape[0]), replace=False)]
    cb = np.stack([_lloyd(sample[:, s * dsub:(s + 1) * dsub], 256, niter, rng, False) for s in range(m)])
    return cent, assign, cb, ivfpq_oracle.encode(x, assign, cent, cb)


def recall(ids, truth):
    k = truth.shape[1]
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(ids, truth)]))
