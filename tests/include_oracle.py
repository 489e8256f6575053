"""Test-side statements of the include rule (amdrec/include.py): a slow loop restatement that the numpy oracle
``amdrec.include.merge_oracle`` is held against, and the helpers the GPU tests share - the lists they build, the expectation
from a search's own result, and the checks every combination gets.  numpy only: no GPU, no torch."""
import numpy as np

from amdrec import eligible, include


def merge_loop(r_pos, r_scores, incl_pos, n, incl_scores, ok=None):
    """The rule of amdrec/include.py, one query, entry by entry in plain Python (same arguments and result as
    ``include.merge_oracle``)."""
    k = len(r_pos)
    R = [(int(p), np.float32(s)) for p, s in zip(r_pos, r_scores) if p >= 0]
    held = {p for p, _ in R}
    V, seen = [], set()
    for i, p in enumerate(incl_pos):
        p = int(p)
        first = p not in seen
        seen.add(p)
        if not (0 <= p < n) or not first:
            continue
        if ok is not None and not ok[i]:
            continue
        if np.isnan(incl_scores[i]):
            continue
        V.append((p, np.float32(incl_scores[i])))
    listed = {p for p, _ in V}
    N = [(p, s) for p, s in V if p not in held]
    over = max(0, len(R) + len(N) - k)
    kept = list(R)
    j = len(kept) - 1
    while over:
        assert j >= 0, "I <= k: there are always enough unlisted entries"
        if kept[j][0] not in listed:
            del kept[j]
            over -= 1
        j -= 1
    merged = [(p, s, 0) for p, s in kept] + [(p, s, 1) for p, s in N]
    # score descending, ties to the lower position: insertion sort, so that nothing rests on a library's sort
    out = []
    for e in merged:
        at = len(out)
        while at > 0 and (out[at - 1][1] < e[1] or (out[at - 1][1] == e[1] and out[at - 1][0] > e[0])):
            at -= 1
        out.insert(at, e)
    pos = np.full(k, -1, dtype=np.int64)
    sc = np.full(k, -np.inf, dtype=np.float32)
    inj = np.zeros(k, dtype=np.uint8)
    for i, (p, s, f) in enumerate(out):
        pos[i], sc[i], inj[i] = p, s, f
    return pos, sc, inj


def build_lists(nq, I, n, own_rows, far_rows, r_pos, bad_rows, twins, seed):
    """[nq, I] include block by position.  Each query draws, rotated by its index so that every kind also leads a list of
    one: its own row (the query equals it), the corpus's least similar rows ``far_rows[q]``, rows of its result ``r_pos[q]``
    (the LAST filled one among them), a duplicate of an earlier entry, positions out of range, padding, the stored
    non-finite rows ``bad_rows`` and a pair of identical rows ``twins`` (a score tie at different positions); random rows
    fill what is left."""
    rng = np.random.default_rng(seed)
    blk = np.full((nq, I), -1, dtype=np.int64)
    for q in range(nq):
        filled = r_pos[q][r_pos[q] >= 0]
        pool = [int(own_rows[q]), int(far_rows[q][0])]
        if len(filled):
            pool += [int(filled[-1]), int(filled[len(filled) // 2])]
        pool += [int(far_rows[q][0]), n + 5, -1, int(bad_rows[q % len(bad_rows)]), int(twins[1]), int(twins[0]), 1 << 40,
                 int(far_rows[q][1]), int(bad_rows[(q + 1) % len(bad_rows)])]
        pool = pool[q % len(pool):] + pool[:q % len(pool)]
        pool += rng.integers(0, n, size=max(0, I - len(pool))).tolist()
        row = np.asarray(pool[:I], dtype=np.int64)
        blk[q] = row if I < 8 else row[rng.permutation(I)]
    return blk


def ref_scores(xb, q, blk, boost=None, w=None):
    """float64 truth of s_p for every list entry of ``blk`` [nq, I] (NaN for entries outside the corpus): <xb[p], q>, plus
    w * boost[p] under a boost."""
    n = len(xb)
    inside = (blk >= 0) & (blk < n)
    p = np.where(inside, blk, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.einsum("qid,qd->qi", xb[p].astype(np.float64), q.astype(np.float64))
        if boost is not None:
            s = s + np.asarray(w, dtype=np.float64)[:, None] * np.asarray(boost, dtype=np.float64)[p]
    return np.where(inside, s, np.nan)


def expect(r_pos, r_sc, blk, n, ref, out_pos, out_sc, ok=None):
    """``include.merge_oracle`` on the search's own result, row by row.  s_p of an entry is the kernel's own score where the
    output holds the position (the order is then checked on the numbers the kernel ordered by), else the float64 truth
    rounded to fp32; an entry whose truth is NaN is NaN either way, so an entry that is wrongly dropped, or wrongly kept,
    shows as a difference."""
    nq, k = r_pos.shape
    pos = np.empty((nq, k), dtype=np.int64)
    sc = np.empty((nq, k), dtype=np.float32)
    inj = np.empty((nq, k), dtype=np.uint8)
    for q in range(nq):
        at = {int(p): j for j, p in enumerate(out_pos[q]) if p >= 0}
        s = np.array([out_sc[q, at[int(p)]] if int(p) in at else np.float32(ref[q, i]) for i, p in enumerate(blk[q])],
                     dtype=np.float32)
        s[np.isnan(ref[q])] = np.nan
        pos[q], sc[q], inj[q] = include.merge_oracle(r_pos[q], r_sc[q], blk[q], n, s, None if ok is None else ok[q])
    return pos, sc, inj


def check(r_pos, r_sc, blk, n, ref, out_pos, out_sc, out_inj, tol, ok=None):
    """What every combination is held to: membership, order and flags exactly the oracle's; kept entries bit-identical to the
    search's; scores non-increasing with ties at ascending position; injected scores within ``tol`` of the truth; every
    valid entry present.  -> the oracle's flags."""
    pos, sc, inj = expect(r_pos, r_sc, blk, n, ref, out_pos, out_sc, ok)
    bad = np.argwhere(out_pos != pos)
    assert not len(bad), (bad[:5], out_pos[bad[0][0]][:12], pos[bad[0][0]][:12], blk[bad[0][0]])
    assert np.array_equal(out_inj.astype(np.uint8), inj)
    assert np.array_equal(out_sc, sc)                                   # kept entries: the search's bits; N: the kernel's own
    nq, k = out_pos.shape
    for q in range(nq):
        f = int((out_pos[q] >= 0).sum())
        assert (out_pos[q, f:] == -1).all() and np.isneginf(out_sc[q, f:]).all() and not out_inj[q, f:].any()
        s, p = out_sc[q, :f], out_pos[q, :f]
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (p[:-1] < p[1:]))).all(), q
        assert len(np.unique(p)) == f
        kept = inj[q] == 0                                              # kept entries: the search's own score bits
        assert np.array_equal(out_sc[q].view(np.uint32)[kept], sc[q].view(np.uint32)[kept])
        at = {int(x): j for j, x in enumerate(p)}
        seen = set()
        for i, x in enumerate(blk[q]):                                  # every valid entry is in the output
            x = int(x)
            valid = 0 <= x < n and x not in seen and not np.isnan(ref[q, i]) and (ok is None or ok[q, i])
            seen.add(x)
            if valid:
                assert x in at, (q, x)
                if out_inj[q, at[x]] and np.isfinite(ref[q, i]):
                    assert abs(float(out_sc[q, at[x]]) - ref[q, i]) <= tol, (q, x, out_sc[q, at[x]], ref[q, i])
                elif out_inj[q, at[x]]:
                    assert out_sc[q, at[x]] == np.float32(ref[q, i])    # +-inf
    return inj


def entry_ok(blk, n, tags=None, require_all=None, require_any=None, excl=None, ids=None):
    """bool [nq, I]: the entry passes the masks on the corpus-order ``tags`` and its id (``ids[p]``, or p) is not in the
    query's exclusion row.  Entries outside the corpus are False."""
    nq, I = blk.shape
    inside = (blk >= 0) & (blk < n)
    p = np.where(inside, blk, 0)
    ok = inside.copy()
    if tags is not None:
        el = eligible.eligible(np.asarray(tags), require_all, require_any)              # [nq, n]
        ok &= el[np.arange(nq)[:, None], p]
    if excl is not None:
        key = p if ids is None else np.asarray(ids)[p]
        for q in range(nq):
            banned = excl[q][excl[q] >= 0]
            ok[q] &= ~np.isin(key[q], banned)
    return ok
