"""The stage-1 score-boost rule (amdrec.boost) restated as plain loops, the seeded boost patterns of the GPU surface and
its float64 oracle.

Rule: s[q][r] = f32(ip[q][r] + f32(w[q] * boost[r])) - two rounded float32 operations -; the result is the rows in order
(s descending, position ascending), rows whose ip is NaN left out, cut to k, the tail (-inf, -1)."""
import numpy as np

N, NQ = 20_000, 513
WEIGHTS = (0.0, 0.5, 1.0, 4.0)          # the per-query weights cycle through these


def weights_for(nq: int) -> np.ndarray:
    return np.array([WEIGHTS[q % len(WEIGHTS)] for q in range(nq)], dtype=np.float32)


def score(ip, w, b) -> np.float32:
    """One element, spelled out: every operand and every result a numpy float32."""
    t = np.float32(np.float32(w) * np.float32(b))
    return np.float32(np.float32(ip) + t)


def topk_loops(ip, boost, weight, k):
    """(scores [nq][k], positions [nq][k]) as nested Python lists, by loops and one sort per query."""
    D, I = [], []
    for q in range(len(ip)):
        rows = []
        for r in range(len(boost)):
            if ip[q][r] != ip[q][r]:                     # NaN ip: never returned
                continue
            rows.append((-float(score(ip[q][r], weight[q], boost[r])), r))
        rows.sort()
        rows = rows[:k]
        D.append([np.float32(-s) for s, _ in rows] + [np.float32(-np.inf)] * (k - len(rows)))
        I.append([r for _, r in rows] + [-1] * (k - len(rows)))
    return D, I


def topk(ip, boost, weight, k):
    """The same in numpy -> (D float32 [nq, k], I int64 [nq, k]); ip float32 [nq, n] (any float dtype is taken as float32)."""
    ip = np.asarray(ip, dtype=np.float32)
    t = np.asarray(weight, dtype=np.float32)[:, None] * np.asarray(boost, dtype=np.float32)[None, :]
    s = ip + t
    assert s.dtype == np.float32 and t.dtype == np.float32
    nq, n = s.shape
    D = np.full((nq, k), -np.inf, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        rows = np.flatnonzero(~np.isnan(ip[q]))
        order = rows[np.lexsort((rows, -s[q, rows].astype(np.float64)))][:k]
        D[q, :len(order)], I[q, :len(order)] = s[q, order], order
    return D, I


def expected64(xb, xq, boost, weight, k):
    """The float64 oracle for the fp32 engine: ip64 + w * b in float64, exact top-k -> (D float32, I int64)."""
    s = xq.astype(np.float64) @ xb.astype(np.float64).T + \
        np.asarray(weight, dtype=np.float64)[:, None] * np.asarray(boost, dtype=np.float64)[None, :]
    nq, n = s.shape
    kk = min(k, n)
    I = np.full((nq, k), -1, dtype=np.int64)
    D = np.full((nq, k), -np.inf, dtype=np.float32)
    for q in range(nq):
        order = np.lexsort((np.arange(n), -s[q]))[:kk]
        I[q, :kk], D[q, :kk] = order, s[q, order].astype(np.float32)
    return D, I


# ---- the seeded boost patterns of the GPU surface -------------------------------------------------------------------
def noise(n=N, seed=11) -> np.ndarray:
    """small noise on the scale of the score gaps"""
    return (0.02 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def sparse_half(n=N, seed=12) -> np.ndarray:
    """1 % of the rows at +0.5: the winners are mostly boosted rows"""
    b = np.zeros(n, dtype=np.float32)
    b[np.random.default_rng(seed).choice(n, size=n // 100, replace=False)] = 0.5
    return b


def demote(rows, n=N) -> np.ndarray:
    """the given rows (the unboosted top-k of some queries) at -1"""
    b = np.zeros(n, dtype=np.float32)
    b[np.asarray(rows, dtype=np.int64)] = -1.0
    return b


def quantised(n=N, seed=13) -> np.ndarray:
    """10 % of the rows at exactly 64.0: with w = 4 the scores are quantised to the ulp of 256 and tie massively"""
    b = np.zeros(n, dtype=np.float32)
    b[np.random.default_rng(seed).choice(n, size=n // 10, replace=False)] = 64.0
    return b


def unseen_only(seen, count, value=2.0, seed=14) -> np.ndarray:
    """``count`` rows the strided sample does not read (``seen``: bool [n]) at ``value``, every other row 0"""
    b = np.zeros(len(seen), dtype=np.float32)
    b[np.random.default_rng(seed).choice(np.flatnonzero(~seen), size=count, replace=False)] = value
    return b
