"""Helpers of the tests of stage-1 score boosts in the inverted-list scans (tests/test_ivf_boost_cpu.py,
tests/test_ivf_boost_gpu.py): the weight cycle, the boost patterns and the host statement of the reference.  numpy only: no
GPU, no torch.  Corpora, queries and (corpus, nprobe) shapes are those of tests/ivf_eligible_oracle.py.

R1b: the index's own PLAIN result for 2048 slots (``ivf_eligible_oracle.PLAIN_K``) - asserted to hold the whole probed set:
its last slot is unfilled for every query - re-keyed on the host.  Per query, over the filled slots (position p, score ip):

    s = float32(ip) + float32(float32(w) * float32(boost[p]))       two rounded float32 operations
    NaN s -> -inf                                                   (the list scans' rule: filed last, not dropped)
    sort by (s descending, position ascending), cut to k, pad with (-inf, -1)

With masks, ``ivf_eligible_oracle.restrict``'s predicate drops the ineligible slots first.  No boosted kernel runs in the
reference: ip is what the plain search on the same scan path wrote for the row."""
import numpy as np

from amdrec import eligible as el
from tests import boost_oracle as bx
from tests.ivf_eligible_oracle import PLAIN_K  # noqa: F401  (the slots of R1b's plain search)

WEIGHTS = (0.0, 1.0, -1.0, 0.25, 4.0, 1.0e-3)      # the per-query weights cycle through these
PATTERNS = ("noise", "sparse_half", "quantised", "signed")
NEG = np.float32(-np.inf)


def weights_for(nq: int) -> np.ndarray:
    return np.array([WEIGHTS[q % len(WEIGHTS)] for q in range(nq)], dtype=np.float32)


def pattern(name: str, n: int) -> np.ndarray:
    """The boost patterns of tests/test_boost_gpu.py at n rows: noise 0.02; 1 % of the rows at +0.5; 10 % at exactly 64.0 (with
    w = 4 the scores are quantised to the ulp of 256: exact ties, and the widest nomination bound); a signed mix (5 % at +0.5,
    5 % at -1.0 over the noise)."""
    if name == "noise":
        return bx.noise(n, seed=11)
    if name == "sparse_half":
        return bx.sparse_half(n, seed=12)
    if name == "quantised":
        return bx.quantised(n, seed=13)
    if name == "signed":
        rng = np.random.default_rng(15)
        b = bx.noise(n, seed=16)
        pick = rng.choice(n, size=n // 10, replace=False)
        b[pick[:n // 20]] = 0.5
        b[pick[n // 20:]] = -1.0
        return b
    raise KeyError(name)


def _eligible_slots(pos_q, tags, a, y):
    t = tags[np.where(pos_q >= 0, pos_q, 0)]
    return (pos_q >= 0) & ((t & a) == a) & ((y == 0) | ((t & y) != 0))


def rekey(pos, scores, boost, weight, k, tags=None, require_all=None, require_any=None):
    """R1b, vectorised per query: pos / scores [nq, PLAIN_K] of the plain search (positions, -1 = unfilled) ->
    (scores float32 [nq, k], positions int64 [nq, k])."""
    pos, scores = np.asarray(pos), np.asarray(scores, dtype=np.float32)
    boost, weight = np.asarray(boost, dtype=np.float32), np.asarray(weight, dtype=np.float32)
    nq = pos.shape[0]
    assert (pos[:, -1] == -1).all(), "R1b needs the whole probed set: the plain result's last slot must be unfilled"
    if tags is not None:
        t = el.as_words(tags, len(tags)).view(np.uint64)
        a = el.as_words(require_all, nq).view(np.uint64)
        y = el.as_words(require_any, nq).view(np.uint64)
    D = np.full((nq, k), NEG, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        ok = pos[q] >= 0 if tags is None else _eligible_slots(pos[q], t, a[q], y[q])
        p, ip = pos[q][ok], scores[q][ok]
        term = weight[q] * boost[p]                                  # one rounding
        with np.errstate(invalid="ignore"):
            s = ip + term                                            # one rounding
        assert term.dtype == np.float32 and s.dtype == np.float32
        s = np.where(np.isnan(s), NEG, s)
        order = np.lexsort((p, -s.astype(np.float64)))[:k]
        D[q, :len(order)], I[q, :len(order)] = s[order], p[order]
    return D, I


def rekey_loops(pos, scores, boost, weight, k, tags=None, require_all=None, require_any=None):
    """``rekey`` slot by slot: bx.score per element, amdrec.eligible.eligible per slot, one sort of tuples per query."""
    D, I = [], []
    for q in range(len(pos)):
        assert pos[q][-1] == -1
        rows = []
        for slot, p in enumerate(pos[q]):
            p = int(p)
            if p < 0:
                continue
            if tags is not None and not el.eligible([int(tags[p])], [int(require_all[q])], [int(require_any[q])])[0, 0]:
                continue
            with np.errstate(invalid="ignore"):
                s = bx.score(scores[q][slot], weight[q], boost[p])
            if s != s:
                s = NEG
            rows.append((-float(s), p))
        rows.sort()
        rows = rows[:k]
        D.append([np.float32(-s) for s, _ in rows] + [NEG] * (k - len(rows)))
        I.append([p for _, p in rows] + [-1] * (k - len(rows)))
    return np.asarray(D, dtype=np.float32), np.asarray(I, dtype=np.int64)
