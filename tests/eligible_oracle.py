"""Helpers of the eligibility-mask tests (tests/test_eligible_cpu.py, tests/test_eligible_gpu.py): seeded tags, the seven
query classes, and the float64 statement of the contract of amdrec.eligible.  numpy only: no GPU, no torch.

Tags: three independent draws per row - bit 0 with probability 0.5, bit 32 with 0.05, bit 63 with 0.5; the high bits are
there to catch a 32-bit truncation of a tag or a mask.  Classes, assigned q % 7, as (require_all, require_any):
(0, 0) everything; (b0, 0); (b0 | b63, 0); (0, b32); (b0 | b32 | b63, 0); (b5, b32): no row carries bit 5, nothing is
eligible; (b63, b0 | b32).  On flat_oracle.case_inputs(n = 20000, "lifted", seed 1) with tags_for(20000, 901) the classes hold
20000 / 10013 / 4926 / 998 / 241 / 0 / 5166 eligible rows (tests/test_eligible_cpu.py asserts it)."""
import numpy as np

from amdrec import eligible as el
from tests import flat_oracle

B0, B5, B32, B63 = 1 << 0, 1 << 5, 1 << 32, 1 << 63
CLASSES = ((0, 0), (B0, 0), (B0 | B63, 0), (0, B32), (B0 | B32 | B63, 0), (B5, B32), (B63, B0 | B32))
CLASS_ROWS_20000 = (20000, 10013, 4926, 998, 241, 0, 5166)


def tags_for(n, seed):
    """uint64 [n]"""
    r = np.random.default_rng(seed).random((n, 3))            # one row of three draws per corpus row
    t = np.zeros(n, dtype=np.uint64)
    for j, (bit, p) in enumerate(((B0, 0.5), (B32, 0.05), (B63, 0.5))):
        t |= np.where(r[:, j] < p, np.uint64(bit), np.uint64(0))
    return t


def masks_for(nq):
    """(require_all, require_any) uint64 [nq]: query q is of class q % 7"""
    a = np.array([CLASSES[q % 7][0] for q in range(nq)], dtype=np.uint64)
    y = np.array([CLASSES[q % 7][1] for q in range(nq)], dtype=np.uint64)
    return a, y


def class_rows(tags, c):
    """Positions of the rows eligible for class c, ascending."""
    a, y = CLASSES[c]
    return np.nonzero(el.eligible(tags, [a], [y])[0])[0]


def expected(xb, xq, k, tags, require_all, require_any):
    """Per query flat_oracle.reference on its eligible rows, positions mapped back, the unfilled tail (-inf, -1).
    -> (D [nq, k] fp32, I [nq, k] int64).  Queries with the same masks share one reference call."""
    a = el.as_words(require_all, len(xq)).view(np.uint64)
    y = el.as_words(require_any, len(xq)).view(np.uint64)
    D = np.full((len(xq), k), -np.inf, dtype=np.float32)
    I = np.full((len(xq), k), -1, dtype=np.int64)
    for ma, my in sorted({(int(u), int(v)) for u, v in zip(a, y)}):
        qs = np.nonzero((a == np.uint64(ma)) & (y == np.uint64(my)))[0]
        rows = np.nonzero(el.eligible(tags, [ma], [my])[0])[0]
        if not len(rows):
            continue
        d, i = flat_oracle.reference(xb[rows], xq[qs], k)
        D[qs], I[qs] = d, np.where(i >= 0, rows[np.maximum(i, 0)], -1)
    return D, I
