"""Aware probes: a coarse step that sees the request's eligibility masks and stage-1 boost weight (IVF and IVFPQ, opt-in
per index: ``FAISSIndex(index_type="IVF" | "IVFPQ", aware_probes=True)`` or ``enable_aware_probes()`` on a built or loaded
index; the flag is a field of the saved header, written only when on - a file without it loads as off; Flat ignores it).

Why.  ``InvertedLists.coarse_probes`` picks the ``nprobe`` lists by <q, centroid> alone.  A request with a rare tag then
spends most of its probes on lists that hold no eligible row and returns a short tail while eligible ads sit a few lists
further out; a request with a boost weight finds a strongly boosted ad only when its list is among the most similar anyway.

Without the flag nothing changes anywhere.  With it, a search that carries masks and / or a boost weight chooses its probes
under the rule below; a search with neither takes the plain coarse path, launch for launch.  ``search_device`` / ``search``
/ ``batch_search`` take ``probe_policy=None | "similarity" | "aware"``: None = the index's flag decides, "similarity" on a
flagged index = the plain probes (A/B runs), "aware" on an index without the flag raises ValueError before the library is
touched.  The pipeline calls follow the index's flag.  ``ShardedRecommender`` keeps probing by similarity (a shard-local
feasibility would make the ranks probe different lists).

The rule.

Per list ``l`` of the current layout (the SUMMARIES, made by ``amdrec_ivf_list_summaries`` whenever the list-order copies
are made or swapped - ``layout()``, ``set_tags``, ``set_boosts``, ``remove_ids``, ``add`` -, never at search time, out of
place: a captured graph keeps the copy it was captured with):

    len[l]                         rows of the list
    tag_or[l]                      OR of its rows' tag words                     (with ``list_tags``)
    boost_hi[l] / boost_lo[l]      max / min of its rows' boosts                 (with ``list_boosts`` and boosts present)

an empty list has tag_or = 0, boost_hi = boost_lo = 0.0.

Feasible(q, l):  ``len[l] > 0``; with masks also ``(tag_or[l] & all_q) == all_q`` and ``any_q == 0 or (tag_or[l] & any_q)
!= 0``.  This is a NECESSARY condition only: two bits of ``require_all`` may sit on different rows of the list, so a feasible
list can still hold no eligible row (an infeasible one never holds one).

Key.  ``c`` is the score the plain key table holds for (q, l), bit for bit (same GEMM mainloop, same three query-tile
shapes).  With a weight ``w_q``:

    b = boost_hi[l] if w_q >= 0 else boost_lo[l]
    t = w_q * b           one rounded fp32 multiply
    s = c + t             one rounded fp32 add

(two roundings, not a fused multiply-add - the scans' rule, amdrec.boost); without a weight ``s = c``.  ``s`` bounds from
above the boosted key of a row whose similarity equals the centroid's.  A NaN ``s`` is filed as the plain table files a NaN
score: as -inf (it ranks last, it is not dropped).

Probes.  The ``nprobe`` best FEASIBLE lists by ``s`` descending, ties to the lower list; fewer feasible lists than
``nprobe`` leave a ``-1`` tail (no list: the grouping, the pair scan and the IVFPQ tables skip it).

Everything after the probes is unchanged - same scans, same phases, same tiles; the two-phase scan's first phase is the
first ``first_phase_probes(nprobe)`` columns of the new order, its tau still the k-th key of a subset.  The result contract:
the existing masked / boosted result over the lists chosen by this rule.

This module holds the rule in numpy (no GPU, no torch): the oracle of the kernels and the host tests.
"""
from __future__ import annotations

import numpy as np

POLICIES = (None, "similarity", "aware")


def check_policy(probe_policy, flagged: bool) -> bool:
    """The ``probe_policy`` argument -> does this search choose its probes under the rule?  (host only: raises before the
    library is touched)"""
    if probe_policy not in POLICIES:
        raise ValueError(f"probe_policy must be None, 'similarity' or 'aware', got {probe_policy!r}")
    if probe_policy == "aware" and not flagged:
        raise ValueError("probe_policy='aware' needs the per-list summaries: FAISSIndex(aware_probes=True) or "
                         "enable_aware_probes()")
    return flagged and probe_policy != "similarity"


def _u64(a):
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64)


def list_summaries(list_off, list_tags=None, list_boosts=None):
    """The summaries in numpy: list_off int64 [nlist + 1], list_tags (u)int64 [N] / list_boosts float32 [N] in list order ->
    (tag_or uint64 [nlist] or None, boost_hi float32 [nlist] or None, boost_lo float32 [nlist] or None)."""
    off = np.asarray(list_off, dtype=np.int64)
    nlist = len(off) - 1
    tag_or = hi = lo = None
    if list_tags is not None:
        t = _u64(list_tags)
        tag_or = np.zeros(nlist, dtype=np.uint64)
        for l in range(nlist):
            if off[l + 1] > off[l]:
                tag_or[l] = np.bitwise_or.reduce(t[off[l]:off[l + 1]])
    if list_boosts is not None:
        b = np.asarray(list_boosts, dtype=np.float32)
        hi, lo = np.zeros(nlist, dtype=np.float32), np.zeros(nlist, dtype=np.float32)
        for l in range(nlist):
            if off[l + 1] > off[l]:
                hi[l], lo[l] = b[off[l]:off[l + 1]].max(), b[off[l]:off[l + 1]].min()
    return tag_or, hi, lo


def feasible(list_len, tag_or=None, require_all=None, require_any=None, nq=None) -> np.ndarray:
    """-> bool [nq, nlist].  Without masks (tag_or None): the non-empty lists, for each of ``nq`` queries."""
    ok = np.asarray(list_len) > 0
    if tag_or is None:
        return np.broadcast_to(ok, (int(nq), len(ok))).copy()
    t, a, y = _u64(tag_or)[None, :], _u64(require_all)[:, None], _u64(require_any)[:, None]
    return ok[None, :] & ((t & a) == a) & ((y == 0) | ((t & y) != 0))


def aware_scores(c, boost_hi=None, boost_lo=None, weight=None) -> np.ndarray:
    """c float32 [nq, nlist] (the plain table's scores) -> s float32 [nq, nlist]; without a weight s = c."""
    c = np.asarray(c, dtype=np.float32)
    if weight is None:
        return c.copy()
    w = np.asarray(weight, dtype=np.float32)[:, None]
    b = np.where(w >= 0, np.asarray(boost_hi, dtype=np.float32)[None, :], np.asarray(boost_lo, dtype=np.float32)[None, :])
    with np.errstate(over="ignore", invalid="ignore"):
        t = (w * b).astype(np.float32)                         # one rounding
        return (c + t).astype(np.float32)                      # one rounding


def rank_last(s) -> np.ndarray:
    """A NaN score is filed as -inf (csrc/invlists.hpp rank_last)."""
    s = np.asarray(s, dtype=np.float32)
    return np.where(np.isnan(s), np.float32(-np.inf), s)


def aware_probes(c, nprobe: int, list_len, tag_or=None, require_all=None, require_any=None, boost_hi=None, boost_lo=None,
                 weight=None):
    """The probes in numpy -> (int64 [nq, nprobe], -1 = none; s float32 [nq, nlist]; feasible bool [nq, nlist])."""
    s = rank_last(aware_scores(c, boost_hi, boost_lo, weight))
    ok = feasible(list_len, tag_or, require_all, require_any, nq=s.shape[0])
    nq, nlist = s.shape
    probes = np.full((nq, nprobe), -1, dtype=np.int64)
    lists = np.arange(nlist)
    for q in range(nq):
        cand = lists[ok[q]]
        order = cand[np.lexsort((cand, -s[q, cand].astype(np.float64)))][:nprobe]
        probes[q, :len(order)] = order
    return probes, s, ok


def aware_probes_slotwise(c, nprobe: int, list_len, tag_or=None, require_all=None, require_any=None, boost_hi=None,
                          boost_lo=None, weight=None) -> np.ndarray:
    """aware_probes as plain loops, one (query, list) slot at a time with Python integers and numpy float32 scalars: the
    statement of the rule the vectorised form is tested against."""
    c = np.asarray(c, dtype=np.float32)
    nq, nlist = c.shape
    out = np.full((nq, nprobe), -1, dtype=np.int64)
    for q in range(nq):
        found = []
        for l in range(nlist):
            if int(list_len[l]) <= 0:
                continue
            if tag_or is not None:
                t, a, y = (int(_u64(np.asarray([v]))[0]) for v in (tag_or[l], require_all[q], require_any[q]))
                if (t & a) != a or (y != 0 and (t & y) == 0):
                    continue
            s = c[q, l]
            if weight is not None:
                w = np.float32(weight[q])
                b = np.float32(boost_hi[l]) if w >= 0 else np.float32(boost_lo[l])
                with np.errstate(over="ignore", invalid="ignore"):
                    s = np.float32(np.float32(w * b) + s)
            if np.isnan(s):
                s = np.float32(-np.inf)
            found.append((-float(s), l))
        found.sort()
        for i, (_, l) in enumerate(found[:nprobe]):
            out[q, i] = l
    return out
