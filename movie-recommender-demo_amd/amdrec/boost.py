"""Per-ad score boosts in the Flat search ("let retrieval see the bid": expected revenue, quality score, freshness,
cold-start exploration bonus - any per-ad prior that should lift an ad into the candidate set, not only reorder it).

The rule (Flat index, both engines, every dimension; IVF-Flat with ``list_boosts``: below; IVFPQ, and IVF without the
flag, raise NotImplementedError).

Per ad.  One float32 ``boost``, finite, any sign.  A row never given one has 0.0; an index that never saw one keeps no
tensor and writes the file it always wrote; -0.0 is stored as +0.0.

Per query.  One float32 weight ``w_q``, finite.  The scalar form is validated on the host; a tensor's values are the
caller's.

Score of row ``r`` for query ``q``.  ``ip`` is the score the same engine returns for that row in an unboosted search (the
fp32 re-score chain under ``prefilter="bf16"``, the MFMA pass's value under ``"fp32"``);

    t = w_q * boost[r]        one rounded fp32 multiply
    s = ip + t                one rounded fp32 add

two roundings, not a fused multiply-add: numpy float32 arithmetic reproduces ``s`` bit for bit.

Result.  The exact top-k under ``s``: ``s`` descending, ties to the lower position; ``s`` is returned as the score; a row
whose ``ip`` is NaN is never returned; with ``k > ntotal`` the tail is unfilled as Flat writes it (-inf, -1); a query with
``w_q == 0`` gets the plain search's positions, and scores equal as numbers.  ``boost_weight=None`` is the plain search,
with not one launch more.

The key is evaluated inside the corpus pass - sample, filter, re-score and fix-up scan all see it -, not as a post-filter
over k + E <= AMDREC_MAX_K rows, so a boost can lift a row from any similarity rank.  ``exclude=`` and ``max_per_group=``
wrap the search and compose; eligibility masks together with a boost are the follow-up (NotImplementedError).

Stage-1 score boosts in the inverted-list scans (IVF-Flat, opt-in per index: ``FAISSIndex(index_type="IVF",
list_boosts=True)`` or ``enable_list_boosts()`` on a built or loaded index; the flag is a field of the saved header, a file
without it loads as off; Flat ignores the flag; IVFPQ with the flag raises NotImplementedError - its scan holds L2 distances
of codes and its refine stage would have to re-rank under the same key).

Without the flag nothing changes: ``add(boosts=)``, ``set_boosts``, ``boost_weight=`` and ``stage1_boost=`` on an IVF or
IVFPQ index raise what they always raised, before the library is touched.

With the flag ``add(boosts=)`` / ``set_boosts`` / ``get_boosts`` work as on Flat (same validation, same ``_boost_max``),
the index keeps ``list_boosts = boosts[row_pos]`` next to its lists (4 bytes per ad, made with the list layout and again
when ``set_boosts`` swaps the tensor - never at search time; a captured graph pins the copy it was captured with), and the
searches and the pipeline calls take the weight.  ``ShardedRecommender`` and ``MicroBatcher`` still do not.

The result is the INDEX'S OWN result under the boosted key: per query the exact top-k under ``s`` of the rows of the lists
the PLAIN search probes.  The probes are chosen by similarity alone - a boosted ad in a list that is not probed is not
found; that is what IVF means.  (Opt-in per index, ``FAISSIndex(aware_probes=True)`` / ``enable_aware_probes()``: the coarse
key of a boosted search becomes <q, centroid> + w_q * the list's largest boost - smallest for w_q < 0 -, so a list that
holds a strongly boosted ad is probed for it; amdrec.probes has the rule.)  ``ip`` is, bit for bit, the score the plain search on the same scan path writes for the
row (the pair scan's fma chain, the grouped scans' MFMA value, the prefilter's fp32 re-score chain); ``t`` and ``s`` are
the two rounded operations above; then the list scans' own rule applies to ``s``: a NaN ``s`` files as -inf (the row ranks
last, it is not dropped); order: ``s`` descending, ties to the lower position; fewer than k probed rows leave the -inf / -1
tail; ``w_q == 0`` gives the plain search's positions; ``boost_weight=None`` launches the kernels it always launched.  In
the two-phase scan the first phase's threshold is the k-th BOOSTED score of the nearest probes - still a lower bound of the
final k-th boosted score, so the scan stays exact -, and the bf16 prefilter's nomination bound is widened for the two
roundings (``amdrec_ivf_filter_bounds_boosted``).

Boost together with masks on an IVF index that has both ``list_tags`` and ``list_boosts``: the exact top-k under ``s`` of
the ELIGIBLE probed rows.  Flat with a boost and masks keeps raising.

This module holds the host helpers (no GPU needed for anything but the final copy).
"""
from __future__ import annotations

import math

import numpy as np
import torch

FOLLOW_UP_MASKS = ("a stage-1 boost together with eligibility masks (require_all / require_any) is not implemented: the "
                   "boosted kernels do not test the predicate yet - that is the follow-up (DESIGN.md, 'Stage-1 score boosts')")


LIST_BOOSTS_IVFPQ = ("list_boosts on an IVFPQ index is not implemented: its scan holds squared L2 distances of codes, not inner "
                     "products, and its refine stage would have to re-rank under the same key (DESIGN.md, 'Stage-1 score boosts "
                     "in the inverted-list scans')")


def follow_up_index(index_type: str) -> str:
    """What an index that does not take boosts raises: IVFPQ, and IVF without ``list_boosts`` (the wording predates the
    opt-in and is pinned by tests)."""
    return (f"stage-1 score boosts are implemented for the Flat index only; the {index_type} list scans do not add the term "
            "yet - that is the follow-up (DESIGN.md, 'Stage-1 score boosts')")


def as_boosts(x, n: int) -> np.ndarray:
    """``n`` boosts as numpy float32 [n], -0.0 stored as +0.0.  ``x``: one number (given to all n), a sequence of numbers, a
    numpy array or a torch tensor of a real dtype.  Non-finite values (also after the rounding to float32), bools and a
    length other than n are refused (ValueError / TypeError)."""
    n = int(n)
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, (bool, np.bool_)):
        raise TypeError("boosts must be numbers, got a bool")
    a = np.asarray(x)
    if a.dtype == object or a.dtype.kind not in "fiu":
        raise TypeError(f"boosts must be real numbers, got dtype {a.dtype}")
    if a.ndim == 0:
        a = np.full(n, a)
    if a.shape != (n,):
        raise ValueError(f"expected {n} boosts, got shape {tuple(a.shape)}")
    with np.errstate(over="ignore"):
        out = a.astype(np.float32)
    if not np.isfinite(out).all():
        raise ValueError("boosts must be finite (as float32)")
    return out + np.float32(0.0)                      # -0.0 + 0.0 = +0.0


def device_boosts(x, n: int, device):
    """as_boosts on the device -> (float32 [n] tensor, max |boost| as a Python float).  A device float32 tensor of the right
    length is checked there (one reduction and a host read: set / add time, never search time)."""
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32:
        if x.shape != (n,):
            raise ValueError(f"expected {n} boosts, got shape {tuple(x.shape)}")
        t = x.contiguous() + 0.0                      # a copy; -0.0 -> +0.0
        bmax = float(t.abs().max()) if n else 0.0
        if not math.isfinite(bmax):
            raise ValueError("boosts must be finite (as float32)")
        return t, bmax
    a = as_boosts(x, n)
    return torch.from_numpy(a).to(device), (float(np.abs(a).max()) if n else 0.0)


def check_weight(w) -> float:
    """A scalar boost weight -> the float32 value as a Python float.  Refused: bools, non-numbers, non-finite values."""
    if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, float, np.integer, np.floating)):
        raise TypeError(f"boost_weight must be a number, a sequence of numbers or a float32 tensor, got {type(w).__name__}")
    with np.errstate(over="ignore"):
        v = float(np.float32(w))
    if not math.isfinite(v):
        raise ValueError(f"boost_weight must be finite (as float32), got {w!r}")
    return v


def as_weights(w, nq: int) -> np.ndarray:
    """The ``boost_weight`` argument of search / batch_search -> numpy float32 [nq]: one number for every query, or a
    sequence / array of nq numbers.  Every value is validated like the scalar form."""
    if isinstance(w, torch.Tensor):
        w = w.detach().cpu().numpy()
    if isinstance(w, np.ndarray) and w.ndim == 0:
        w = w.item()
    if isinstance(w, (int, float, np.integer, np.floating, bool, np.bool_)):
        return np.full(int(nq), check_weight(w), dtype=np.float32)
    vals = [check_weight(v) for v in (w.tolist() if isinstance(w, np.ndarray) else list(w))]
    if len(vals) != nq:
        raise ValueError(f"{len(vals)} boost weights for {nq} queries")
    return np.asarray(vals, dtype=np.float32)


def device_weights(w, nq: int, device) -> torch.Tensor:
    """The ``boost_weight`` argument of search_device -> device float32 [nq].  A scalar is validated on the host (finite)
    and filled; a device float32 tensor [nq] is taken as it is - its values are the caller's."""
    if isinstance(w, torch.Tensor):
        if not w.is_cuda or w.dtype != torch.float32:
            raise TypeError(f"a boost_weight tensor must be a device float32 tensor, got {w.dtype} on {w.device}")
        if w.shape != (nq,):
            raise ValueError(f"boost_weight must be [{nq}], got {tuple(w.shape)}")
        return w.contiguous()
    return torch.full((nq,), check_weight(w), dtype=torch.float32, device=device)


def boosted_scores(ip, boost, weight) -> np.ndarray:
    """The rule in numpy: ip float32 [nq, n] (the engine's unboosted scores), boost [n], weight [nq] -> s float32 [nq, n]."""
    ip = np.asarray(ip, dtype=np.float32)
    t = np.asarray(weight, dtype=np.float32)[:, None] * np.asarray(boost, dtype=np.float32)[None, :]      # one rounding
    return ip + t                                                                                          # one rounding


def boost_oracle(ip, boost, weight, k: int):
    """The result in numpy: (positions int64 [nq, k], scores float32 [nq, k]) - the top-k under boosted_scores, s descending,
    ties to the lower position, rows whose ip is NaN left out, the tail unfilled (-1, -inf)."""
    s = boosted_scores(ip, boost, weight)
    nq, n = s.shape
    pos = np.full((nq, k), -1, dtype=np.int64)
    sc = np.full((nq, k), -np.inf, dtype=np.float32)
    ok = ~np.isnan(np.asarray(ip, dtype=np.float32))
    for q in range(nq):
        rows = np.flatnonzero(ok[q] & ~np.isnan(s[q]))
        order = rows[np.lexsort((rows, -s[q, rows].astype(np.float64)))][:k]
        pos[q, :len(order)] = order
        sc[q, :len(order)] = s[q, order]
    return pos, sc
