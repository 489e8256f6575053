"""Per-request must-consider lists ("score these ads for this user": retargeting lists, direct-sold or guaranteed campaigns,
ads in a cart, freshly added ads whose embedding is still poor, exploration slots) - a second candidate source next to the
similarity search.

The rule, the same for Flat and IVF (IVFPQ keeps codes, not rows: NotImplementedError).  Per query:

- ``R`` is the result the same call returns without the list: ``k`` entries (position, score), ``f`` of them filled, ordered
  by score descending, ties to the lower position, the unfilled tail last.  Masks, exclusion list, boost weight and probe
  policy apply to it as given.
- ``L`` is the query's include list of ``I`` ad ids; negative entries are padding.

``V``, the valid entries of ``L``, in list order - an entry counts when

1. its id resolves to a corpus position ``p`` in ``[0, n)`` (unknown ids are ignored; where ids repeat in the index, ``p`` is
   the lowest position);
2. ``p`` has not occurred earlier in ``L``;
3. if the call carries ``require_all`` / ``require_any``: row ``p`` passes the predicate of amdrec.eligible on ``tags[p]``
   (the corpus-order tags, for Flat and IVF alike);
4. the row's id is not in the call's exclusion list (exclusion wins over inclusion);
5. its score ``s_p`` is not NaN (a stored NaN row or a NaN query drops the entry).

``s_p`` is the fp32 value of the searches' shared re-score chain (csrc/topk_utils.hpp ``dot_rows``: a per-lane fma chain, then
the xor butterfly); with a boost weight it is followed by the two rounded operations of amdrec.boost (``RowBoost``).  Then

- ``A = V ∩ positions(R)``: these entries are left exactly as the search wrote them - position, score and rank unchanged;
- ``N = V \\ positions(R)``, ``m = |N|``;
- ``R`` loses its ``max(0, f + m - k)`` lowest-ranked filled entries that are not in ``V`` (there are always enough of them:
  ``I <= k`` is enforced);
- the output is the kept entries and ``N`` together, ordered by score descending, ties to the lower position, then the
  unfilled tail (-1, -inf);
- a byte per slot, ``injected``, is 1 exactly for the entries of ``N``.

So every entry of ``V`` is in the output; a list of padding only returns ``R`` bit for bit; ``include=None`` or ``I = 0`` is
the plain call with not one launch more.  ``1 <= I <= min(k, AMDREC_MAX_INCLUDE = 64)``.  A per-group cap at the search level
(``max_per_group``) together with a list raises ValueError: whether the cap runs before or after the injection is not decided.

The merge is one launch of ``amdrec_include_merge`` (csrc/include.hip) behind the unchanged search.  This module holds the
numpy oracle of the rule, the host helpers (no GPU needed) and the binding call.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

CAP_ORDER = ("an include list together with max_per_group at the search level: whether the per-group cap applies before or "
             "after the listed ads are merged in is left undecided, so the combination is refused (the stage-2 cap of the "
             "pipeline, which sees the merged candidates, works)")
IVFPQ = ("an include list on an IVFPQ index: the index keeps codes, not rows, so a listed ad cannot be given its exact score "
         "(as amdrec.diversity says of the same index); use Flat or IVF")


def check_include(k: int, I: int) -> int:
    """-> I; ValueError for a list wider than AMDREC_MAX_INCLUDE or than k (every valid entry must fit the result)."""
    k, I = int(k), int(I)
    if I < 0:
        raise ValueError(f"an include list cannot have {I} entries")
    if I > _lib.MAX_INCLUDE:
        raise ValueError(f"an include list of {I} entries per query exceeds AMDREC_MAX_INCLUDE = {_lib.MAX_INCLUDE}")
    if I > k:
        raise ValueError(f"an include list of {I} entries per query exceeds k = {k}: every listed ad must fit the result")
    return I


def merge_oracle(r_pos, r_scores, incl_pos, n: int, incl_scores, ok=None):
    """The rule in numpy, one query.  ``r_pos`` / ``r_scores`` [k]: R.  ``incl_pos`` [I]: the list as corpus positions
    (negative, or >= ``n``: ignored).  ``incl_scores`` [I]: s_p of every entry (NaN drops it; ignored entries may hold
    anything).  ``ok`` (bool [I], optional): the entry passes the masks and is not excluded.
    -> (positions int64 [k], scores float32 [k], injected uint8 [k])."""
    r_pos = np.asarray(r_pos, dtype=np.int64)
    r_scores = np.asarray(r_scores, dtype=np.float32)
    L = np.asarray(incl_pos, dtype=np.int64).reshape(-1)
    s = np.asarray(incl_scores, dtype=np.float32).reshape(-1)
    k = r_pos.shape[0]
    filled = r_pos >= 0
    f = int(filled.sum())
    valid = (L >= 0) & (L < int(n)) & ~np.isnan(s)
    if ok is not None:
        valid &= np.asarray(ok, dtype=bool).reshape(-1)
    first = np.zeros(L.shape[0], dtype=bool)
    first[np.unique(L, return_index=True)[1]] = True
    valid &= first
    V, Vs = L[valid], s[valid]
    held = np.isin(V, r_pos[filled])
    Np, Ns = V[~held], Vs[~held]
    m = Np.shape[0]
    keep = filled.copy()
    evict = max(0, f + m - k)
    if evict:
        unlisted = np.flatnonzero(filled & ~np.isin(r_pos, V))
        keep[unlisted[unlisted.shape[0] - evict:]] = False
    pos = np.concatenate([r_pos[keep], Np])
    sc = np.concatenate([r_scores[keep], Ns])
    inj = np.concatenate([np.zeros(int(keep.sum()), dtype=np.uint8), np.ones(m, dtype=np.uint8)])
    order = np.lexsort((pos, -sc.astype(np.float64)))
    out_pos = np.full(k, -1, dtype=np.int64)
    out_sc = np.full(k, -np.inf, dtype=np.float32)
    out_inj = np.zeros(k, dtype=np.uint8)
    out_pos[:order.shape[0]], out_sc[:order.shape[0]], out_inj[:order.shape[0]] = pos[order], sc[order], inj[order]
    return out_pos, out_sc, out_inj


def _id_list(seq) -> list:
    out = []
    for x in ([] if seq is None else seq):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
            raise TypeError(f"included ad ids must be integers, got {x!r} ({type(x).__name__})")
        if x < 0:
            raise ValueError(f"included ad ids must be >= 0 (negative entries are the padding), got {x}")
        out.append(int(x))
    return out


def pad_inclusions(seqs: Sequence, width: Optional[int] = None) -> np.ndarray:
    """One id sequence per query -> int64 [nq, I], each row its ids then -1 padding; I = the longest list, or ``width``
    (ValueError if a list is longer).  Negative ids and non-integers are refused."""
    rows = [_id_list(s) for s in seqs]
    longest = max((len(r) for r in rows), default=0)
    if width is None:
        width = longest
    elif int(width) < longest:
        raise ValueError(f"an include list has {longest} entries, more than width = {width}")
    out = np.full((len(rows), int(width)), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def as_block(include, nq: int) -> Optional[np.ndarray]:
    """The ``include`` argument of the numpy-level calls (a list of per-query sequences, or an integer array [nq, I] whose
    negative entries are padding) -> int64 [nq, I], or None for "no list" (None, or I = 0)."""
    if include is None:
        return None
    if isinstance(include, torch.Tensor):
        include = include.detach().cpu().numpy()
    if isinstance(include, np.ndarray) and include.dtype != object:
        if include.dtype.kind not in "iu" or include.ndim != 2:
            raise TypeError(f"an include array must be an integer array [nq, I], got {include.dtype} {include.shape}")
        blk = np.ascontiguousarray(include, dtype=np.int64)
    else:
        blk = pad_inclusions(include)
    if blk.shape[0] != nq:
        raise ValueError(f"{blk.shape[0]} include lists for {nq} queries")
    return blk if blk.shape[1] else None


def build_id_table(ids: torch.Tensor):
    """The lookup table of an index's integer ids (``ids`` int64 [n], any device): (the ids in ascending order, the position
    of each) from a STABLE sort, so that among rows that share an id the lowest position comes first."""
    srt, order = torch.sort(ids, stable=True)
    return srt, order


def lookup_positions(table, ids: torch.Tensor) -> torch.Tensor:
    """Ad ids (int64, any shape) -> corpus positions through ``build_id_table``'s table: the lowest position that carries
    the id, -1 where no row does (and for negative entries, the padding).  No host synchronisation."""
    srt, order = table
    if srt.shape[0] == 0:
        return torch.full_like(ids, -1)
    at = torch.searchsorted(srt, ids.contiguous()).clamp_(max=srt.shape[0] - 1)
    hit = (srt[at] == ids) & (ids >= 0)
    return torch.where(hit, order[at], torch.full_like(ids, -1))


def merge(pos: torch.Tensor, scores: torch.Tensor, incl_pos: torch.Tensor, rows: torch.Tensor, n_rows: int,
          queries: torch.Tensor, elig=None, exclude: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None,
          boost=None, want_injected: bool = True):
    """amdrec_include_merge on device tensors: ``pos`` / ``scores`` [nq, k] (a search's result by position), ``incl_pos``
    int64 [nq, I] corpus positions, ``rows`` the fp32 corpus (its first ``n_rows`` rows count), ``queries`` [nq, d] as the
    search saw them (normalised).  ``elig`` = (tags [>= n_rows], require_all [nq], require_any [nq]); ``exclude`` int64
    [nq, E] with ``ids`` [>= n_rows] where ids are not positions; ``boost`` = (boosts [>= n_rows], weights [nq]).
    -> (positions, scores, injected uint8 or None), each [nq, k]."""
    nq, k = pos.shape
    dev = pos.device
    incl_pos = _lib.require_gpu(incl_pos, "include", torch.int64)
    if incl_pos.dim() != 2 or incl_pos.shape[0] != nq or (incl_pos.shape[1] > 1 and incl_pos.stride(1) != 1):
        raise ValueError(f"include must be int64 [{nq}, I] with contiguous rows, got {tuple(incl_pos.shape)}")
    I = incl_pos.shape[1]
    queries = _lib.require_gpu(queries, "queries", torch.float32)
    d = rows.shape[1]
    if queries.dim() != 2 or queries.shape != (nq, d) or (d > 1 and queries.stride(1) != 1):
        raise ValueError(f"queries must be float32 [{nq}, {d}] with contiguous rows, got {tuple(queries.shape)}")
    pos, scores = pos.contiguous(), scores.contiguous()
    tags = ra = ry = None
    if elig is not None:
        tags, ra, ry = elig
    E = ld_e = 0
    if exclude is not None and exclude.shape[-1] > 0:
        exclude = _lib.require_gpu(exclude, "exclude", torch.int64)
        if exclude.dim() != 2 or exclude.shape[0] != nq or (exclude.shape[1] > 1 and exclude.stride(1) != 1):
            raise ValueError(f"exclude must be int64 [{nq}, E] with contiguous rows, got {tuple(exclude.shape)}")
        E = exclude.shape[1]
        ld_e = exclude.stride(0) if nq > 1 else E
    else:
        exclude = ids = None
    boosts, w = (None, None) if boost is None else boost
    out_pos = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_inj = torch.empty((nq, k), dtype=torch.uint8, device=dev) if want_injected else None
    _lib.check(_lib.load().amdrec_include_merge(
        _lib.ptr(pos), _lib.ptr(scores), nq, k, _lib.ptr(incl_pos), I, incl_pos.stride(0) if nq > 1 else I,
        _lib.ptr(rows), rows.stride(0), n_rows, d, _lib.ptr(queries), queries.stride(0) if nq > 1 else d, _lib.ptr(tags),
        _lib.ptr(ra), _lib.ptr(ry), _lib.ptr(exclude), E, ld_e, _lib.ptr(ids), _lib.ptr(boosts), _lib.ptr(w),
        _lib.ptr(out_pos), _lib.ptr(out_scores), _lib.ptr(out_inj), _lib.stream_ptr(dev)))
    return out_pos, out_scores, out_inj
