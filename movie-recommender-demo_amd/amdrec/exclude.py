"""Per-request exclusion lists ("not these ads for this user": frequency caps, blocked advertisers, hidden ads).

Contract, the same for every index type: a search for ``k`` with the exclusion block ``excl[i, 0:E]`` of query ``i`` (ad ids;
negative entries are padding and match nothing) is the UNFILTERED search of the same index for ``kc = k + E`` entries with
every entry whose id is in ``excl[i]`` removed, the survivors in their order (score, then lower position), cut to the first
``k``; slots past the last survivor are unfilled as that index type writes unfilled slots (Flat / IVF: -inf and position -1;
IVFPQ: +inf and -1).  At most E entries leave the best k + E, so with unique ids at least k of them stay: for Flat the result
is the exact top-k of the corpus without the excluded ads, for IVF / IVFPQ the best k non-excluded rows of the probed lists
(with refine, the re-rank sees k + E as its k).  With ids that are not unique one excluded id may remove several rows, and
the tail can then be unfilled although eligible rows exist further down.  ``k + E <= AMDREC_MAX_K``.

The removal is one launch of ``amdrec_exclude_compact`` (csrc/exclude.hip) behind the unchanged search kernels; the over-fetch
is the price of leaving the tuned scans alone.  This module holds the host helpers (no GPU needed) and the binding call.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib


def check_exclude(k: int, E: int) -> int:
    """-> kc = k + E, the candidates the unfiltered search is asked for; ValueError when that exceeds AMDREC_MAX_K."""
    k, E = int(k), int(E)
    if E < 0:
        raise ValueError(f"an exclusion list cannot have {E} entries")
    if k + E > _lib.MAX_K:
        raise ValueError(f"k + E = {k} + {E} exceeds AMDREC_MAX_K = {_lib.MAX_K}: a search with an exclusion list of E entries "
                         f"per query asks the index for k + E candidates")
    return k + E


def _id_list(seq) -> list:
    out = []
    for x in ([] if seq is None else seq):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
            raise TypeError(f"excluded ad ids must be integers, got {x!r} ({type(x).__name__})")
        if x < 0:
            raise ValueError(f"excluded ad ids must be >= 0 (negative entries are the padding), got {x}")
        out.append(int(x))
    return out


def pad_exclusions(seqs: Sequence, width: Optional[int] = None) -> np.ndarray:
    """One id sequence per query -> int64 [nq, E], each row its ids then -1 padding; E = the longest list, or ``width``
    (ValueError if a list is longer).  Negative ids and non-integers are refused."""
    rows = [_id_list(s) for s in seqs]
    longest = max((len(r) for r in rows), default=0)
    if width is None:
        width = longest
    elif int(width) < longest:
        raise ValueError(f"an exclusion list has {longest} entries, more than width = {width}")
    out = np.full((len(rows), int(width)), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def as_block(exclude, nq: int) -> Optional[np.ndarray]:
    """The ``exclude`` argument of the numpy-level calls (a list of per-query sequences, or an integer array [nq, E] whose
    negative entries are padding) -> int64 [nq, E], or None for "no list" (None, or E = 0)."""
    if exclude is None:
        return None
    if isinstance(exclude, torch.Tensor):
        exclude = exclude.detach().cpu().numpy()
    if isinstance(exclude, np.ndarray) and exclude.dtype != object:
        if exclude.dtype.kind not in "iu" or exclude.ndim != 2:
            raise TypeError(f"an exclusion array must be an integer array [nq, E], got {exclude.dtype} {exclude.shape}")
        blk = np.ascontiguousarray(exclude, dtype=np.int64)
    else:
        blk = pad_exclusions(exclude)
    if blk.shape[0] != nq:
        raise ValueError(f"{blk.shape[0]} exclusion lists for {nq} queries")
    return blk if blk.shape[1] else None


def compact(keys: torch.Tensor, scores: torch.Tensor, carry: Optional[torch.Tensor], excl: torch.Tensor, k: int,
            fill_score: float, want_keys: bool = True):
    """amdrec_exclude_compact on device tensors: ``keys`` / ``scores`` / ``carry`` [nq, kc] (carry may be None), ``excl``
    int64 [nq, E] -> (keys or None, scores, carry or None), each [nq, k].  Unfilled slots: -1 / ``fill_score`` / -1."""
    nq, kc = keys.shape
    dev = keys.device
    excl = _lib.require_gpu(excl, "exclude", torch.int64)
    if excl.dim() != 2 or excl.shape[0] != nq or excl.stride(1) != 1:
        raise ValueError(f"exclude must be int64 [{nq}, E] with contiguous rows, got {tuple(excl.shape)}")
    out_keys = torch.empty((nq, k), dtype=torch.int64, device=dev) if want_keys or carry is None else None
    out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_carry = None if carry is None else torch.empty((nq, k), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().amdrec_exclude_compact(
        _lib.ptr(keys), _lib.ptr(scores), _lib.ptr(carry), nq, kc, _lib.ptr(excl), excl.shape[1],
        excl.stride(0) if nq > 1 else excl.shape[1], k, -1, fill_score, -1, _lib.ptr(out_keys), _lib.ptr(out_scores),
        _lib.ptr(out_carry), _lib.stream_ptr(dev)))
    return out_keys, out_scores, out_carry
