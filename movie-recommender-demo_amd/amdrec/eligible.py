"""Per-request eligibility masks ("only the ads this request may be shown": geo, device and placement targeting, paused
campaigns, brand-safety classes).

Contract (Flat index, both engines, every dimension; an IVF / IVFPQ index constructed with ``list_tags=True`` applies the same
predicate inside its list scans and returns its own result restricted to eligible rows).  Every ad carries one 64-bit TAG word; the library does not interpret
it, the caller assigns the bits; an ad that was never given a tag has tag 0.  Every query carries two 64-bit words,
``require_all`` and ``require_any``.  Row ``r`` is eligible for query ``q`` iff

    (tags[r] & all[q]) == all[q]   and   (any[q] == 0 or (tags[r] & any[q]) != 0)

so ``all = any = 0`` admits every row.  The result for ``(q, k)`` is the exact top-k of the query's eligible rows in the
search's own total order (score descending, ties to the lower position), with the scores the plain search returns for those
rows; a row whose score is NaN is never returned; with fewer than ``k`` eligible rows the tail is unfilled as Flat writes
unfilled slots (-inf, position -1).  Unlike an exclusion list (amdrec.exclude: a post-filter, k + E <= AMDREC_MAX_K) the
predicate is tested inside the corpus pass where a row enters the candidate pool, so the number of ineligible rows is not
limited.  With ``exclude`` the filtered search runs for k + E and the usual compaction follows.

Words travel as int64 holding the bit pattern (torch has no usable uint64): bit 63 set reads as a negative number.  This
module holds the host helpers (no GPU needed).
"""
from __future__ import annotations

import numpy as np
import torch

_U64 = (1 << 64) - 1


def as_words(x, n: int) -> np.ndarray:
    """``n`` 64-bit words as int64 bit patterns (numpy [n]).  ``x``: one Python int (given to all n) or a sequence of them,
    0 <= v < 2**64, or negative down to -2**63 (already a bit pattern); a numpy uint64 / int64 array; a torch int64 tensor.
    Floats, bools, other dtypes and a length other than n are refused."""
    n = int(n)
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.int64:
            raise TypeError(f"64-bit words must be torch.int64, got {x.dtype}")
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray) and x.dtype != object:
        if x.dtype not in (np.dtype(np.uint64), np.dtype(np.int64)):
            raise TypeError(f"64-bit words must be uint64 or int64, got {x.dtype}")
        out = np.ascontiguousarray(x).view(np.int64).reshape(-1) if x.ndim else np.full(n, x.astype(np.uint64).view(np.int64))
    else:
        seq = [x] * n if isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)) else list(x)
        vals = []
        for v in seq:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"64-bit words must be integers, got {v!r} ({type(v).__name__})")
            v = int(v)
            if not -(1 << 63) <= v <= _U64:
                raise ValueError(f"{v} does not fit 64 bits")
            vals.append(v & _U64)
        out = np.array(vals, dtype=np.uint64).view(np.int64)
    if out.shape != (n,):
        raise ValueError(f"expected {n} words, got {out.size}")
    return out


def eligible(tags, require_all, require_any) -> np.ndarray:
    """The contract in numpy: tags [n], require_all / require_any [nq] (anything as_words takes) -> bool [nq, n]."""
    t = as_words(tags, len(tags)).view(np.uint64)[None, :]
    a = as_words(require_all, len(require_all)).view(np.uint64)[:, None]
    y = as_words(require_any, len(require_any)).view(np.uint64)[:, None]
    return ((t & a) == a) & ((y == 0) | ((t & y) != 0))


def device_words(x, n: int, device) -> torch.Tensor:
    """as_words on the device (a device int64 tensor of the right length is taken as it is)."""
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int64:
        if x.shape != (n,):
            raise ValueError(f"expected {n} words, got {tuple(x.shape)}")
        return x.contiguous()
    return torch.from_numpy(as_words(x, n)).to(device)


def device_masks(require_all, require_any, nq: int, device):
    """The two mask arguments of a search -> (all, any) device int64 [nq], or (None, None) when neither is given; where one
    is given the other defaults to 0."""
    if require_all is None and require_any is None:
        return None, None
    return (device_words(0 if require_all is None else require_all, nq, device),
            device_words(0 if require_any is None else require_any, nq, device))
