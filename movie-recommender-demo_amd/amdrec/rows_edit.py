"""Live corpus: the host helpers and binding calls behind ``FAISSIndex.remove_ids`` and ``AdRecommenderInference.remove_ads``
/ ``add_ads``.

Every per-ad structure of this package is a row array in insertion order, so removing ads is an order-preserving compaction
of a known set of tensors: ``amdrec_remove_plan`` (csrc/rows_edit.hip) turns the ascending list of ids to remove into
``kept``, the old positions of the rows that stay, and ``amdrec_rows_gather`` moves one array by it, byte for byte, whatever
its row format.  Nothing is recomputed, and nothing is written where it lies: a gather fills a NEW tensor that the owner then
swaps in, so a search in flight or a captured graph keeps reading the tensors it started with.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

MAX_ROWS = (1 << 31) - 1           # rows one amdrec_remove_plan call takes


def removal_list(ad_ids) -> np.ndarray:
    """The ids of a removal call (a sequence, a numpy array or a torch tensor of integers) -> int64, ascending, unique: the
    form amdrec_remove_plan searches.  TypeError for anything that is not an integer (bool included), ValueError for a
    negative id (no row has one: negative entries are the padding of the exclusion lists)."""
    if isinstance(ad_ids, torch.Tensor):
        ad_ids = ad_ids.detach().cpu().numpy()
    if isinstance(ad_ids, np.ndarray) and ad_ids.dtype != object:
        if ad_ids.dtype.kind not in "iu":
            raise TypeError(f"ad ids to remove must be integers, got an array of {ad_ids.dtype}")
        if ad_ids.dtype.kind == "u" and ad_ids.size and int(ad_ids.max()) > np.iinfo(np.int64).max:
            raise ValueError("ad ids to remove must fit int64")
        arr = ad_ids.astype(np.int64).ravel()
    else:
        vals = []
        for x in ([] if ad_ids is None else ad_ids):
            if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
                raise TypeError(f"ad ids to remove must be integers, got {x!r} ({type(x).__name__})")
            vals.append(int(x))
        arr = np.asarray(vals, dtype=np.int64)
    if arr.size and int(arr.min()) < 0:
        raise ValueError(f"ad ids to remove must be >= 0, got {int(arr.min())}")
    return np.unique(arr)


def remove_plan(ids: Optional[torch.Tensor], n: int, remove: torch.Tensor) -> torch.Tensor:
    """amdrec_remove_plan: ``ids`` int64 [>= n] on the device (None: a row's key is its position), ``remove`` device int64,
    ascending and unique (``removal_list``) -> ``kept`` int64 [n_kept], the old positions of the rows whose key is not in
    ``remove``, ascending.  Reads n_kept back: one host synchronisation."""
    n = int(n)
    dev = remove.device
    remove = _lib.require_gpu(remove, "remove", torch.int64).contiguous()
    if ids is not None:
        ids = _lib.require_gpu(ids, "ids", torch.int64)
        if ids.dim() != 1 or ids.shape[0] < n or (n and ids.stride(0) != 1):
            raise ValueError(f"ids must be a contiguous int64 vector of at least {n} entries")
    if n > MAX_ROWS:
        raise ValueError(f"{n} rows: a removal plan takes at most 2^31 - 1")
    lib = _lib.load()
    kept = torch.empty((n,), dtype=torch.int64, device=dev)
    n_kept = torch.zeros((1,), dtype=torch.int64, device=dev)
    nbytes = _lib.C.c_size_t(0)
    _lib.check(lib.amdrec_remove_plan_workspace(n, _lib.C.byref(nbytes)))
    ws = _lib.WORKSPACE.get(nbytes.value, dev)
    _lib.check(lib.amdrec_remove_plan(_lib.ptr(ids), n, _lib.ptr(remove), remove.numel(), _lib.ptr(kept), _lib.ptr(n_kept),
                                      _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return kept[:int(n_kept.item())]


def gather_rows(src: torch.Tensor, pos: torch.Tensor, n_src: Optional[int] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """amdrec_rows_gather: a NEW tensor (or ``out``, which must not share memory with ``src``) whose row j is row pos[j] of
    ``src[:n_src]``, byte for byte; a position outside [0, n_src) gives a row of zeros.  ``src``: a device tensor of any
    dtype whose rows (everything behind dim 0) are contiguous; its row pitch may be larger than a row."""
    src = _lib.require_gpu(src, "src")
    pos = _lib.require_gpu(pos, "pos", torch.int64).contiguous()
    row_shape = tuple(src.shape[1:])
    row_elems = int(np.prod(row_shape)) if row_shape else 1
    n_src = src.shape[0] if n_src is None else int(n_src)
    if src.dim() < 1 or n_src > src.shape[0] or not _rows_contiguous(src):
        raise ValueError("gather_rows needs a tensor [rows, ...] with contiguous rows and n_src <= rows")
    m = pos.numel()
    if out is None:
        out = torch.empty((m,) + row_shape, dtype=src.dtype, device=src.device)
    elif out.shape != (m,) + row_shape or out.dtype != src.dtype or not _rows_contiguous(out):
        raise ValueError("out must be [len(pos), ...] of src's dtype with contiguous rows")
    es = src.element_size()
    if m and row_elems:
        _lib.check(_lib.load().amdrec_rows_gather(
            _lib.ptr(src), _pitch(src, row_elems) * es, n_src, _lib.ptr(pos), m, row_elems * es, _lib.ptr(out),
            _pitch(out, row_elems) * es, _lib.stream_ptr(src.device)))
    return out


def _pitch(t: torch.Tensor, row_elems: int) -> int:
    """Elements from one row to the next (a tensor of at most one row has no pitch to speak of)."""
    return t.stride(0) if t.shape[0] > 1 else row_elems


def _rows_contiguous(t: torch.Tensor) -> bool:
    """Each row is one run of bytes, and the rows do not interleave."""
    if t.shape[0] == 0:
        return True
    row_elems = int(np.prod(t.shape[1:])) if t.dim() > 1 else 1
    return t[0:1].is_contiguous() and _pitch(t, row_elems) >= row_elems


def grown_copy(old: torch.Tensor, n_old: int, n_new: int) -> torch.Tensor:
    """A new tensor [n_new, ...] whose first n_old rows are a copy of ``old``'s (the appended rows are left to the caller)."""
    new = torch.empty((n_new,) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)
    new[:n_old].copy_(old[:n_old])
    return new


def plan_for(ids: Optional[torch.Tensor], n: int, remove_sorted: np.ndarray, device) -> Tuple[torch.Tensor, int]:
    """``remove_plan`` from the host list -> (kept, rows removed)."""
    kept = remove_plan(ids, n, torch.from_numpy(np.ascontiguousarray(remove_sorted, dtype=np.int64)).to(device))
    return kept, int(n) - int(kept.shape[0])
