"""Per-group caps ("at most c ads of one advertiser in an answer, whichever c rank best").

Every ad may carry one int64 GROUP key (advertiser, campaign: the caller decides; ``FAISSIndex.add(groups=)`` /
``set_groups``); a negative key means ungrouped, never capped; an ad that was never given one has -1.  The rule is greedy in
rank order: an entry is accepted while fewer than ``c`` accepted entries share its group.  That equals "keep an entry iff
fewer than ``c`` better-ranked entries have its group, then cut to k": an entry's fate depends only on its own group's
prefix, so the kernels decide every entry in parallel, on the device.

* Stage 2 (``max_per_group``): ``amdrec_select_topk_capped`` visits a user's candidates in the selection's order (CTR logit
  descending, slot ascending, NaN logits last; unfilled slots are no candidates) and reports the first ``top_k`` accepted
  ones.  A short result means the user's candidate list holds fewer than ``top_k`` ads the cap lets through.
* Stage 1 (``FAISSIndex.search_device(max_per_group=, group_overfetch=)``): the index's own search for
  ``K1 = min(k * group_overfetch, AMDREC_MAX_K - E)`` positions (E: the width of an exclusion list, 0 without one), masks and
  exclusion included, then ``amdrec_group_cap_compact`` to ``k``.  The result is BY DEFINITION the rule applied to the
  index's own top-``K1``, for Flat, IVF and IVFPQ alike, with or without refine: a row can come back short although the
  corpus holds more ads of other groups further down than ``K1``.

This module holds the host helpers (no GPU needed) and the binding call of the compaction.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def check_cap(max_per_group, what: str = "max_per_group") -> int:
    """A cap as the entries take it: an integer in [1, AMDREC_MAX_K] (larger values are clamped: no list is longer)."""
    if isinstance(max_per_group, (bool, np.bool_)) or not isinstance(max_per_group, (int, np.integer)):
        raise TypeError(f"{what} must be an integer, got {max_per_group!r} ({type(max_per_group).__name__})")
    if max_per_group <= 0:
        raise ValueError(f"{what} must be >= 1, got {int(max_per_group)}")
    return min(int(max_per_group), _lib.MAX_K)


def overfetch_k(k: int, group_overfetch: int, E: int = 0) -> int:
    """-> K1 = min(k * group_overfetch, AMDREC_MAX_K - E), the positions the capped search asks the index for; ValueError
    when that is fewer than k (k + E exceeds AMDREC_MAX_K) or group_overfetch < 1."""
    k, E = int(k), int(E)
    if isinstance(group_overfetch, (bool, np.bool_)) or not isinstance(group_overfetch, (int, np.integer)) or group_overfetch < 1:
        raise ValueError(f"group_overfetch must be an integer >= 1, got {group_overfetch!r}")
    if k < 1:
        raise ValueError(f"k must be >= 1, got {k}")
    k1 = min(k * int(group_overfetch), _lib.MAX_K - E)
    if k1 < k:
        raise ValueError(f"a capped search for k = {k} with an exclusion list of E = {E} entries needs k + E <= AMDREC_MAX_K = "
                         f"{_lib.MAX_K}: the index can be asked for at most AMDREC_MAX_K - E = {_lib.MAX_K - E} positions")
    return k1


def as_keys(groups, n: int) -> np.ndarray:
    """``n`` group keys as int64 (numpy [n]): a sequence of Python ints, an integer numpy array or an integer torch tensor.
    Floats, bools and a length other than n are refused."""
    n = int(n)
    if isinstance(groups, torch.Tensor):
        if groups.is_floating_point() or groups.is_complex() or groups.dtype == torch.bool:
            raise TypeError(f"group keys must be integers, got {groups.dtype}")
        groups = groups.detach().cpu().numpy()
    if isinstance(groups, np.ndarray) and groups.dtype != object:
        if groups.dtype.kind not in "iu":
            raise TypeError(f"group keys must be integers, got an array of {groups.dtype}")
        if groups.dtype.kind == "u" and groups.size and int(groups.max()) > np.iinfo(np.int64).max:
            raise ValueError("group keys must fit int64")
        out = np.ascontiguousarray(groups, dtype=np.int64)
    else:
        vals = []
        for v in groups:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"group keys must be integers, got {v!r} ({type(v).__name__})")
            if not -(1 << 63) <= int(v) < (1 << 63):
                raise ValueError(f"group key {v} does not fit int64")
            vals.append(int(v))
        out = np.asarray(vals, dtype=np.int64)
    if out.shape != (n,):
        raise ValueError(f"expected {n} group keys, got an array of shape {tuple(out.shape)}")
    return out


def device_keys(groups, n: int, device) -> torch.Tensor:
    """as_keys on the device (a device int64 tensor of the right length is taken as it is)."""
    if isinstance(groups, torch.Tensor) and groups.is_cuda and groups.dtype == torch.int64:
        if groups.shape != (n,):
            raise ValueError(f"expected {n} group keys, got a tensor of shape {tuple(groups.shape)}")
        return groups.contiguous()
    return torch.from_numpy(as_keys(groups, n)).to(device)


def compact(pos: torch.Tensor, scores: torch.Tensor, group_of: torch.Tensor, n_rows: int, max_per_group: int, k: int,
            fill_score: float):
    """amdrec_group_cap_compact on device tensors: ``pos`` int64 / ``scores`` float32 [nq, kc] in the index's order,
    ``group_of`` int64 [>= n_rows] -> (pos, scores), each [nq, k].  Unfilled slots: -1 / ``fill_score``."""
    pos = _lib.require_gpu(pos, "pos", torch.int64).contiguous()
    scores = _lib.require_gpu(scores, "scores", torch.float32).contiguous()
    group_of = _lib.require_gpu(group_of, "group_of", torch.int64)
    if pos.dim() != 2 or scores.shape != pos.shape:
        raise ValueError(f"pos and scores must both be [nq, kc], got {tuple(pos.shape)} and {tuple(scores.shape)}")
    if group_of.dim() != 1 or group_of.shape[0] < n_rows or not group_of.is_contiguous():
        raise ValueError(f"group_of must be a contiguous int64 vector of at least {n_rows} keys, got {tuple(group_of.shape)}")
    nq, kc = pos.shape
    dev = pos.device
    out_pos = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().amdrec_group_cap_compact(
        _lib.ptr(pos), _lib.ptr(scores), nq, kc, _lib.ptr(group_of), int(n_rows), int(max_per_group), int(k), fill_score,
        _lib.ptr(out_pos), _lib.ptr(out_scores), _lib.stream_ptr(dev)))
    return out_pos, out_scores
