"""ctypes binding of libamdrec.so (include/amdrec.h).

There is no CPU fallback: if the library is missing or a call fails this raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# AMDREC_LIB_PATH: developer override for A/B runs of two builds of the library in otherwise identical processes
LIB_PATH = os.environ.get("AMDREC_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "libamdrec.so")

ABI_VERSION = 14
MAX_K = 2048
MAX_INCLUDE = 64


class AmdrecError(RuntimeError):
    pass


_lib = None

_i64, _i32, _sz, _vp, _fp = C.c_int64, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p

# name -> argtypes (restype is int unless listed in _RESTYPE); mirrors include/amdrec.h
_SIGNATURES = {
    "amdrec_abi_version": [],
    "amdrec_last_error": [],
    "amdrec_flat_search_workspace": [_i64, _i64, _i32, C.POINTER(_sz)],
    "amdrec_bf16_rows": [_fp, _i64, _i64, _i32, _vp, _i64, _fp, _vp],
    "amdrec_flat_search_mixed_workspace": [_i64, _i64, _i32, _i32, C.POINTER(_sz)],
    "amdrec_flat_search_mixed": [_fp, _i64, _i64, _i32, _vp, _i64, _fp, _fp, _i64, _i64, _i32, _i64, _fp, _vp, _vp,
                                 _sz, _vp, _vp],
    "amdrec_flat_search": [_fp, _i64, _i64, _i32, _fp, _i64, _i64, _i32, _i64, _fp, _vp, _vp, _sz, _vp, _vp],
    "amdrec_flat_search_eligible": [_fp, _i64, _i64, _i32, _fp, _i64, _i64, _i32, _i64, _fp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "amdrec_flat_search_mixed_eligible": [_fp, _i64, _i64, _i32, _vp, _i64, _fp, _fp, _i64, _i64, _i32, _i64, _fp, _vp, _vp,
                                          _sz, _vp, _vp, _vp, _vp, _vp],
    # the *_boosted searches: their plain twin's arguments + (boost, weight, boost_max)
    "amdrec_flat_search_boosted": [_fp, _i64, _i64, _i32, _fp, _i64, _i64, _i32, _i64, _fp, _vp, _vp, _sz, _vp, _vp, _fp, _fp,
                                   C.c_float],
    "amdrec_flat_search_mixed_boosted": [_fp, _i64, _i64, _i32, _vp, _i64, _fp, _fp, _i64, _i64, _i32, _i64, _fp, _vp, _vp,
                                         _sz, _vp, _vp, _fp, _fp, C.c_float],
    "amdrec_ivf_scan": [_fp, _i64, _i32, _vp, _vp, _fp, _i64, _i64, _vp, _vp, _i32, _vp, _i64, _i64, _vp],
    "amdrec_ivf_scan_grouped": [_fp, _i64, _i32, _vp, _vp, _i32, _i64, _fp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i32,
                                _vp, _i64, _i64, _fp, _i64, _vp, _vp],
    "amdrec_ivf_filter_bounds": [_fp, _i64, _i64, _i32, _vp, _i64, _fp, _fp, _i64, _fp, _vp],
    "amdrec_ivf_scan_grouped_mixed": [_fp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _i64, _fp, _i64, _vp, _i64, _vp, _vp, _i64,
                                      _i32, _vp, _vp, _i64, _i64, _fp, _i64, _fp, _vp, _vp],
    # the *_eligible list scans: their plain twin's arguments + (list_tags, require_all, require_any)
    "amdrec_ivf_scan_eligible": [_fp, _i64, _i32, _vp, _vp, _fp, _i64, _i64, _vp, _vp, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _vp],
    "amdrec_ivf_scan_grouped_eligible": [_fp, _i64, _i32, _vp, _vp, _i32, _i64, _fp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _vp,
                                         _i32, _vp, _i64, _i64, _fp, _i64, _vp, _vp, _vp, _vp, _vp],
    "amdrec_ivf_scan_grouped_mixed_eligible": [_fp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _i64, _fp, _i64, _vp, _i64, _vp, _vp,
                                               _i64, _i32, _vp, _vp, _i64, _i64, _fp, _i64, _fp, _vp, _vp, _vp, _vp, _vp],
    # the *_boosted list scans: their twin's arguments + (list_boosts, weight); the boosted bound: + (weight, boost_max)
    "amdrec_ivf_scan_boosted": [_fp, _i64, _i32, _vp, _vp, _fp, _i64, _i64, _vp, _vp, _i32, _vp, _i64, _i64, _vp, _fp, _fp],
    "amdrec_ivf_scan_eligible_boosted": [_fp, _i64, _i32, _vp, _vp, _fp, _i64, _i64, _vp, _vp, _i32, _vp, _i64, _i64, _vp, _vp, _vp,
                                         _vp, _fp, _fp],
    "amdrec_ivf_scan_grouped_boosted": [_fp, _i64, _i32, _vp, _vp, _i32, _i64, _fp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _vp,
                                        _i32, _vp, _i64, _i64, _fp, _i64, _vp, _vp, _fp, _fp],
    "amdrec_ivf_scan_grouped_eligible_boosted": [_fp, _i64, _i32, _vp, _vp, _i32, _i64, _fp, _i64, _vp, _vp, _i64, _i32, _vp, _vp,
                                                 _vp, _i32, _vp, _i64, _i64, _fp, _i64, _vp, _vp, _vp, _vp, _vp, _fp, _fp],
    "amdrec_ivf_filter_bounds_boosted": [_fp, _i64, _i64, _i32, _vp, _i64, _fp, _fp, _i64, _fp, _vp, _fp, C.c_float],
    "amdrec_ivf_scan_grouped_mixed_boosted": [_fp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _i64, _fp, _i64, _vp, _i64, _vp, _vp,
                                              _i64, _i32, _vp, _vp, _i64, _i64, _fp, _i64, _fp, _vp, _vp, _fp, _fp],
    "amdrec_ivf_scan_grouped_mixed_eligible_boosted": [_fp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _i64, _fp, _i64, _vp, _i64, _vp,
                                                       _vp, _i64, _i32, _vp, _vp, _i64, _i64, _fp, _i64, _fp, _vp, _vp, _vp, _vp,
                                                       _vp, _fp, _fp],
    "amdrec_ivfpq_scan_finite_eligible": [_vp, _i32, _vp, _vp, _vp, _i32, _i64, _fp, _i32, _vp, _vp, _i64, _i32, _vp, _vp, _vp,
                                          _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp],
    "amdrec_ivf_select": [_vp, _i64, _vp, _i64, _i32, _fp, _vp, _vp],
    "amdrec_ivf_select_split": [_vp, _i64, _vp, _i64, _i32, _i32, _fp, _vp, _vp, _sz, _vp, _vp],
    "amdrec_ivf_coarse_keys": [_fp, _i32, _i64, _i32, _fp, _i64, _i64, _vp, _i64, _vp],
    # amdrec_ivf_coarse_keys' arguments up to ld_keys + (list_len, tag_or, require_all, require_any, boost_hi, boost_lo, weight)
    "amdrec_ivf_coarse_keys_aware": [_fp, _i32, _i64, _i32, _fp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _fp, _fp, _fp, _vp],
    "amdrec_ivf_list_summaries": [_vp, _i32, _vp, _fp, _vp, _fp, _fp, _vp],
    "amdrec_ivf_group": [_vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _sz, _vp],
    "amdrec_ivf_assign": [_fp, _i64, _i64, _i32, _fp, _i32, _i64, _vp, _fp, _vp, _sz, _vp],
    "amdrec_ivf_kmeans_workspace": [_i64, _i32, _i32, C.POINTER(_sz)],
    "amdrec_ivf_kmeans_step": [_fp, _i64, _i64, _i32, _fp, _i32, _i64, _vp, _sz, _vp],
    "amdrec_ivfpq_encode": [_fp, _i64, _i64, _i32, _vp, _fp, _i64, _i32, _fp, _i32, _vp, _vp],
    "amdrec_ivfpq_train_workspace": [_i64, _i32, _i32, C.POINTER(_sz)],
    "amdrec_ivfpq_train_step": [_fp, _i64, _i64, _i32, _vp, _fp, _i64, _i32, _fp, _i32, _vp, _sz, _vp],
    "amdrec_ivfpq_tables": [_fp, _i64, _i64, _i32, _vp, _i64, _i32, _fp, _i64, _i32, _fp, _i32, _fp, _vp],
    "amdrec_ivfpq_scan": [_vp, _i32, _vp, _vp, _i32, _i64, _fp, _i32, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _i64,
                          _i64, _vp],
    "amdrec_ivfpq_scan_finite": [_vp, _i32, _vp, _vp, _vp, _i32, _i64, _fp, _i32, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp,
                                 _i64, _i64, _vp],
    "amdrec_ivfpq_distances": [_fp, _i64, _i32, _fp, _vp],
    "amdrec_ivfpq_rerank": [_vp, _i32, _i64, _i64, _i32, _vp, _fp, _i64, _i64, _vp, _i32, _i64, _i32, _fp, _vp, _vp, _sz, _vp,
                            _vp],
    "amdrec_topk_merge": [_fp, _vp, _i32, _i64, _i64, _i64, _i32, _fp, _vp, _vp],
    "amdrec_topk_merge_partial": [_fp, _vp, _i32, _i32, _i64, _i64, _i64, _i32, _fp, _vp, _vp, _vp],
    "amdrec_tower_workspace": [_vp, _i64, C.POINTER(_sz)],
    "amdrec_tower_forward": [_vp, _vp, _fp, _i64, _fp, _i64, _vp, _vp, _sz, _vp],
    "amdrec_ranker_workspace": [_vp, _i64, C.POINTER(_sz)],
    "amdrec_ranker_forward": [_vp, _vp, _fp, _i64, _vp, _vp, _i64, _fp, _i64, _vp, _i64, _i64, _vp, _sz, _vp],
    "amdrec_ranker_forward_ctr_first": [_vp, _vp, _fp, _i64, _vp, _vp, _i64, _fp, _i64, _vp, _i64, _i64, _fp, _i64, _vp, _sz, _vp],
    "amdrec_ranker_ctr_first_supported": [_vp, _i64],
    "amdrec_ranker_winner_heads": [_vp, _fp, _i64, _i64, _vp, _i64, _i32, _i32, _fp, _vp, _sz, _vp],
    "amdrec_ranker_ctr_first_workspace": [_vp, _i64, _i64, C.POINTER(_sz)],
    "amdrec_l2_normalize": [_fp, _i64, _fp, _i64, _i64, _i32, _vp],
    "amdrec_remap_ids": [_vp, _vp, _i64, _vp, _i64, _vp],
    "amdrec_exclude_compact": [_vp, _fp, _vp, _i64, _i32, _vp, _i32, _i64, _i32, _i64, C.c_float, _i64, _vp, _fp, _vp, _vp],
    # (pos, scores, nq, k, include, n_include, ld_include, X, ldx, n_rows, d, Q, ldq, tags, require_all, require_any, exclude,
    # n_exclude, ld_exclude, ids, boosts, boost_w, out_pos, out_scores, out_injected, stream)
    "amdrec_include_merge": [_vp, _fp, _i64, _i32, _vp, _i32, _i64, _fp, _i64, _i64, _i32, _fp, _i64, _vp, _vp, _vp, _vp, _i32,
                             _i64, _vp, _fp, _fp, _vp, _fp, _vp, _vp],
    "amdrec_remove_plan_workspace": [_i64, C.POINTER(_sz)],
    "amdrec_remove_plan": [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _sz, _vp],
    "amdrec_rows_gather": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp],
    "amdrec_profile_enable": [_i32],
    "amdrec_profile_only": [C.c_char_p],
    "amdrec_profile_report": [_vp, _i32, C.POINTER(_i32)],
    "amdrec_ranker_project_ads": [_vp, _vp, _i64, _fp, _i64, _vp, _sz, _vp],
    "amdrec_ranker_project_ads_hidden": [_vp, _vp, _i64, _fp, _i64, _vp, _sz, _vp],
    "amdrec_ranker_x3_prefix": [_vp, _fp, _i64, _i64, _i32, _fp, _i64, _fp, _i64, _vp, _sz, _vp],
    "amdrec_prep_numerical": [_fp, _fp, _fp, _fp, _i64, _i32, _vp],
    "amdrec_select_topk": [_fp, _i64, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _vp, _fp, _vp, _vp],
    # amdrec_select_topk's arguments up to out_slots + (group_of, n_group_rows, max_per_group, stream)
    "amdrec_select_topk_capped": [_fp, _i64, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _vp, _fp, _vp, _vp, _i64, _i32, _vp],
    # amdrec_select_topk's arguments up to top_k + (bid_of, n_bid_rows, reserve, group_of, n_group_rows, max_per_group),
    # its outputs + (out_ecpm, out_price, stream)
    "amdrec_select_topk_auction": [_fp, _i64, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _fp, _i64, _fp, _vp, _i64, _i32, _vp, _fp,
                                   _vp, _fp, _fp, _vp],
    # amdrec_select_topk's arguments up to top_k + (rows, n_rows, ld_rows, dim, lam, pool, group_of, n_group_rows,
    # max_per_group), its outputs + (out_values, stream)
    "amdrec_select_topk_diverse": [_fp, _i64, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _fp, _i64, _i64, _i32, C.c_float, _i32,
                                   _vp, _i64, _i32, _vp, _fp, _vp, _fp, _vp],
    # (logits, ld, n_tasks, cand_ids, cand_pos, n_users, k_c, top_k, weights, group_of, n_group_rows, max_per_group, out_ids,
    # out_scores, out_slots, out_values, stream)
    "amdrec_select_topk_value": [_fp, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _fp, _vp, _i64, _i32, _vp, _fp, _vp, _fp, _vp],
    # the same with rank_task behind n_tasks, (bid_of, n_bid_rows, reserve) behind weights and (out_ecpm, out_price) behind
    # out_values
    "amdrec_select_topk_value_auction": [_fp, _i64, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _fp, _fp, _i64, _fp, _vp, _i64, _i32,
                                         _vp, _fp, _vp, _fp, _fp, _fp, _vp],
    # amdrec_select_topk_capped's arguments up to max_per_group + (temperature, seeds, greedy, out_propensity, stream)
    "amdrec_select_topk_sampled": [_fp, _i64, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _vp, _fp, _vp, _vp, _i64, _i32, _fp, _vp,
                                   _i32, _fp, _vp],
    "amdrec_group_cap_compact": [_vp, _fp, _i64, _i32, _vp, _i64, _i32, _i32, C.c_float, _vp, _fp, _vp],
}
_RESTYPE = {"amdrec_last_error": C.c_char_p}


def exported_symbols():
    return list(_SIGNATURES)


def load():
    """Load libamdrec.so once; raise (never fall back) if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmdrecError(
            f"{LIB_PATH} not found: build it with `python movie-recommender-demo_amd/build.py` "
            "(there is no CPU fallback for the HIP path)")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name)       # AttributeError if the symbol is missing
        fn.argtypes = argtypes
        fn.restype = _RESTYPE.get(name, C.c_int)
    v = lib.amdrec_abi_version()
    if v != ABI_VERSION:
        raise AmdrecError(f"libamdrec ABI {v} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


_tls = threading.local()          # .prev_device: the thread's HIP device before stream_ptr() switched it (else None)


def check(status):
    """Status check of a C call - and the end of the call's device scope: if ``stream_ptr`` switched the calling
    thread's current HIP device for this call, switch it back (a call on a tensor that lives on cuda:N must not leave
    the caller's later ``device='cuda'`` allocations and launches on cuda:N)."""
    prev = getattr(_tls, "prev_device", None)
    if prev is not None:
        _tls.prev_device = None
        torch.cuda.set_device(prev)
    if status != 0:
        msg = load().amdrec_last_error()
        raise AmdrecError(f"libamdrec error {status}: {msg.decode() if msg else '?'}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    """hipStream_t of torch's current stream on ``device`` - and make ``device`` the calling thread's current HIP
    device for the duration of ONE C call: the C entry points launch kernels, set function attributes and memset on the
    CURRENT device (amdrec.h), so a tensor on cuda:N (N != 0), or a call from a fresh thread (whose current device is
    0), must switch first.  Every binding call site evaluates this as the last argument of ``check(lib.fn(...,
    stream_ptr(dev)))``: the switch happens right before the C call and ``check`` restores the previous device right
    after it, so the caller's current device is unchanged by an amdrec call."""
    cur = torch.cuda.current_device()
    idx = cur
    if device is not None:
        dev = device if isinstance(device, torch.device) else torch.device(device)
        if dev.type == "cuda" and dev.index is not None:
            idx = dev.index
            if idx != cur:
                if getattr(_tls, "prev_device", None) is None:
                    _tls.prev_device = cur
                torch.cuda.set_device(dev)
    # the raw handle straight from the C side: torch.cuda.current_stream() builds a Stream object through three layers of
    # device-index parsing - 5 us per call, nine calls per request (a seventh of a single request's host time)
    return C.c_void_p(_raw_stream(idx))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda i: torch.cuda.current_stream(i).cuda_stream)


def require_gpu(t, name, dtype=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise AmdrecError(f"{name} must be a tensor on a HIP device (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise AmdrecError(f"{name} must be {dtype}, got {t.dtype}")
    return t


class ProfileEntry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_int64), ("total_ms", C.c_double),
                ("flops", C.c_double), ("bytes", C.c_double)]


def profile_enable(on: bool, only: str = ""):
    """Per-launch HIP-event timing on / off (clears the counters); ``only``: time just the tags with this prefix."""
    check(load().amdrec_profile_only(only.encode() if only else None))
    check(load().amdrec_profile_enable(1 if on else 0))


def profile_report():
    """-> {tag: dict(launches, total_ms, flops, bytes)} (synchronises with the recorded events)."""
    arr = (ProfileEntry * 64)()
    n = C.c_int(0)
    check(load().amdrec_profile_report(C.cast(arr, C.c_void_p), 64, C.byref(n)))
    return {arr[i].name.decode(): {"launches": arr[i].launches, "total_ms": arr[i].total_ms,
                                   "flops": arr[i].flops, "bytes": arr[i].bytes} for i in range(n.value)}


# Every registration of a Parameter / buffer / submodule on ANY nn.Module bumps this epoch (torch's global registration
# hooks: `module.weight = nn.Parameter(...)`, `load_state_dict(assign=True)` on a child and parametrize all go through
# register_parameter; assigning to an existing buffer name calls the buffer hooks).  One integer compare per forward tells
# tensor_versions() whether some tensor OBJECT may have been replaced since it cached its list.
_REG_EPOCH = [0]


def _bump_registration_epoch(*_args):
    _REG_EPOCH[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_bump_registration_epoch)
torch.nn.modules.module.register_module_buffer_registration_hook(_bump_registration_epoch)
torch.nn.modules.module.register_module_module_registration_hook(_bump_registration_epoch)


def tensor_versions(module) -> tuple:
    """``_version`` of every parameter and buffer of ``module`` - the part of the drop-ins' packing-cache key that detects
    in-place weight updates (optimizer steps, ``copy_``).  The tensor list itself is cached on the module: walking
    ``parameters()`` on every call cost 0.1 ms per forward on the serving path (a fifth of a single request).  The cache is
    dropped by the drop-ins' ``_apply`` / ``load_state_dict`` / ``invalidate``, and re-walked whenever any Parameter, buffer
    or submodule has been (re-)registered anywhere since it was taken (``_REG_EPOCH``): a REPLACED Parameter object is
    seen - the new tensor's identity enters the key - and the replaced tensors are released."""
    d = module.__dict__
    tl = d.get("_amdrec_tensor_list")
    if tl is None or d.get("_amdrec_tensor_epoch") != _REG_EPOCH[0]:
        tl = [*module.parameters(), *module.buffers()]
        d["_amdrec_tensor_list"] = tl
        d["_amdrec_tensor_epoch"] = _REG_EPOCH[0]
        d["_amdrec_tensor_ids"] = hash(tuple(id(t) for t in tl))
    return (d["_amdrec_tensor_ids"], *[t._version for t in tl])


def drop_tensor_list(module):
    module.__dict__.pop("_amdrec_tensor_list", None)


def copyable_state(module, derived=("_packed", "_ad_cache")) -> dict:
    """``__getstate__`` of the drop-ins: the module's ``__dict__`` without its derived state.  The packed weights hold a
    ctypes structure of raw device pointers (not picklable, and a copy must not point into the original's buffers), the
    per-ad caches belong to the original's pack, and the cached tensor list names the ORIGINAL's tensors: a copy
    (``copy.deepcopy``, ``pickle``, ``torch.save`` of the whole module) starts with none of them and packs for itself on
    first use."""
    state = dict(module.__dict__)
    for name in ("_amdrec_tensor_list", "_amdrec_tensor_epoch", "_amdrec_tensor_ids", "_ctr_first_why"):
        state.pop(name, None)
    for name in derived:
        if name in state:
            state[name] = None
    return state


class Workspace:
    """Grow-only per-device scratch buffer handed to the C ABI (caller-owned workspace).

    Kernels launched on one stream use it one after the other, so a single buffer per device is enough
    for eager calls.  A captured HIP graph bakes the buffer's address into its kernel nodes, so it must
    never share (or outlive) a buffer that may be re-allocated: ``private()`` installs a separate,
    pre-sized arena for the duration of a capture and the graph owner keeps it alive."""

    def __init__(self):
        self._buf = {}
        self._override = None

    def get(self, nbytes, device):
        if self._override is not None:
            return self._override.get(nbytes, device)
        key = torch.device(device)
        if key.index is None and key.type == "cuda":
            key = torch.device("cuda", torch.cuda.current_device())
        buf = self._buf.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = None
            self._buf[key] = None
            buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=key)
            assert buf.data_ptr() % 256 == 0
            self._buf[key] = buf
        return buf

    def private(self, arena: "FixedArena"):
        ws = self

        class _Ctx:
            def __enter__(self_):
                self_.prev, ws._override = ws._override, arena
                return arena

            def __exit__(self_, *exc):
                ws._override = self_.prev
                return False
        return _Ctx()


class FixedArena:
    """A workspace of fixed size that refuses to grow (for graph capture)."""

    def __init__(self, nbytes, device):
        self.buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        self.high_water = 0

    def get(self, nbytes, device):
        self.high_water = max(self.high_water, int(nbytes))
        if nbytes > self.buf.numel():
            raise AmdrecError(f"graph workspace too small: need {nbytes} bytes, have {self.buf.numel()}")
        return self.buf


class MeasuringArena:
    """Records the largest request while delegating to the shared workspace (sizing pass)."""

    def __init__(self, inner):
        self.inner, self.high_water = inner, 0

    def get(self, nbytes, device):
        self.high_water = max(self.high_water, int(nbytes))
        return self.inner.get(nbytes, device)


WORKSPACE = Workspace()


class Gate:
    """What threads that share the library must agree on, process-wide like the workspace it protects.

    ``enqueue`` (a re-entrant lock): held while a call enqueues its device work.  The launches of one call write and read
    the shared workspace one after the other on one stream; launches of two calling threads interleaved on that stream would
    read each other's intermediate results.  Lazily built state (packed weights, per-ad caches, limits) is built under it
    too.  The serving entry points of ``AdRecommenderInference`` take it themselves - around the enqueue only, not around
    their host work or their wait for the device; whoever drives models or an index directly from several threads takes it
    around each call.

    ``serving()`` / ``capturing()``: a graph capture swaps the workspace for a private arena (``Workspace.private``) and
    puts the runtime into its global capture mode, in which another thread's event wait or copy invalidates the capture: it
    cannot run beside serving calls of other threads.  Neither waits for the other; the one that comes second raises
    AmdrecError, before it has touched the device."""

    def __init__(self):
        self.enqueue = threading.RLock()
        self._mu = threading.Lock()
        self._calls = {}              # thread ident -> depth of its serving calls in flight
        self._capturer = None         # thread ident of the capturing thread, and ...
        self._capture_depth = 0       # ... the depth of its captures
        # (the scopes hold no state of their own: one object each serves every call - the serving path pays no allocation)
        self._serving, self._capturing = _Scope(self._enter_call, self._exit_call), _Scope(self._enter_capture, self._exit_capture)

    def serving(self):
        return self._serving

    def capturing(self):
        return self._capturing

    def _enter_call(self):
        me = threading.get_ident()
        with self._mu:
            if self._capturer is not None and self._capturer != me:
                raise AmdrecError("a graph capture is in progress on another thread: serving calls cannot run beside capture() "
                                  "(INTEGRATION.md, threads)")
            self._calls[me] = self._calls.get(me, 0) + 1

    def _exit_call(self):
        me = threading.get_ident()
        with self._mu:
            left = self._calls[me] - 1
            if left:
                self._calls[me] = left
            else:
                del self._calls[me]

    def _enter_capture(self):
        me = threading.get_ident()
        with self._mu:
            if (self._capturer is not None and self._capturer != me) or any(t != me for t in self._calls):
                raise AmdrecError("capture() while other threads are serving or capturing: a graph capture swaps the process-wide "
                                  "workspace and the runtime's capture mode is global (INTEGRATION.md, threads)")
            self._capturer = me
            self._capture_depth += 1

    def _exit_capture(self):
        with self._mu:
            self._capture_depth -= 1
            if not self._capture_depth:
                self._capturer = None


class _Scope:
    __slots__ = ("_enter", "_exit")

    def __init__(self, enter, exit_):
        self._enter, self._exit = enter, exit_

    def __enter__(self):
        self._enter()

    def __exit__(self, *exc):
        self._exit()
        return False


GATE = Gate()
