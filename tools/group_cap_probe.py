"""Dev tool: what the per-group caps cost on the device.  In ONE process, after a warm-up, alternating over REPS repeats (each
a HIP-event pair around ITERS back-to-back launches, divided by ITERS):
  stage 2 at the serving shape (512 users x 500 candidates, top 10): amdrec_select_topk of this build, amdrec_select_topk of a
  second build of the library if one is given (--parent-lib: the parent commit's build, loaded next to this one), and
  amdrec_select_topk_capped with cap 2 over group keys of which every user's candidates hold ~8 per advertiser;
  the general path of the two (513 candidates, top 10) the same way;
  stage 1: amdrec_group_cap_compact 512 x 1000 -> 500, cap 3, against amdrec_exclude_compact 512 x 1000 -> 500 with a
  64-entry list (the launch the exclusion path pays at the same shape).
The spread is (max - min) / median over the repeats of one cell.
usage: python tools/group_cap_probe.py [--out FILE] [--parent-lib PATH] [--reps R] [--iters N]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--iters", type=int, default=50)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommender-demo_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from amdrec import _lib  # noqa: E402


def stats(us):
    med = statistics.median(us)
    return {"median_us": round(med, 3), "min_us": round(min(us), 3), "max_us": round(max(us), 3),
            "spread": round((max(us) - min(us)) / med, 4), "repeats": len(us)}


def event_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def alternate(cells):
    """{name: launch} -> {name: stats}: one warm-up round, then REPS rounds that visit every cell in turn."""
    for name, fn in cells.items():
        assert fn() == 0, (name, _lib.load().amdrec_last_error())
        event_us(fn, 3)
    times = {name: [] for name in cells}
    for _ in range(ARGS.reps):
        for name, fn in cells.items():
            times[name].append(event_us(fn, ARGS.iters))
    return {name: stats(t) for name, t in times.items()}


def select_cells(lib, parent, users, k_c, top_k, cap, n_ads=1_000_000, n_groups=60):
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(users + k_c)
    logits = torch.randn((3, users * k_c), generator=g, device=dev)
    pos = torch.randint(0, n_ads, (users, k_c), generator=g, device=dev)
    groups = torch.randint(0, n_groups, (n_ads,), generator=g, device=dev)
    ids = torch.empty((users, top_k), dtype=torch.int64, device=dev)
    sc = torch.empty((3, users, top_k), dtype=torch.float32, device=dev)
    keep = (logits, pos, groups, ids, sc)
    st = _lib.stream_ptr(dev)
    head = (_lib.ptr(logits), logits.stride(0), 3, 0, _lib.ptr(pos), _lib.ptr(pos), users, k_c, top_k, _lib.ptr(ids),
            _lib.ptr(sc), None)
    cells = {"select_topk": lambda: lib.amdrec_select_topk(*head, st)}
    if parent is not None:
        cells["select_topk_parent_build"] = lambda: parent.amdrec_select_topk(*head, st)
    cells["select_topk_capped"] = lambda: lib.amdrec_select_topk_capped(*head, _lib.ptr(groups), n_ads, cap, st)
    res = alternate(cells)
    base = res["select_topk_parent_build" if parent is not None else "select_topk"]["median_us"]
    res["capped_over_uncapped"] = round(res["select_topk_capped"]["median_us"] / base, 3)
    res["shape"] = {"users": users, "candidates": k_c, "top_k": top_k, "cap": cap, "groups": n_groups}
    del keep
    return res


def compact_cells(lib, nq, kc, k, cap, n_ads=1_000_000, n_groups=200, E=64):
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(nq + kc)
    pos = torch.randint(0, n_ads, (nq, kc), generator=g, device=dev)
    scores = torch.sort(torch.randn((nq, kc), generator=g, device=dev), dim=1, descending=True)[0].contiguous()
    groups = torch.randint(0, n_groups, (n_ads,), generator=g, device=dev)
    excl = pos[:, torch.randperm(kc, device=dev)[:E]].contiguous()
    out_pos = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_sc = torch.empty((nq, k), dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)
    ninf = float("-inf")
    cells = {
        "group_cap_compact": lambda: lib.amdrec_group_cap_compact(_lib.ptr(pos), _lib.ptr(scores), nq, kc, _lib.ptr(groups),
                                                                  n_ads, cap, k, ninf, _lib.ptr(out_pos), _lib.ptr(out_sc), st),
        "exclude_compact": lambda: lib.amdrec_exclude_compact(_lib.ptr(pos), _lib.ptr(scores), None, nq, kc, _lib.ptr(excl), E, E,
                                                              k, -1, ninf, -1, _lib.ptr(out_pos), _lib.ptr(out_sc), None, st),
    }
    res = alternate(cells)
    res["shape"] = {"queries": nq, "kc": kc, "k": k, "cap": cap, "groups": n_groups, "exclude_width": E}
    return res


def main():
    lib = _lib.load()
    parent = None
    if ARGS.parent_lib:
        parent = C.CDLL(os.path.abspath(ARGS.parent_lib))
        parent.amdrec_select_topk.argtypes = _lib._SIGNATURES["amdrec_select_topk"]
        parent.amdrec_select_topk.restype = C.c_int
        assert not hasattr(parent, "amdrec_select_topk_capped"), "--parent-lib must be a build without the capped entry"
    res = {"device": torch.cuda.get_device_name(0), "repeats": ARGS.reps, "launches_per_repeat": ARGS.iters,
           "parent_build": bool(parent),
           "stage2_serving": select_cells(lib, parent, 512, 500, 10, 2),
           "stage2_general": select_cells(lib, parent, 512, 513, 10, 2),
           "stage1_compact": compact_cells(lib, 512, 1000, 500, 3)}
    print(json.dumps(res, indent=1))
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
