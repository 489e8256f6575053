"""Dev tool: what a stage-1 score boost costs in the inverted-list scans (FAISSIndex(index_type="IVF", list_boosts=True)).
1M x 256 randn rows, k = 500, batch B in {1, 32, 512}; indexes IVF(100, 10) and IVF(1024, 32) with AMDREC_IVF_MIXED=0 and =1.
Per cell: search time (HIP events, mean of REPS searches over ROT rotating query batches, after 3 warm-up searches) and the
scan / bound / select kernels alone (amdrec_profile_* tags).
Arms, in this order, on ONE index per (nlist, nprobe) - only the boosts and the weight change: no weight (the plain search);
w = 0 (the boosted kernels, nothing reordered); noise 0.02 at w = 1; 1 % of the rows at +0.5 at w = 1; 10 % at 64.0 at w = 4
(|w| boost_max = 256: the widest nomination bound, scores quantised to the ulp of 256); no weight again.  The first and the
last arm are the same search: their difference is the run's own spread.
usage: python tools/ivf_boost_latency.py [--out FILE] [--n ROWS] [--only NAME] [--batches 1,32,512]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--only", default=None, help="one of the index names below")
ap.add_argument("--batches", default="1,32,512")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommender-demo_amd"))
import torch  # noqa: E402
from amdrec import _lib  # noqa: E402
from amdrec.index import FAISSIndex  # noqa: E402

K, REPS, ROT = 500, 20, 4
BATCHES = tuple(int(b) for b in ARGS.batches.split(","))
# name -> (nlist, nprobe, AMDREC_IVF_MIXED or None)
INDEXES = {"IVF(100,10)": (100, 10, None), "IVF(1024,32) fp32 filter": (1024, 32, "0"), "IVF(1024,32) bf16 prefilter": (1024, 32, "1")}
# arm -> (boost pattern or None, weight or None)
ARMS = (("none", None, None), ("w=0", "noise", 0.0), ("noise 0.02, w=1", "noise", 1.0), ("1% at +0.5, w=1", "sparse", 1.0),
        ("10% at 64.0, w=4", "quantised", 4.0), ("none again", None, None))


def timed(fn, reps=REPS):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels_ms(fn, reps=10):
    """-> {tag: ms per search} of the search's list-scan, bound and select kernels"""
    torch.cuda.synchronize()
    _lib.profile_enable(True, only="iv")
    for i in range(reps):
        fn(i)
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    return {t: round(e["total_ms"] / reps, 4) for t, e in sorted(rep.items())}


def patterns(n, g, dev):
    sparse = torch.zeros(n, device=dev)
    sparse[torch.randperm(n, generator=g, device=dev)[:n // 100]] = 0.5
    quant = torch.zeros(n, device=dev)
    quant[torch.randperm(n, generator=g, device=dev)[:n // 10]] = 64.0
    return {"noise": 0.02 * torch.randn(n, generator=g, device=dev), "sparse": sparse, "quantised": quant}


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    n = ARGS.n
    x = torch.randn((n, 256), generator=g, device=dev)
    boosts = patterns(n, g, dev)
    qs = {B: [torch.randn((B, 256), generator=g, device=dev) for _ in range(ROT)] for B in BATCHES}
    out, built = [], {}
    for name, (nlist, nprobe, mixed) in INDEXES.items():
        if ARGS.only and name != ARGS.only:
            continue
        if mixed is None:
            os.environ.pop("AMDREC_IVF_MIXED", None)
        else:
            os.environ["AMDREC_IVF_MIXED"] = mixed
        if (nlist, nprobe) not in built:                            # (the two IVF(1024,32) arms share the index)
            built.clear()
            idx = FAISSIndex(256, index_type="IVF", nlist=nlist, nprobe=nprobe, list_boosts=True)
            idx.add(x)
            built[(nlist, nprobe)] = idx
        idx = built[(nlist, nprobe)]
        for B in BATCHES:
            for arm, pat, weight in ARMS:
                if pat is not None:
                    idx.set_boosts(boosts[pat])
                if weight is None:
                    fn = lambda i: idx.search_device(qs[B][i % ROT], K)                            # noqa: E731
                else:
                    w = torch.full((B,), weight, dtype=torch.float32, device=dev)
                    fn = lambda i: idx.search_device(qs[B][i % ROT], K, boost_weight=w)            # noqa: E731
                rec = {"index": name, "B": B, "n": n, "k": K, "arm": arm, "search_ms": round(timed(fn), 4),
                       "kernel_ms_per_search": kernels_ms(fn)}
                print(json.dumps(rec), flush=True)
                out.append(rec)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": 3, "rotating_inputs": ROT,
                       "runs_per_cell": 1, "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
