"""Dev tool: what per-ad score boosts cost in the Flat search (bf16 engine).  1M x 256 randn rows, k = 500, batch B in
{1, 32, 512}; per cell: search time (HIP events, mean of REPS searches over ROT rotating query batches), the search's kernels
by profile tag (corpus pass, sample, finalize, fix-up), and n_fixup of one search.  The yardstick is the plain search of the
same run, measured first and again last: their difference is the run's own spread.
Arms: none; w = 0 (the boosted kernels, every term zero); small-noise boosts (0.02 randn, w = 1); 1 % of the rows at +0.5
(w = 1); 10 % of the rows at 64.0 with w = 4 (|w| boost_max = 256: the widened error bound, quantised scores and ties).
usage: python tools/boost_latency.py [--out FILE] [--n ROWS]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--n", type=int, default=1_000_000)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommender-demo_amd"))
import torch  # noqa: E402
from amdrec import _lib  # noqa: E402
from amdrec.index import FAISSIndex  # noqa: E402

BATCHES, K, REPS, ROT = (1, 32, 512), 500, 20, 4


def timed(fn, reps=REPS):
    for i in range(min(3, reps)):
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
    """-> {tag: ms per launch} of the search's kernels, and the sum per search"""
    torch.cuda.synchronize()
    _lib.profile_enable(True, only="search_")
    for i in range(reps):
        fn(i)
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    per = {t: round(e["total_ms"] / e["launches"], 4) for t, e in sorted(rep.items())}
    return per, round(sum(e["total_ms"] for e in rep.values()) / reps, 4)


def n_fixup(idx, fn):
    idx.n_fixup_out = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    fn(0)
    torch.cuda.synchronize()
    n, idx.n_fixup_out = int(idx.n_fixup_out.item()), None
    return n


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    n = ARGS.n
    x = torch.randn((n, 256), generator=g, device=dev)
    noise = 0.02 * torch.randn(n, generator=g, device=dev)
    sparse = (torch.rand(n, generator=g, device=dev) < 0.01).to(torch.float32) * 0.5
    quant = (torch.rand(n, generator=g, device=dev) < 0.10).to(torch.float32) * 64.0
    idx = FAISSIndex(256, index_type="Flat")
    idx.add(x, boosts=noise)
    arms = [("none", None, None), ("w=0", noise, 0.0), ("noise 0.02, w=1", noise, 1.0), ("1% at +0.5, w=1", sparse, 1.0),
            ("10% at 64.0, w=4", quant, 4.0), ("none (again)", None, None)]
    out = []
    for B in BATCHES:
        qs = [torch.randn((B, 256), generator=g, device=dev) for _ in range(ROT)]
        for name, boosts, w in arms:
            if boosts is not None:
                idx.set_boosts(boosts)
            wt = None if w is None else torch.full((B,), w, dtype=torch.float32, device=dev)
            fn = lambda i: idx.search_device(qs[i % ROT], K, boost_weight=wt)                  # noqa: E731
            per, total = kernels_ms(fn)
            rec = {"B": B, "n": n, "k": K, "arm": name, "search_ms": round(timed(fn), 4), "kernels_ms_per_search": total,
                   "kernel_ms": per, "n_fixup": n_fixup(idx, fn)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": REPS, "rotating_inputs": ROT, "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
