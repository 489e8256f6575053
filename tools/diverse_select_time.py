"""Dev tool: what the diversified selection (amdrec_select_topk_diverse, csrc/select.hip) costs on the benchmark's workload.
Builds bench.py's pipeline (its models, its corpus of --ads rows, a batch of 512 users), takes one recommend_device call's own
logits and candidates, and in ONE process, after a warm-up, alternating over REPS repeats (each a HIP-event pair around ITERS
back-to-back launches, divided by ITERS) times
  amdrec_select_topk against amdrec_select_topk_diverse at pool 64 and 128 (lam 0.7; 512 x 500 -> 10, rows of 256 floats),
  and the end-to-end recommend_device step without and with diversity (pool 64 and 128), both heads modes' default.
The spread is (max - min) / median over the repeats of one cell.
usage: python tools/diverse_select_time.py [--out FILE] [--ads N] [--reps R] [--iters N]"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--ads", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--step-iters", type=int, default=10)
ARGS = ap.parse_args()
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "movie-recommender-demo_amd"))
import torch  # noqa: E402
import bench  # noqa: E402
from amdrec import _lib, synth  # noqa: E402
from amdrec.index import FAISSIndex  # noqa: E402
from amdrec.pipeline import AdRecommenderInference  # noqa: E402

B, TOP_K, K1, LAM = 512, 10, 500, 0.7


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


def alternate(cells, iters):
    for fn in cells.values():
        fn()
        event_us(fn, 3)
    times = {name: [] for name in cells}
    for _ in range(ARGS.reps):
        for name, fn in cells.items():
            times[name].append(event_us(fn, iters))
    return {name: stats(t) for name, t in times.items()}


def main():
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    tt, rk, _, (user, ad, nnum) = bench.build_models(dev)
    index = FAISSIndex(bench.DIM, index_type="Flat", device=dev)
    index.add(bench.device_corpus(ARGS.ads, bench.DIM, dev))
    ad_table = torch.from_numpy(synth.ad_features(ad, ARGS.ads, seed=99)).to(dev)
    rec = AdRecommenderInference(two_tower_model=tt, transformer_ranker=rk, faiss_index=index, ad_features=ad_table)
    uc, un = (torch.from_numpy(a).to(dev) for a in synth.user_batch(user, nnum, B, seed=2024))
    out = rec.recommend_device(uc, un, TOP_K, K1)
    logits, pos = out["logits"], out["candidate_ids"]                      # default ids: an id is a position
    ids = torch.empty((B, TOP_K), dtype=torch.int64, device=dev)
    sc = torch.empty((logits.shape[0], B, TOP_K), dtype=torch.float32, device=dev)
    val = torch.empty((B, TOP_K), dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)
    head = (_lib.ptr(logits), logits.stride(0), logits.shape[0], 0, _lib.ptr(pos), _lib.ptr(pos), B, K1, TOP_K)
    outs = (_lib.ptr(ids), _lib.ptr(sc), None)
    xb = index._xb

    def diverse(pool):
        def launch():
            assert lib.amdrec_select_topk_diverse(*head, _lib.ptr(xb), index._n, xb.stride(0), index.dimension, LAM, pool,
                                                  None, 0, 0, *outs, _lib.ptr(val), st) == 0, lib.amdrec_last_error()
        return launch

    def plain():
        assert lib.amdrec_select_topk(*head, *outs, st) == 0

    res = {"device": torch.cuda.get_device_name(0), "repeats": ARGS.reps, "ads": ARGS.ads,
           "shape": {"users": B, "candidates": K1, "top_k": TOP_K, "dim": index.dimension, "lam": LAM},
           "launch": alternate({"select_topk": plain, "select_topk_diverse_pool64": diverse(64),
                                "select_topk_diverse_pool128": diverse(128)}, ARGS.iters),
           "step": alternate({"plain": lambda: rec.recommend_device(uc, un, TOP_K, K1),
                              "diversity_pool64": lambda: rec.recommend_device(uc, un, TOP_K, K1, diversity=LAM),
                              "diversity_pool128": lambda: rec.recommend_device(uc, un, TOP_K, K1, diversity=LAM,
                                                                                diversity_pool=128)}, ARGS.step_iters)}
    moved = int((rec.recommend_device(uc, un, TOP_K, K1, diversity=LAM)["ad_ids"] != out["ad_ids"]).any(dim=1).sum())
    res["users_whose_answer_changes_at_pool64"] = moved
    print(json.dumps(res, indent=1))
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
