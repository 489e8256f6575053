"""Dev tool: what value ranking (amdrec_select_topk_value / _value_auction, csrc/select.hip) costs on the benchmark's workload.
Builds bench.py's pipeline (its models, its corpus of --ads rows, a batch of 512 users) and in ONE process, after a warm-up,
alternating over REPS repeats (each a HIP-event pair around ITERS back-to-back launches, divided by ITERS) times
  amdrec_select_topk against amdrec_select_topk_value, and amdrec_select_topk_auction against amdrec_select_topk_value_auction
  (three tasks, all weights nonzero, no cap, no reserve) at 512 x 500 -> 10 (one recommend_device call's own logits and
  candidates), 1 x 500 -> 10 and 64 x 2048 -> 100, the sort shape (random logits);
  and the end-to-end recommend_device step at 512 users without and with head_weights, on an instance in heads_mode "all" and
  on one in "ctr_first" (which runs a call with head_weights on all heads: what such a caller gives up).
The spread is (max - min) / median over the repeats of one cell.
usage: python tools/value_select_time.py [--out FILE] [--ads N] [--reps R] [--iters N]"""
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

B, TOP_K, K1 = 512, 10, 500
WEIGHTS = {"ctr": 1.0, "engagement": 0.5, "revenue": 0.25}


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


def launches(lib, dev, logits, pos, bids, n_users, k_c, top_k, weights):
    """The four entries on one shape -> {name: launch}."""
    n_tasks = logits.shape[0]
    ids = torch.empty((n_users, top_k), dtype=torch.int64, device=dev)
    sc = torch.empty((n_tasks, n_users, top_k), dtype=torch.float32, device=dev)
    val, ecpm, price = (torch.empty((n_users, top_k), dtype=torch.float32, device=dev) for _ in range(3))
    w = torch.tensor([weights], dtype=torch.float32, device=dev).expand(n_users, n_tasks).contiguous()
    st = _lib.stream_ptr(dev)
    lg = (_lib.ptr(logits), logits.stride(0), n_tasks)
    cands = (_lib.ptr(pos), _lib.ptr(pos), n_users, k_c, top_k)
    outs = (_lib.ptr(ids), _lib.ptr(sc), None)
    bid = (_lib.ptr(bids), bids.shape[0], None)

    def check(rc):
        assert rc == 0, lib.amdrec_last_error()
    return {"select_topk": lambda: check(lib.amdrec_select_topk(*lg, 0, *cands, *outs, st)),
            "select_topk_value": lambda: check(lib.amdrec_select_topk_value(*lg, *cands, _lib.ptr(w), None, 0, 0, *outs,
                                                                            _lib.ptr(val), st)),
            "select_topk_auction": lambda: check(lib.amdrec_select_topk_auction(*lg, 0, *cands, *bid, None, 0, 0, *outs,
                                                                                _lib.ptr(ecpm), _lib.ptr(price), st)),
            "select_topk_value_auction": lambda: check(lib.amdrec_select_topk_value_auction(
                *lg, 0, *cands, _lib.ptr(w), *bid, None, 0, 0, *outs, _lib.ptr(val), _lib.ptr(ecpm), _lib.ptr(price), st))}


def main():
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    tt, rk, _, (user, ad, nnum) = bench.build_models(dev)
    index = FAISSIndex(bench.DIM, index_type="Flat", device=dev)
    index.add(bench.device_corpus(ARGS.ads, bench.DIM, dev))
    gen = torch.Generator(device=dev).manual_seed(7)
    index.set_bids(torch.rand(ARGS.ads, generator=gen, device=dev) * 4)
    ad_table = torch.from_numpy(synth.ad_features(ad, ARGS.ads, seed=99)).to(dev)
    recs = {mode: AdRecommenderInference(two_tower_model=tt, transformer_ranker=rk, faiss_index=index, ad_features=ad_table,
                                         heads=mode) for mode in ("all", "ctr_first")}
    uc, un = (torch.from_numpy(a).to(dev) for a in synth.user_batch(user, nnum, B, seed=2024))
    out = recs["all"].recommend_device(uc, un, TOP_K, K1)
    tasks = list(out["tasks"])
    weights = [WEIGHTS.get(t, 0.0) for t in tasks]
    res = {"device": torch.cuda.get_device_name(0), "repeats": ARGS.reps, "ads": ARGS.ads, "tasks": tasks,
           "weights": weights, "launch": {}, "step": {}}
    shapes = {"512x500_top10": (B, K1, TOP_K, out["logits"], out["candidate_ids"])}      # default ids: an id is a position
    for name, (n, k_c, top_k) in (("1x500_top10", (1, 500, 10)), ("64x2048_top100", (64, 2048, 100))):
        logits = torch.randn((len(tasks), n * k_c), generator=gen, device=dev) * 2
        pos = torch.randint(0, ARGS.ads, (n, k_c), generator=gen, device=dev)
        shapes[name] = (n, k_c, top_k, logits, pos)
    for name, (n, k_c, top_k, logits, pos) in shapes.items():
        res["launch"][name] = alternate(launches(lib, dev, logits, pos, index._bids, n, k_c, top_k, weights), ARGS.iters)
    for mode, rec in recs.items():
        res["step"][f"heads_{mode}"] = alternate(
            {"plain": lambda rec=rec: rec.recommend_device(uc, un, TOP_K, K1),
             "head_weights": lambda rec=rec: rec.recommend_device(uc, un, TOP_K, K1, head_weights=WEIGHTS),
             "ecpm": lambda rec=rec: rec.recommend_device(uc, un, TOP_K, K1, rank_by="ecpm"),
             "ecpm_head_weights": lambda rec=rec: rec.recommend_device(uc, un, TOP_K, K1, rank_by="ecpm", head_weights=WEIGHTS)},
            ARGS.step_iters)
    moved = int((recs["all"].recommend_device(uc, un, TOP_K, K1, head_weights=WEIGHTS)["ad_ids"] != out["ad_ids"]).any(dim=1).sum())
    res["users_whose_answer_changes"] = moved
    print(json.dumps(res, indent=1))
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
