#!/usr/bin/env python3
"""Dev tool: same-run A/B of the ranker engines "f16x3" (three fp16 products per MAC) and "f16" (one), on the benchmark's
workload: 1M x 256 Flat corpus, both ranker caches, stage1_k 500, top_k 10.

    python tools/ranker_engine_ab.py [--blocks 4] [--warmup 20] [--samples 30] [--out profiles/f16_engine_ab.json]

One process, one device.  Every arm has its own ranker (a copy of the same weights, packed and cached once, so no arm pays a
repack inside the timed region) and the arms alternate in blocks - A B A B ... - of --warmup (>= 20) untimed and --samples
timed runs each (blocks x samples >= 100 per arm).  Per arm: the median over all samples, the median of each block, and the
spread = largest - smallest block median.  The yardstick is f16x3 in this run; "faster" is claimed only where f16's median
beats f16x3's by more than the spread of f16x3's own blocks.
 (a) the ranker launch alone at 256 000 rows (512 users x 500 candidates through score_candidates): the time of the one
     row-owner launch by the library's per-launch events (amdrec_profile_report), with the first FFN cached and uncached;
 (b) one recommend_device step at B = 512, users rotating through 8 seeded batches, bracketed by a pair of HIP events;
 (c) one request at B = 1, likewise (f16x3 runs the column-split kernel there, f16 the 64-row shape).
For (b) and (c) a separate profiled pass gives the per-tag kernel table.  Prints one JSON line per measurement and writes
them all to --out."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "movie-recommender-demo_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from amdrec import _lib, synth  # noqa: E402
from amdrec.index import FAISSIndex  # noqa: E402
from amdrec.pipeline import AdRecommenderInference  # noqa: E402

N_ADS, DIM, TOP_K, STAGE1_K, N_USER_BATCHES = 1_000_000, 256, 10, 500, 8
ENGINES = ("f16x3", "f16")
TAGS_128 = {"f16x3": "ranker_rowowner16_128_x3", "f16": "ranker_rowowner16_128_f16"}


def summary(blocks):
    """blocks: per block the samples (ms) -> median, block medians and their spread."""
    allv = np.concatenate(blocks)
    med = [float(np.median(b)) for b in blocks]
    return {"samples": int(allv.size), "median_ms": round(float(np.median(allv)), 4), "p95_ms": round(float(np.percentile(allv, 95)), 4),
            "min_ms": round(float(allv.min()), 4), "block_medians_ms": [round(m, 4) for m in med],
            "block_spread_ms": round(max(med) - min(med), 4)}


def alternate(arms, n_blocks, warmup, samples, run):
    """run(arm, i) -> ms or None (None: timed by the caller's events) for arms alternating in blocks."""
    out = {a: [] for a in arms}
    for _ in range(n_blocks):
        for a in arms:
            for i in range(warmup):
                run(a, i, False)
            torch.cuda.synchronize()
            out[a].append(np.array(run(a, range(samples), True)))
    return {a: summary(b) for a, b in out.items()}


def verdict(res, base="f16x3", new="f16"):
    gain = res[base]["median_ms"] - res[new]["median_ms"]
    return {"f16x3_over_f16": round(res[base]["median_ms"] / res[new]["median_ms"], 4), "gain_ms": round(gain, 4),
            "f16x3_block_spread_ms": res[base]["block_spread_ms"], "faster_beyond_spread": bool(gain > res[base]["block_spread_ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--profile-steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_engine_ab.json"))
    a = ap.parse_args()
    warmup = max(a.warmup, 20)
    samples = max(a.samples, -(-100 // max(a.blocks, 1)))
    dev = torch.device("cuda:0")
    tt, rk0, _, (user, ad, nnum) = bench.build_models(dev)
    idx = FAISSIndex(DIM, index_type="Flat", device=dev)
    idx.add(bench.device_corpus(N_ADS, DIM, dev))
    table = torch.from_numpy(synth.ad_features(ad, N_ADS, seed=99)).to(dev)
    users = []
    for s in range(N_USER_BATCHES):
        uc, un = synth.user_batch(user, nnum, 512, seed=100 + s)
        users.append((torch.from_numpy(uc).to(dev), torch.from_numpy(un).to(dev)))
    results = {"tool": "tools/ranker_engine_ab.py", "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "warmup_per_block": warmup,
               "samples_per_block": samples, "corpus": [N_ADS, DIM], "stage1_k": STAGE1_K, "top_k": TOP_K}

    def ranker(engine, cached):
        rk = copy.deepcopy(rk0)
        rk.gemm_engine, rk.cache_first_ffn = engine, cached
        rk.ensure_ad_cache(table)
        return rk

    # ---- (a) the ranker launch alone, 256 000 rows ----
    cand = torch.from_numpy(np.random.default_rng(5).integers(0, N_ADS, (512, STAGE1_K))).to(dev)
    for cached in (True, False):
        rks = {e: ranker(e, cached) for e in ENGINES}

        def launch(e, it, timed):
            def one(i):
                uc, un = users[i % N_USER_BATCHES]
                return rks[e].score_candidates(uc, un, cand, table)
            if not timed:
                one(it)
                return None
            ms = []
            for i in it:
                _lib.profile_enable(True)
                one(i)
                torch.cuda.synchronize()
                rep = _lib.profile_report()
                _lib.profile_enable(False)
                assert rep[TAGS_128[e]]["launches"] == 1, rep
                ms.append(rep[TAGS_128[e]]["total_ms"])
            return ms
        res = alternate(ENGINES, a.blocks, warmup, samples, launch)
        key = "a_launch_256000_rows_" + ("cached_first_ffn" if cached else "uncached_first_ffn")
        results[key] = {**res, "verdict": verdict(res)}
        print(json.dumps({key: results[key]}), flush=True)
        if not cached:
            del rks
    # ---- (b), (c) the serving step ----
    recs = {e: AdRecommenderInference(two_tower_model=tt, transformer_ranker=ranker(e, True), faiss_index=idx, ad_features=table)
            for e in ENGINES}
    for key, B in (("b_step_B512", 512), ("c_request_B1", 1)):
        def step(e, it, timed):
            def one(i):
                uc, un = users[i % N_USER_BATCHES]
                return recs[e].recommend_device(uc[:B], un[:B], TOP_K, STAGE1_K)
            if not timed:
                one(it)
                return None
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in it]
            for i, (e0, e1) in zip(it, ev):
                e0.record()
                one(i)
                e1.record()
            torch.cuda.synchronize()
            return [e0.elapsed_time(e1) for e0, e1 in ev]
        res = alternate(ENGINES, a.blocks, warmup, samples, step)
        kern = {}
        for e in ENGINES:
            _lib.profile_enable(True)
            for i in range(a.profile_steps):
                step(e, i, False)
            torch.cuda.synchronize()
            rep = _lib.profile_report()
            _lib.profile_enable(False)
            kern[e] = {t: round(1000.0 * r["total_ms"] / a.profile_steps, 2) for t, r in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"])}
        results[key] = {**res, "verdict": verdict(res), "kernels_us_per_step": kern}
        print(json.dumps({key: results[key]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
