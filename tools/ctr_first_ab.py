#!/usr/bin/env python3
"""Dev tool: A/B of the serving step with stage 2 in "all" mode against "ctr_first" (AdRecommenderInference ``heads``), on
the benchmark's workload: 1M x 256 corpus, both ranker caches, stage1_k 500, top_k 10, B in {1, 32, 512}.

    python tools/ctr_first_ab.py [--warmup 20] [--steps 100] [--batches 1,32,512] [--label NAME]

Per arm and batch size: --warmup (>= 20) untimed steps, then --steps (>= 100) steps each bracketed by its own pair of HIP
events on the launch stream (users rotate through 8 seeded batches) -> median and p95 of the step; then a separate pass with
the library's per-launch events on for the per-tag kernel table (amdrec_profile_report: the events cost the stream ~10 us
per launch, so that pass is not the one the step times come from).  On a tree without the mode (the parent commit) the tool
runs the all-heads arm alone: run it there for the noise figure.  Prints one JSON line per (arm, B) and the tables."""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--profile-steps", type=int, default=20)
    ap.add_argument("--batches", default="1,32,512")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    warmup, steps = max(a.warmup, 20), max(a.steps, 100)
    dev = torch.device("cuda:0")
    tt, rk, _, (user, ad, nnum) = bench.build_models(dev)
    idx = FAISSIndex(DIM, index_type="Flat", device=dev)
    idx.add(bench.device_corpus(N_ADS, DIM, dev))
    table = torch.from_numpy(synth.ad_features(ad, N_ADS, seed=99)).to(dev)
    rec = AdRecommenderInference(two_tower_model=tt, transformer_ranker=rk, faiss_index=idx, ad_features=table)
    has_mode = hasattr(rec, "heads_mode")
    arms = ["all", "ctr_first"] if has_mode else ["all"]
    print(f"# ctr_first_ab {a.label}: arms {arms}, warmup {warmup}, steps {steps}, corpus {N_ADS} x {DIM}, stage1_k {STAGE1_K}, "
          f"top_k {TOP_K}", flush=True)
    users = []
    for s in range(N_USER_BATCHES):
        uc, un = synth.user_batch(user, nnum, 512, seed=100 + s)
        users.append((torch.from_numpy(uc).to(dev), torch.from_numpy(un).to(dev)))

    def step(arm, B, i):
        uc, un = users[i % N_USER_BATCHES]
        if has_mode:
            return rec.recommend_device(uc[:B], un[:B], TOP_K, STAGE1_K, heads=arm)
        return rec.recommend_device(uc[:B], un[:B], TOP_K, STAGE1_K)

    for B in [int(b) for b in a.batches.split(",")]:
        if has_mode:                                                  # the two arms must agree before either is timed
            x, y = step("all", B, 0), None
            x = {k: v.clone() for k, v in x.items() if isinstance(v, torch.Tensor)}
            y = step("ctr_first", B, 0)
            same = all(torch.equal(x[k], y[k]) for k in ("ad_ids", "scores")) and torch.equal(x["logits"][0], y["logits"][0])
            print(f"# B={B}: ctr_first runs as {rec.heads_mode_effective('ctr_first')}, logits {tuple(y['logits'].shape)}, "
                  f"bit-identical to all: {same}", flush=True)
            assert same
        for arm in arms:
            for i in range(warmup):
                step(arm, B, i)
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            for i, (e0, e1) in enumerate(ev):
                e0.record()
                step(arm, B, i)
                e1.record()
            torch.cuda.synchronize()
            ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
            _lib.profile_enable(True)
            for i in range(a.profile_steps):
                step(arm, B, i)
            torch.cuda.synchronize()
            rep = _lib.profile_report()
            _lib.profile_enable(False)
            row = {"label": a.label, "arm": arm, "B": B, "steps": steps, "median_ms": round(float(np.median(ms)), 4),
                   "p95_ms": round(float(np.percentile(ms, 95)), 4), "min_ms": round(float(ms.min()), 4),
                   "kernels_us_per_step": {t: round(1000.0 * r["total_ms"] / a.profile_steps, 2)
                                           for t, r in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"])}}
            print(json.dumps(row), flush=True)
            print(f"  {'tag':34s} {'launches/step':>13s} {'us/step':>10s}")
            for t, r in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"]):
                print(f"  {t:34s} {r['launches'] / a.profile_steps:13.2f} {1000.0 * r['total_ms'] / a.profile_steps:10.2f}")
            sys.stdout.flush()


if __name__ == "__main__":
    main()
