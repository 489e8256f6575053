"""Dev tool: what aware probes (amdrec.probes) buy and cost.  1M x 256 clustered rows (amdrec.devsynth), 64 queries near corpus
rows, k = 500; indexes IVF(100, 10) and IVF(4096, 64) with list_tags + list_boosts + aware_probes.
Recall part.  Per (index, tag pattern, selectivity) and probe policy ("similarity" | "aware"): fill rate (filled slots over
min(k, eligible ads), mean over queries) and recall@500 against the masked Flat result (share of the Flat result's filled slots
that the IVF result holds).  Tag patterns: "random" - the tag on a random share of the ads; "clustered" - the tag on all ads
nearest to a random subset of 1024 anchor directions (region-correlated, independent of the index's own partition).  Boost arm:
0.1 % of the ads at boost +0.5, w = 1, against the boosted Flat result; also the share of the boosted ads of the Flat result
that each policy finds.
Time part.  The coarse step, plain export against aware export (keys + select, as coarse_probes runs them), by HIP events,
alternating A B A B in the same process, REPS calls per window over ROT rotating query batches after 3 warm-up calls, 3 windows
each (their spread is the run's own); the summary kernel at 1M and 10M rows over 4096 lists.
usage: python tools/aware_probes_recall.py [--out FILE] [--n ROWS] [--skip-time]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--skip-time", action="store_true")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommender-demo_amd"))
import torch  # noqa: E402
from amdrec import _lib, devsynth  # noqa: E402
from amdrec.index import FAISSIndex  # noqa: E402

DIM, K, NQ, REPS, ROT, WINDOWS = 256, 500, 64, 200, 4, 3
INDEXES = ((100, 10), (4096, 64))
SELECTIVITIES = (0.1, 0.01, 0.001)
ANCHORS = 1024
TAG = 1


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


def tag_patterns(x, g, dev):
    """-> {(pattern, selectivity): int64 [n] tag words}"""
    n = x.shape[0]
    out = {}
    anchors = torch.randn((ANCHORS, DIM), generator=g, device=dev)
    near = torch.empty(n, dtype=torch.int64, device=dev)
    for s in range(0, n, 1 << 18):
        near[s:s + (1 << 18)] = (x[s:s + (1 << 18)] @ anchors.T).argmax(dim=1)
    order = torch.randperm(ANCHORS, generator=g, device=dev)
    for sel in SELECTIVITIES:
        t = torch.zeros(n, dtype=torch.int64, device=dev)
        t[torch.randperm(n, generator=g, device=dev)[:max(1, int(n * sel))]] = TAG
        out[("random", sel)] = t
        pick = torch.zeros(ANCHORS, dtype=torch.bool, device=dev)
        pick[order[:max(1, round(ANCHORS * sel))]] = True
        out[("clustered", sel)] = pick[near].to(torch.int64) * TAG
    return out


def recall(pos, ref):
    """mean over queries of |pos & ref| / |ref filled| (queries whose reference is empty are left out)"""
    vals = []
    for p, r in zip(pos.tolist(), ref.tolist()):
        r = {v for v in r if v >= 0}
        if r:
            vals.append(len(r & set(p)) / len(r))
    return round(sum(vals) / max(1, len(vals)), 4)


def fill(pos, eligible):
    want = min(K, eligible)
    return round(float((pos >= 0).sum(dim=1).float().mean()) / max(1, want), 4)


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    n = ARGS.n
    x = devsynth.device_clustered_corpus(n, DIM, dev, n_clusters=4096, spread=0.5)
    q = x[torch.randperm(n, generator=g, device=dev)[:NQ]] + 0.3 * torch.randn((NQ, DIM), generator=g, device=dev) / DIM ** 0.5
    tags = tag_patterns(x, g, dev)
    boosts = torch.zeros(n, device=dev)
    boosted = torch.randperm(n, generator=g, device=dev)[:max(1, n // 1000)]
    boosts[boosted] = 0.5
    ma, my = torch.full((NQ,), TAG, dtype=torch.int64, device=dev), torch.zeros(NQ, dtype=torch.int64, device=dev)
    w = torch.ones(NQ, device=dev)
    flat = FAISSIndex(DIM, index_type="Flat")
    flat.add(x, boosts=boosts)
    ref = {}
    for key, t in tags.items():
        flat.set_tags(t)
        ref[key] = flat.search_device(q, K, return_positions=True, require_all=ma, require_any=my)[0].clone()
    ref_boost = flat.search_device(q, K, return_positions=True, boost_weight=w)[0].clone()
    is_boosted = torch.zeros(n + 1, dtype=torch.bool, device=dev)
    is_boosted[boosted] = True
    rows, times = [], []
    for nlist, nprobe in INDEXES:
        idx = FAISSIndex(DIM, index_type="IVF", nlist=nlist, nprobe=nprobe, list_tags=True, list_boosts=True, aware_probes=True)
        idx.add(x, boosts=boosts)
        idx.search_device(q[:1], 1)                                       # lays the lists out (the summaries come with them)
        name = f"IVF({nlist},{nprobe})"
        for (pattern, sel), t in tags.items():
            idx.set_tags(t)
            eligible = int((t != 0).sum())
            infeasible = float((idx._ivf.list_tag_or == 0).float().mean())
            for policy in ("similarity", "aware"):
                pos = idx.search_device(q, K, return_positions=True, require_all=ma, require_any=my, probe_policy=policy)[0]
                rec = {"index": name, "arm": "masks", "tags": pattern, "selectivity": sel, "eligible_ads": eligible,
                       "lists_without_an_eligible_ad": round(infeasible, 4), "policy": policy, "fill_rate": fill(pos, eligible),
                       "recall_at_500_vs_flat": recall(pos, ref[(pattern, sel)])}
                print(json.dumps(rec), flush=True)
                rows.append(rec)
        for policy in ("similarity", "aware"):
            pos = idx.search_device(q, K, return_positions=True, boost_weight=w, probe_policy=policy)[0]
            rb = torch.where(is_boosted[ref_boost], ref_boost, torch.full_like(ref_boost, -1))      # the Flat result's boosted ads
            rec = {"index": name, "arm": "boost 0.1% at +0.5, w=1", "policy": policy, "fill_rate": fill(pos, n),
                   "recall_at_500_vs_flat": recall(pos, ref_boost), "boosted_ads_in_flat_result_per_query":
                   round(float((rb >= 0).sum(dim=1).float().mean()), 2), "recall_of_those": recall(pos, rb)}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
        if ARGS.skip_time:
            continue
        st = idx._ivf
        idx.set_tags(tags[("random", 0.01)])
        for B in (1, 64, 512):
            qs = [idx._normalize_(torch.randn((B, DIM), generator=g, device=dev)) for _ in range(ROT)]
            a, y = torch.full((B,), TAG, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)
            wt = torch.ones(B, device=dev)
            arms = {"plain": lambda i: st.coarse_probes(qs[i % ROT], nprobe),
                    "aware masks": lambda i: st.coarse_probes(qs[i % ROT], nprobe, elig=(a, y)),
                    "aware masks+boost": lambda i: st.coarse_probes(qs[i % ROT], nprobe, elig=(a, y), boost=(wt, 0.5))}
            ms = {k_: [] for k_ in arms}
            for _ in range(WINDOWS):                                      # A B C A B C ...
                for k_, fn in arms.items():
                    ms[k_].append(round(timed(fn), 5))
            rec = {"index": name, "B": B, "coarse_step_ms_per_call": ms}
            print(json.dumps(rec), flush=True)
            times.append(rec)
    summaries = []
    if not ARGS.skip_time:
        lib = _lib.load()
        for rows_n in (1_000_000, 10_000_000):
            nlist = 4096
            lens = torch.randint(0, 2 * rows_n // nlist, (nlist,), generator=g, device=dev)
            off = torch.zeros(nlist + 1, dtype=torch.int64, device=dev)
            off[1:] = torch.cumsum(lens, 0)
            total = int(off[-1])
            lt = torch.randint(0, 1 << 40, (total,), generator=g, device=dev)
            lb = torch.randn(total, generator=g, device=dev)
            t_or, hi, lo = (torch.zeros(nlist, dtype=torch.int64, device=dev), torch.zeros(nlist, device=dev),
                            torch.zeros(nlist, device=dev))

            def run(i):
                _lib.check(lib.amdrec_ivf_list_summaries(_lib.ptr(off), nlist, _lib.ptr(lt), _lib.ptr(lb), _lib.ptr(t_or),
                                                         _lib.ptr(hi), _lib.ptr(lo), _lib.stream_ptr(dev)))
            ms = [round(timed(run), 5) for _ in range(WINDOWS)]
            rec = {"summary_kernel_rows": total, "nlist": nlist, "ms_per_call": ms,
                   "GBps": round(total * 12 / (min(ms) * 1e-3) / 1e9, 1)}
            print(json.dumps(rec), flush=True)
            summaries.append(rec)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "n": n, "dim": DIM, "k": K, "queries": NQ, "reps": REPS, "warmup": 3,
                       "rotating_inputs": ROT, "windows": WINDOWS, "recall": rows, "coarse_step": times, "summaries": summaries},
                      f, indent=1)


if __name__ == "__main__":
    main()
