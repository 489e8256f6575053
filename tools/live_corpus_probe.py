"""Dev tool: what it costs to retire and insert ads in a live corpus.  Builds the 1M-ad Flat pipeline (demo models, both
per-ad ranker caches) and, after a warm-up, alternating over REPS repeats in ONE process:
  remove_ads of 1 000 and of 100 000 ids, and add_ads of the same rows (host clock closed by a synchronise: remove_ads reads
  the survivor count back);
  per stored tensor, amdrec_rows_gather against torch.index_select with the same ``kept`` (HIP events);
  the rebuild a user does without this feature: a fresh index ``add`` over the survivors plus ``ensure_ad_cache`` on their
  table (host clock + synchronise).
Bytes moved are computed from the shapes.  The spread is (max - min) / median over the repeats of one cell.
usage: python tools/live_corpus_probe.py [--out FILE] [--n ROWS] [--reps R]"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommender-demo_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from amdrec import rows_edit, synth  # noqa: E402
from amdrec.index import FAISSIndex  # noqa: E402
from amdrec.pipeline import AdRecommenderInference, build_faiss_index  # noqa: E402
from amdrec.ranker import TransformerRanker  # noqa: E402
from amdrec.towers import TwoTowerModel  # noqa: E402

SIZES = (1_000, 100_000)


def stats(ms, nbytes=None):
    med = statistics.median(ms)
    out = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
           "spread": round((max(ms) - min(ms)) / med, 4), "repeats": len(ms)}
    if nbytes is not None:
        out["bytes"] = int(nbytes)
        out["GB_per_s"] = round(nbytes / med / 1e6, 1)
    return out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    del r
    return e0.elapsed_time(e1)


def row_bytes(rec):
    """{tensor: bytes per ad} of everything remove_ads gathers in this pipeline."""
    c = rec.transformer_ranker._ad_cache
    t = {"xb": rec.faiss_index._xb, "ids": rec.faiss_index._ids, "ad_features": rec.ad_features, "proj_cache": c[4]}
    if c[5] is not None:
        t["hidden_cache"] = c[5]
    return {k: v[0:1].numel() * v.element_size() for k, v in t.items()}, t


def main():
    dev = torch.device("cuda:0")
    n = ARGS.n
    user, ad, nnum = synth.demo_dims()
    to_t = lambda sd: {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}   # noqa: E731
    tt = TwoTowerModel(dict(user), dict(ad), nnum)
    tt.load_state_dict(to_t(synth.two_tower_state(user, ad, nnum, seed=3)))
    rk = TransformerRanker(dict(user), dict(ad), nnum)
    rk.load_state_dict(to_t(synth.ranker_state(user, ad, nnum, seed=4, cross_scale=1.0 / 16)))
    table = synth.ad_features(ad, n, seed=5)
    rec = AdRecommenderInference(device="cuda:0", two_tower_model=tt, transformer_ranker=rk,
                                 faiss_index=build_faiss_index(tt, table, device="cuda:0", index_type="Flat"),
                                 ad_features=table)
    uc, un = (torch.from_numpy(a).cuda() for a in synth.user_batch(user, nnum, 36, seed=10))
    rec.recommend_device(uc, un, 10, 500)                                     # builds both caches
    idx = rec.faiss_index
    per_row, _ = row_bytes(rec)
    d = idx.dimension
    res = {"device": torch.cuda.get_device_name(0), "n_ads": n, "repeats": ARGS.reps, "bytes_per_ad": per_row,
           "hidden_cache": rk._ad_cache[5] is not None, "remove_ads": {}, "add_ads": {}, "rows_gather_vs_index_select": {},
           "rebuild": {}}
    rng = np.random.default_rng(11)
    sets = {m: np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64) for m in SIZES}

    def cycle(m, times_rm, times_add):
        """Remove the m ids, then add the same ads back (their stored rows, features and ids)."""
        S = torch.from_numpy(sets[m]).to(dev)
        where = torch.isin(idx._ids[:idx._n], S).nonzero().squeeze(1)
        emb, feats, ids = idx._xb[where].clone(), rec.ad_features[where].clone(), idx._ids[where].cpu().tolist()
        t = host_ms(lambda: rec.remove_ads(sets[m]))
        assert idx.index.ntotal == n - m
        rec.recommend_device(uc, un, 10, 500)
        t2 = host_ms(lambda: rec.add_ads(emb, feats, ids))
        assert idx.index.ntotal == n and rk._cache_for(rec.ad_features) is not None
        rec.recommend_device(uc, un, 10, 500)
        if times_rm is not None:
            times_rm.append(t)
            times_add.append(t2)

    for m in SIZES:                                                           # warm-up: one cycle of each size
        cycle(m, None, None)
    t_rm, t_add = {m: [] for m in SIZES}, {m: [] for m in SIZES}
    for _ in range(ARGS.reps):                                                # alternating
        for m in SIZES:
            cycle(m, t_rm[m], t_add[m])
    total = sum(per_row.values())
    for m in SIZES:
        moved = (n - m) * 2 * total + ((n - m) * (d * 4 + d * 2) if idx._mixed else 0)     # gathers + the bf16 shadow rebuild
        res["remove_ads"][str(m)] = stats(t_rm[m], moved)
        appended = m * 2 * (d * 4 + 8 + per_row["ad_features"]) + n * 2 * (total - d * 4 - 8)   # grown copies of table + caches
        res["add_ads"][str(m)] = stats(t_add[m], appended)

    # the gather kernel alone against torch.index_select, same kept, same tensors
    for m in SIZES:
        kept = rows_edit.remove_plan(idx._ids, idx._n, torch.from_numpy(sets[m]).to(dev))
        _, tensors = row_bytes(rec)
        cell = {}
        for name, t in tensors.items():
            src = t[:idx._n]
            assert torch.equal(rows_edit.gather_rows(src, kept), torch.index_select(src, 0, kept))
            a, b = [], []
            for _ in range(ARGS.reps):
                a.append(event_ms(lambda: rows_edit.gather_rows(src, kept)))
                b.append(event_ms(lambda: torch.index_select(src, 0, kept)))
            nbytes = kept.numel() * (2 * per_row[name] + 8)
            sa, sb = stats(a, nbytes), stats(b, nbytes)
            cell[name] = {"rows_gather": sa, "index_select": sb,
                          "slower_beyond_spread": bool(sa["median_ms"] > sb["median_ms"] * (1 + max(sa["spread"], sb["spread"])))}
        res["rows_gather_vs_index_select"][str(m)] = cell

    # what a user does today: a fresh index over the survivors and both caches from scratch
    m = SIZES[-1]
    keep = torch.from_numpy(np.setdiff1d(np.arange(n), sets[m])).to(dev)
    emb, feats = idx._xb[:n][keep].clone(), rec.ad_features[keep].clone()
    ids = idx._ids[:n][keep].cpu().tolist()
    rk2 = TransformerRanker(dict(user), dict(ad), nnum)
    rk2.load_state_dict(to_t(synth.ranker_state(user, ad, nnum, seed=4, cross_scale=1.0 / 16)))
    rk2 = rk2.to(dev).eval()
    rk2._pack(dev)

    def rebuild():
        fresh = FAISSIndex(d, index_type="Flat", device=dev)
        fresh.add(emb, ids)
        rk2.cache_ad_projection(None)                                         # (drops the caches, keeps the packed weights)
        rk2.ensure_ad_cache(feats)
    rebuild()
    res["rebuild"] = {"survivors": int(keep.numel()), **stats([host_ms(rebuild) for _ in range(max(3, ARGS.reps))]),
                      "what": "fresh Flat index add() over the survivors + ensure_ad_cache (both caches) on their table"}
    print(json.dumps(res, indent=1))
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
