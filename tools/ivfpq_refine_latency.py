"""Dev tool: refined IVFPQ against plain IVFPQ and IVF-Flat on the same corpus, same box, same run.  Per shape and batch:
search time (HIP events, mean of REPS searches) of plain IVFPQ at k and at k' = min(k x factor, 2048), of the refined index
with fp32 and bf16 rows, and of IVF-Flat; the re-rank kernel's own time (amdrec_profile_* tag ivfpq_rerank) with its bytes
(nq x k' x row bytes) over that time; recall@k of each against Flat; resident device bytes per ad.
usage: python tools/ivfpq_refine_latency.py [--shapes 1m,10m] [--out FILE]
  1m : 1M x 256, nlist 100 / nprobe 10 (the reference's defaults)      10m: 10M x 256, nlist 4096 / nprobe 64
B in {1, 32, 512}, k = 500, pq_m = 8, refine_factor = 4.  Corpus and queries: torch.randn (as tools/ivfpq_latency.py)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommender-demo_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from amdrec import _lib, ivfpq  # noqa: E402
from amdrec.index import FAISSIndex  # noqa: E402

SHAPES = {"1m": (1_000_000, 100, 10), "10m": (10_000_000, 4096, 64)}
BATCHES, K, FACTOR, REPS = (1, 32, 512), 500, 4, 20
ACHIEVABLE_TBPS = 6.3          # the HBM rate the micro-architecture guide gives as achievable


def timed(fn, reps=REPS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rerank_ms(fn, reps=10):
    torch.cuda.synchronize()
    _lib.profile_enable(True, only="ivfpq_rerank")
    for _ in range(reps):
        fn()
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    return rep["ivfpq_rerank"]["total_ms"] / reps


def nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts if isinstance(t, torch.Tensor))


def resident_bytes(idx):
    """As tools/ivfpq_latency.py, plus the kept rows of a refined index."""
    lists = idx._ivf.lists
    per_list = () if lists is None else (lists.rows, lists.spos, lists.off, lists.lens)
    if idx._pq is not None:
        return nbytes(idx._ids, idx._pq.codes, idx._pq.finite, idx._pq.assign, idx._pq.rows, *per_list)
    return nbytes(idx._ids, idx._xb, idx._ivf.assign, *per_list, *(idx._ivf._shadow or ()))


def recall(ids, ref):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / ref.shape[1] for a, b in zip(ids, ref)]))


def run_shape(name, out):
    n, nlist, nprobe = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.randn((n, 256), generator=g, device=dev)
    idx = {}
    for key, kw in (("ivfpq", {}), ("refine_fp32", {"refine": "fp32", "refine_factor": FACTOR}),
                    ("refine_bf16", {"refine": "bf16", "refine_factor": FACTOR})):
        idx[key] = FAISSIndex(256, index_type="IVFPQ", nlist=nlist, nprobe=nprobe, **kw)
        idx[key].add(x)
    idx["ivf_flat"] = FAISSIndex(256, index_type="IVF", nlist=nlist, nprobe=nprobe)
    idx["ivf_flat"].add(x)
    flat = FAISSIndex(256, index_type="Flat")
    flat.add(x)
    del x
    torch.cuda.empty_cache()
    kc = ivfpq.refine_candidates(K, FACTOR)
    for B in BATCHES:
        q = torch.randn((B, 256), generator=g, device=dev)
        fids = flat.search_device(q, K)[0].cpu().numpy()
        ms = {key: timed(lambda i=i: i.search_device(q, K)) for key, i in idx.items()}
        ms["ivfpq_at_kc"] = timed(lambda: idx["ivfpq"].search_device(q, kc))
        rec_at = {key: recall(i.search_device(q, K)[0].cpu().numpy(), fids) for key, i in idx.items()}
        rr = {}
        for key, row_bytes in (("refine_fp32", 1024), ("refine_bf16", 512)):
            t = rerank_ms(lambda key=key: idx[key].search_device(q, K))
            gb = B * kc * row_bytes / 1e9
            rr[key] = {"ms": round(t, 4), "row_gbytes": round(gb, 4), "tb_per_s": round(gb / t, 3),
                       "share_of_achievable": round(gb / t / ACHIEVABLE_TBPS, 3)}
        rec = {"shape": name, "n": n, "nlist": nlist, "nprobe": nprobe, "B": B, "k": K, "kc": kc, "pq_m": 8, "factor": FACTOR,
               "search_ms": {key: round(v, 4) for key, v in ms.items()}, "rerank_kernel": rr,
               "recall_at_k_vs_flat": {key: round(v, 4) for key, v in rec_at.items()},
               "device_bytes_per_ad": {key: round(resident_bytes(i) / n, 2) for key, i in idx.items()}}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    del idx, flat
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1m,10m")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for s in a.shapes.split(","):
        run_shape(s, out)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "achievable_tb_per_s": ACHIEVABLE_TBPS, "rows": out}, f,
                      indent=1)


if __name__ == "__main__":
    main()
