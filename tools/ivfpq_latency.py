"""Dev tool: IVFPQ search against IVF-Flat on the same corpus, same box, same run.  Per shape and batch: total search time
(HIP events, mean of REPS searches), IVFPQ per-stage device times (coarse probes, distance tables, table-lookup scan,
final select; amdrec_profile_* tags), recall@k of both against Flat, and the indexes' resident device bytes per ad.
usage: python tools/ivfpq_latency.py [--shapes 1m,10m] [--out FILE]
  1m : 1M x 256, nlist 100 / nprobe 10 (the reference's defaults)      10m: 10M x 256, nlist 4096 / nprobe 64
B in {1, 32, 512}, k = 500, pq_m = 8.  Corpus and queries: torch.randn (as the reference's benchmark, :390-391)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommender-demo_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from amdrec import _lib  # noqa: E402
from amdrec.index import FAISSIndex  # noqa: E402

SHAPES = {"1m": (1_000_000, 100, 10), "10m": (10_000_000, 4096, 64)}
BATCHES, K, REPS = (1, 32, 512), 500, 20


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


def profiled(fn, reps=5):
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    for _ in range(reps):
        fn()
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    return {k: v["total_ms"] / reps for k, v in rep.items()}


def nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts if isinstance(t, torch.Tensor))


def resident_bytes(idx):
    """Device bytes the index holds once searched: ids, assignment, the list-contiguous copy and its row -> position map,
    and the vectors (IVF-Flat: the fp32 rows, their list-contiguous copy and, if built, its bf16 shadow) or the codes
    (IVFPQ: in insertion order and list-contiguous, and the per-row finite flags).  Centroids, codebooks and workspaces are
    per index, not per ad."""
    lists = idx._ivf.lists
    per_list = () if lists is None else (lists.rows, lists.spos, lists.off, lists.lens)
    if idx._pq is not None:
        return nbytes(idx._ids, idx._pq.codes, idx._pq.finite, idx._pq.assign, *per_list)
    return nbytes(idx._ids, idx._xb, idx._ivf.assign, *per_list, *(idx._ivf._shadow or ()))


def recall(ids, ref):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / ref.shape[1] for a, b in zip(ids, ref)]))


def run_shape(name, out):
    n, nlist, nprobe = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.randn((n, 256), generator=g, device=dev)
    t0 = time.time()
    pq = FAISSIndex(256, index_type="IVFPQ", nlist=nlist, nprobe=nprobe)
    pq.add(x)
    torch.cuda.synchronize()
    pq_add = time.time() - t0
    t0 = time.time()
    ivf = FAISSIndex(256, index_type="IVF", nlist=nlist, nprobe=nprobe)
    ivf.add(x)
    torch.cuda.synchronize()
    ivf_add = time.time() - t0
    flat = FAISSIndex(256, index_type="Flat")
    flat.add(x)
    del x
    torch.cuda.empty_cache()
    st = pq._pq
    for B in BATCHES:
        q = torch.randn((B, 256), generator=g, device=dev)
        qn = pq._normalize_(q.clone())
        fids, _ = flat.search_device(q, K)
        ms_pq = timed(lambda: pq.search_device(q, K))
        ms_ivf = timed(lambda: ivf.search_device(q, K))
        ids_pq, _ = pq.search_device(q, K)
        ids_ivf, _ = ivf.search_device(q, K)
        torch.cuda.synchronize()
        pq_bytes, ivf_bytes = resident_bytes(pq), resident_bytes(ivf)
        prof = profiled(lambda: pq.search_device(q, K))
        ms_coarse = timed(lambda: st.coarse_probes(qn, nprobe))
        prof_coarse = profiled(lambda: st.coarse_probes(qn, nprobe))
        # lists' rows scanned per query (codes: m bytes a row) and pool keys written (8 bytes each)
        probes = st.coarse_probes(qn, nprobe).cpu().numpy()
        lens = np.bincount(st.assign.cpu().numpy(), minlength=nlist)
        rows = int(sum(lens[p[p >= 0]].sum() for p in probes))
        rec = {"shape": name, "n": n, "nlist": nlist, "nprobe": nprobe, "B": B, "k": K, "pq_m": st.m,
               "ivfpq_ms": round(ms_pq, 4), "ivf_flat_ms": round(ms_ivf, 4),
               "stages_ms": {"coarse": round(ms_coarse, 4),
                             "tables": round(prof.get("ivfpq_tables", 0.0), 4),
                             "scan": round(prof.get("ivfpq_scan", 0.0), 4),
                             "select": round(prof.get("ivf_select", 0.0) - prof_coarse.get("ivf_select", 0.0), 4)},
               "ivfpq_kernel_tags_ms": {k: round(v, 4) for k, v in sorted(prof.items())},
               "recall_at_k_vs_flat": {"ivfpq": round(recall(ids_pq.cpu().numpy(), fids.cpu().numpy()), 4),
                                       "ivf_flat": round(recall(ids_ivf.cpu().numpy(), fids.cpu().numpy()), 4)},
               "scanned_rows": rows, "pool_key_bytes": rows * 8, "code_bytes_scanned": rows * st.m,
               "table_bytes": B * nprobe * st.m * 256 * 4,
               "device_bytes_per_ad": {"ivfpq": round(pq_bytes / n, 2), "ivf_flat": round(ivf_bytes / n, 2)},
               "add_s": {"ivfpq": round(pq_add, 2), "ivf_flat": round(ivf_add, 2)}}
        line = json.dumps(rec)
        print(line, flush=True)
        out.append(rec)
    del pq, ivf, flat
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
            json.dump({"device": torch.cuda.get_device_name(0), "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
