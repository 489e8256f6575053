"""Dev tool: what per-request eligibility masks cost in the inverted-list scans (FAISSIndex(..., list_tags=True)).  1M x 256 randn
rows, k = 500, batch B in {1, 32, 512}; indexes IVF(100, 10), IVF(1024, 32) with AMDREC_IVF_MIXED=0 and =1, IVFPQ(1024, 32, m 8).
Per cell: search time (HIP events, mean of REPS searches over ROT rotating query batches, after 3 warm-up searches) and the scan /
select kernels alone (amdrec_profile_* tags), and - the floor for the filter - the plain search of the twin index: built
identically (same quantizer, same codebooks), the ineligible rows then taken out with remove_ids.
Cells: no masks; zero masks (every row eligible, the filtered kernels); a fraction f = 0.5 / 0.1 / 0.01 of the corpus eligible;
and 300 eligible rows, fewer than k: the first phase's threshold stays at -inf.
usage: python tools/ivf_eligible_latency.py [--out FILE] [--n ROWS] [--only NAME]"""
import argparse
import json
import os
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--only", default=None, help="one of the index names below")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommender-demo_amd"))
import torch  # noqa: E402
from amdrec import _lib  # noqa: E402
from amdrec.index import FAISSIndex  # noqa: E402

BATCHES, K, REPS, ROT, FEW = (1, 32, 512), 500, 20, 4, 300
FRACTIONS = ((0.5, 1 << 0), (0.1, 1 << 33), (0.01, 1 << 62))          # (eligible fraction, the tag bit that marks it)
FEW_BIT = 1 << 5
# name -> (index type, nlist, nprobe, AMDREC_IVF_MIXED or None)
INDEXES = {"IVF(100,10)": ("IVF", 100, 10, None), "IVF(1024,32) fp32 filter": ("IVF", 1024, 32, "0"),
           "IVF(1024,32) bf16 prefilter": ("IVF", 1024, 32, "1"), "IVFPQ(1024,32,m8)": ("IVFPQ", 1024, 32, None)}


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
    """-> {tag: ms per search} of the search's list-scan and select kernels"""
    torch.cuda.synchronize()
    _lib.profile_enable(True, only="iv")
    for i in range(reps):
        fn(i)
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    return {t: round(e["total_ms"] / reps, 4) for t, e in sorted(rep.items())}


def word(bit, B, dev):
    return torch.full((B,), bit - (1 << 64) if bit >> 63 else bit, dtype=torch.int64, device=dev)


def build(kind, nlist, nprobe, x, tags, like=None):
    """An opted-in index over x; ``like``: an index whose quantizer (and codebooks) the new one takes over."""
    idx = FAISSIndex(256, index_type=kind, nlist=nlist, nprobe=nprobe, list_tags=True)
    if like is None:
        idx.add(x, tags=tags)
    elif kind == "IVF":
        idx.set_trained_centroids(like.centroids)
        idx.add(x, tags=tags)
    else:                                                           # IVFPQ: the same file, read twice
        with tempfile.TemporaryDirectory() as d:
            like.save(os.path.join(d, "ix"))
            idx.load(os.path.join(d, "ix"))
    return idx


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    n = ARGS.n
    x = torch.randn((n, 256), generator=g, device=dev)
    tags = torch.zeros(n, dtype=torch.int64, device=dev)
    for f, bit in FRACTIONS:
        tags |= (torch.rand(n, generator=g, device=dev) < f).to(torch.int64) * bit
    tags[torch.randperm(n, generator=g, device=dev)[:FEW]] |= FEW_BIT
    cells = [("none", None), ("zero masks", 0)] + [(f"f={f}", bit) for f, bit in FRACTIONS] + [(f"{FEW} eligible rows", FEW_BIT)]
    qs = {B: [torch.randn((B, 256), generator=g, device=dev) for _ in range(ROT)] for B in BATCHES}
    out, built = [], {}
    for name, (kind, nlist, nprobe, mixed) in INDEXES.items():
        if ARGS.only and name != ARGS.only:
            continue
        if mixed is None:
            os.environ.pop("AMDREC_IVF_MIXED", None)
        else:
            os.environ["AMDREC_IVF_MIXED"] = mixed
        key = (kind, nlist, nprobe)
        if key not in built:                                        # (the two IVF(1024,32) arms share index and twins)
            built.clear()
            idx = build(kind, nlist, nprobe, x, tags)
            twins = {}
            for cname, bit in cells:
                if bit:
                    twin = build(kind, nlist, nprobe, x, tags, like=idx)
                    gone = torch.nonzero((tags & bit) == 0).flatten()
                    twin.remove_ids(gone)
                    twins[cname] = (twin, n - int(gone.numel()))
            built[key] = (idx, twins)
        idx, twins = built[key]
        for B in BATCHES:
            zero = torch.zeros(B, dtype=torch.int64, device=dev)
            for cname, bit in cells:
                if bit is None:
                    fn = lambda i: idx.search_device(qs[B][i % ROT], K)                                  # noqa: E731
                else:
                    ma = word(bit, B, dev) if bit else zero
                    fn = lambda i: idx.search_device(qs[B][i % ROT], K, require_all=ma, require_any=zero)    # noqa: E731
                rec = {"index": name, "B": B, "n": n, "k": K, "masks": cname, "search_ms": round(timed(fn), 4),
                       "kernel_ms_per_search": kernels_ms(fn)}
                if cname in twins:
                    twin, rows = twins[cname]
                    rec["eligible_rows"] = rows
                    rec["twin_after_remove_ids_ms"] = round(timed(lambda i: twin.search_device(qs[B][i % ROT], K)), 4)
                print(json.dumps(rec), flush=True)
                out.append(rec)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": 3, "rotating_inputs": ROT,
                       "runs_per_cell": 1, "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
