"""Dev tool: what per-request eligibility masks cost in the Flat search (bf16 engine).  1M x 256 randn rows, k = 500, batch B in
{1, 32, 512}; per cell: search time (HIP events, mean of REPS searches over ROT rotating query batches), the filtered kernels
alone (amdrec_profile_* tags with "_elig"), n_fixup of one search, and - the floor, and what a user would otherwise maintain -
the plain search of a Flat index built from the eligible rows alone.
Cells: no masks; zero masks (every row eligible, the filtered kernels); a fraction f = 0.5 / 0.1 / 0.01 of the corpus
eligible; and 300 eligible rows, fewer than k: every query takes the exact fix-up scan.
usage: python tools/eligible_latency.py [--out FILE] [--n ROWS]"""
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

BATCHES, K, REPS, ROT, FEW = (1, 32, 512), 500, 20, 4, 300
FRACTIONS = ((0.5, 1 << 0), (0.1, 1 << 33), (0.01, 1 << 62))          # (eligible fraction, the tag bit that marks it)
FEW_BIT = 1 << 5


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


def word(bit, B, dev):
    return torch.full((B,), bit - (1 << 64) if bit >> 63 else bit, dtype=torch.int64, device=dev)


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
    idx = FAISSIndex(256, index_type="Flat")
    idx.add(x, tags=tags)
    cells = [("none", None, None), ("zero masks", 0, None)] + [(f"f={f}", bit, bit) for f, bit in FRACTIONS] + \
            [(f"{FEW} eligible rows", FEW_BIT, FEW_BIT)]
    subs = {}
    for name, bit, sub_bit in cells:
        if sub_bit is not None:
            keep = torch.nonzero(tags & sub_bit).flatten()
            s = FAISSIndex(256, index_type="Flat")
            s.add(x[keep])
            subs[name] = (s, int(keep.numel()))
    out = []
    for B in BATCHES:
        qs = [torch.randn((B, 256), generator=g, device=dev) for _ in range(ROT)]
        zero = torch.zeros(B, dtype=torch.int64, device=dev)
        for name, bit, _ in cells:
            if bit is None:
                fn = lambda i: idx.search_device(qs[i % ROT], K)                               # noqa: E731
            else:
                ma = word(bit, B, dev) if bit else zero
                fn = lambda i: idx.search_device(qs[i % ROT], K, require_all=ma, require_any=zero)   # noqa: E731
            reps = 4 if bit == FEW_BIT else REPS                      # (the exact scan of every query: seconds at B = 512)
            per, total = kernels_ms(fn, min(reps, 10))
            rec = {"B": B, "n": n, "k": K, "masks": name, "search_ms": round(timed(fn, reps), 4), "kernels_ms_per_search": total,
                   "kernel_ms": per, "n_fixup": n_fixup(idx, fn)}
            if name in subs:
                s, rows = subs[name]
                rec["eligible_rows"] = rows
                rec["index_of_eligible_rows_ms"] = round(timed(lambda i: s.search_device(qs[i % ROT], K)), 4)
            print(json.dumps(rec), flush=True)
            out.append(rec)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": REPS, "rotating_inputs": ROT, "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
