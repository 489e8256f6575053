"""Dev tool: what a per-request include list costs.  Flat index over 1M x 256 randn rows, batch B in {1, 512}, k = 500 and
I in {8, 64}: same-run A/B of search_device without and with a list (HIP events, mean of REPS searches over ROT rotating
query batches and list blocks; the two arms interleaved, so that clock and cache state drift hits both), the merge kernel
alone (amdrec_profile_* tag include_merge), and beside it the exclude_compact launch of a search with an exclusion list of
E = I entries.  The lists name random corpus rows: none of them is in the result, so every entry is scored and merged in
(the expensive case: I random 1 KB row reads per query).
usage: python tools/include_latency.py [--out FILE] [--pkg DIR] [--n ROWS]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "include_merge.json"))
ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommender-demo_amd"))
ap.add_argument("--n", type=int, default=1_000_000)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.pkg))
import torch  # noqa: E402
from amdrec import _lib  # noqa: E402
from amdrec.index import FAISSIndex  # noqa: E402

BATCHES, K, WIDTHS, REPS, ROT = (1, 512), 500, (8, 64), 20, 4


def timed_ab(fa, fb, reps=REPS):
    """Mean ms of fa(i) and of fb(i), measured in alternation (a, b, a, b, ...) with one event pair per call."""
    for i in range(3):
        fa(i)
        fb(i)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    for i in range(reps):
        ev[i][0].record()
        fa(i)
        ev[i][1].record()
        ev[i][2].record()
        fb(i)
        ev[i][3].record()
    torch.cuda.synchronize()
    return (sum(e[0].elapsed_time(e[1]) for e in ev) / reps, sum(e[2].elapsed_time(e[3]) for e in ev) / reps)


def kernel_ms(fn, tag, reps=10):
    torch.cuda.synchronize()
    _lib.profile_enable(True, only=tag)
    for i in range(reps):
        fn(i)
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    return rep[tag]["total_ms"] / rep[tag]["launches"]


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    idx = FAISSIndex(256, index_type="Flat")
    idx.add(torch.randn((ARGS.n, 256), generator=g, device=dev))
    rows = []
    for B in BATCHES:
        qs = [torch.randn((B, 256), generator=g, device=dev) for _ in range(ROT)]
        for width in WIDTHS:
            ls = [torch.randint(0, ARGS.n, (B, width), generator=g, device=dev) for _ in range(ROT)]
            plain, listed = timed_ab(lambda i: idx.search_device(qs[i % ROT], K),
                                     lambda i: idx.search_device(qs[i % ROT], K, include=ls[i % ROT]))
            inj = sum(int(idx.search_device(qs[r], K, include=ls[r], return_injected=True)[2].sum()) for r in range(ROT))
            row = {"index": "Flat", "n": ARGS.n, "B": B, "k": K, "I": width, "search_ms": round(plain, 4),
                   "search_include_ms": round(listed, 4), "delta_ms": round(listed - plain, 4),
                   "injected_per_query": inj / (ROT * B),
                   "include_merge_kernel_ms": round(kernel_ms(
                       lambda i: idx.search_device(qs[i % ROT], K, include=ls[i % ROT]), "include_merge"), 4),
                   "exclude_compact_kernel_ms_at_E=I": round(kernel_ms(
                       lambda i: idx.search_device(qs[i % ROT], K, exclude=ls[i % ROT]), "exclude_compact"), 4)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": REPS, "rotating_inputs": ROT, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
