"""Dev tool: per-launch time of the top-k tags (search_finalize_mixed, search_fixup, ivf_select, ivfpq_rerank) by the
library's own timing hook, at the shapes of bench.py's search, tools/ivf_latency.py and tools/ivfpq_refine_latency.py; one
JSON line {tag@shape: mean ms per launch}.  For A/B runs of two builds of the library (AMDREC_LIB_PATH) in alternating fresh
processes: profiles/topk_helpers_ab.log.
usage: AMDREC_LIB_PATH=/path/to/libamdrec.so python tools/topk_tags_time.py"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "movie-recommender-demo_amd"))
import torch  # noqa: E402
from amdrec import _lib  # noqa: E402
from amdrec.index import FAISSIndex  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(1)
REPS = 30
out = {}


def tags(fn, prefix, reps=REPS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    _lib.profile_enable(True, only=prefix)
    for _ in range(reps):
        fn()
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    return {t: v["total_ms"] / v["launches"] for t, v in rep.items()}


x = torch.randn((1_000_000, 256), generator=g, device=dev)
flat = FAISSIndex(256, index_type="Flat")
flat.add(x)
for B in (1, 32, 512):
    q = torch.randn((B, 256), generator=g, device=dev)
    for pre in ("search_finalize_mixed", "search_fixup"):
        for t, ms in tags(lambda: flat.search_device(q, 500), pre).items():
            out[f"{t}@B{B}"] = ms
# the small finalize shapes (256 queries, short lists)
xs = x[:20_000, :64].contiguous()
small = FAISSIndex(64, index_type="Flat")
small.add(xs)
q = torch.randn((256, 64), generator=g, device=dev)
for k in (64, 300):
    for t, ms in tags(lambda: small.search_device(q, k), "search_finalize_mixed").items():
        out[f"{t}@20k_B256_k{k}"] = ms
del flat, small
ivf = FAISSIndex(256, index_type="IVF", nlist=100, nprobe=10)
ivf.add(x)
for B in (1, 8, 64, 512):
    q = torch.randn((B, 256), generator=g, device=dev)
    rep = tags(lambda: ivf.search_device(q, 500), "ivf_select")
    out[f"ivf_select@B{B}"] = rep["ivf_select"]
del ivf
# ivfpq_rerank at the refine tool's shape: 1M x 256 rows, kc = 2000 candidates, k = 500
x16 = x.to(torch.bfloat16)
for B in (1, 32, 512):
    q = torch.randn((B, 256), generator=g, device=dev)
    cand = torch.stack([torch.randperm(1_000_000, generator=g, device=dev)[:2000] for _ in range(B)]).contiguous()
    D = torch.empty((B, 500), dtype=torch.float32, device=dev)
    I = torch.empty((B, 500), dtype=torch.int64, device=dev)
    ws = torch.zeros(B * 2000, dtype=torch.int64, device=dev)
    tk = torch.zeros(B, dtype=torch.int32, device=dev)
    for name, rows, b16 in (("fp32", x, 0), ("bf16", x16, 1)):
        def run():
            _lib.check(lib.amdrec_ivfpq_rerank(_lib.ptr(rows), b16, 1_000_000, 256, 256, None, _lib.ptr(q), B, 256, _lib.ptr(cand),
                                               2000, 0, 500, _lib.ptr(D), _lib.ptr(I), _lib.ptr(ws), ws.numel() * 8, _lib.ptr(tk),
                                               _lib.stream_ptr(dev)))
        out[f"ivfpq_rerank_{name}@B{B}"] = tags(run, "ivfpq_rerank")["ivfpq_rerank"]
print(json.dumps({k: round(v, 5) for k, v in out.items()}))
