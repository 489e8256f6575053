"""Dev tool: are two builds of the library bit-identical on the row-owner ranker kernels?  For the `demo` case every prefix
length of amdrec_ranker_x3_prefix at 429, 4429 and 16813 rows (the column-split, the 64-row and the 128-row shape of the
16-row kernel, each with a ragged tail; 429 rows on the 32-row kernel too) and one amdrec_ranker_forward pass through the
folded + hidden-cache program at 16385 rows (tests/test_ffn1_cache_gpu.py).  Each library (AMDREC_LIB_PATH, amdrec/_lib.py)
runs in its own fresh child process under its own time limit; a child that fails ends the run.  The parent process never
touches the GPU: it compares the saved row states and logits with torch.equal.  Log: profiles/x3b_strip_bitident.log.
usage: python tools/x3_bitident.py LIB_A LIB_B"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "movie-recommender-demo_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

PREFIX_ROWS = [128 * 3 + 45, 4096 + 64 * 5 + 13, 16384 + 128 * 3 + 45]
N_ADS, USERS, K = 2000, 5, 3277             # 16385 rows: the smallest pass that takes the hidden-cache program
CHILD_SECONDS = 240


def child(out_path):
    from amdrec import _lib, synth
    from amdrec.ranker import TransformerRanker
    from tests import cases
    lib = _lib.load()
    dev = torch.device("cuda:0")
    out = {}

    def model(cross):
        user, ad, nnum, sd, _ = cases.ranker_case("demo", cross)
        m = TransformerRanker(dict(user), dict(ad), nnum, **cases.arch("demo")["rk"])
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        return m.to(dev).eval(), (user, ad, nnum)

    m, _ = model("randn")
    gen = torch.Generator().manual_seed(41)
    for variant, row_counts in ((16, PREFIX_ROWS), (32, PREFIX_ROWS[:1])):
        m.x3_variant = variant
        params, tasks = m._pack(dev)
        n_total = 2 * len(m.transformer_layers) + 3 + 1
        for rows in row_counts:
            X = torch.randn(rows, 256, generator=gen).to(dev)
            ws = torch.empty(((rows + 127) // 128) * 128 * 1024, dtype=torch.uint8, device=dev)
            for n in range(1, n_total + 1):
                x_out = torch.full((rows, 256), float("nan"), dtype=torch.float32, device=dev)
                logits = torch.full((len(tasks), rows), float("nan"), dtype=torch.float32, device=dev)
                _lib.check(lib.amdrec_ranker_x3_prefix(C.byref(params), _lib.ptr(X), X.stride(0), rows, n, _lib.ptr(x_out),
                                                       x_out.stride(0), _lib.ptr(logits), logits.stride(0), _lib.ptr(ws),
                                                       ws.numel(), _lib.stream_ptr(dev)))
                torch.cuda.synchronize()
                out[f"prefix/variant{variant}/rows{rows}/n{n}/x"] = x_out.cpu()
                if n == n_total:
                    out[f"prefix/variant{variant}/rows{rows}/n{n}/logits"] = logits.cpu()

    # the folded + hidden-cache program through amdrec_ranker_forward (score_candidates on a cached ad table)
    m, (user, ad, nnum) = model("scaled")
    uc, un = synth.user_batch(user, nnum, USERS, seed=81)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    table = cu(synth.ad_features(ad, N_ADS, seed=82))
    cand = np.random.default_rng(K).integers(0, N_ADS, (USERS, K))
    m.gemm_engine, m.cache_first_ffn = "f16x3", True
    m.ensure_ad_cache(table)
    _lib.profile_enable(True)
    got = m.score_candidates(cu(uc), cu(un), cu(cand), table, check_indices=True)
    torch.cuda.synchronize()
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    tag = "ranker_rowowner16_128_x3"
    rows = USERS * K
    assert m._hidden_cache_for(table) is not None and tag in rep, list(rep)
    assert rep[tag]["flops"] == 2.0 * rows * (2_146_496 - 256 * 1024), rep[tag]       # the cached program was priced
    for t, v in got.items():
        out[f"forward_hidden_cache/rows{rows}/{t}"] = v.cpu()
    torch.save(out, out_path)


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    libs = sys.argv[1:3]
    saved = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(libs):
            path = os.path.join(tmp, f"x3_bitident_{i}.pt")
            r = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child", path],
                               env={**os.environ, "AMDREC_LIB_PATH": os.path.abspath(lib)})
            if r.returncode != 0:
                print(json.dumps({"lib": lib, "exit": r.returncode, "result": "child failed: nothing more was started"}))
                return 1
            saved.append(torch.load(path))
    a, b = saved
    assert sorted(a) == sorted(b)
    differ = [k for k in sorted(a) if not torch.equal(a[k], b[k])]
    finite = all(torch.isfinite(v).all().item() for v in a.values())
    sha = [hashlib.sha256(b"".join(d[k].contiguous().view(torch.uint8).numpy().tobytes() for k in sorted(d))).hexdigest() for d in saved]
    for k in sorted(a):
        print(f"{'equal ' if k not in differ else 'DIFFER'} {k} {tuple(a[k].shape)}")
    print(json.dumps({"libs": libs, "tensors": len(a), "differ": differ, "all_finite": finite, "sha256": sha,
                      "result": "bit-identical" if not differ else "DIFFERENT"}))
    return 1 if differ or not finite else 0


if __name__ == "__main__":
    sys.exit(main())
