"""Dev tool: are two builds of the library bit-identical on the layer-by-layer engine (csrc/layers.hip, csrc/tower_small.hip and
the launchers of csrc/gemm_core.hpp) - and do they launch the same kernels?  Per case it saves the outputs AND the profile-tag
list (amdrec_profile_enable: tag, launches, algorithmic flops and bytes): with identical kernels the tags are what catches a
wrong shape or engine choice that would still pass the float64 tolerances.
  towers  (tests/cases.py): the default towers at 1, 257, 1025, 4096 (GEMV R = 1 / 2, pipe, fused kernels), 4097 and 9001 rows
          (small and wide tile shapes); single_linear, past_ts_width (also at 17 rows), eight_layers, no_numerical at 4097 and
          9001; single_linear at ROW_CHUNK + 1 rows (second pass)
  ranker  engines fp32 and bf16x6 at 17, 4097 and 9001 rows: default, narrow, minimal, wide_embed, past_param_edge, six_layers,
          no_numerical; engine f16x3, default at 500 rows (the projection in front of the row-owner kernel)
  score_candidates with and without the ad-projection cache at U = 3, k = 500 (small user-projection kernel, split projection)
          and U = 65, k = 160 (tile GEMM), engines fp32 and f16x3; the caches ensure_ad_cache builds (project_ads, both widths)
Each library (AMDREC_LIB_PATH, amdrec/_lib.py) runs in its own fresh child process under its own time limit; a child that fails
ends the run.  The parent process never touches the GPU: it compares what the children saved with torch.equal and ==.
Log: profiles/layers_dispatch_bitident.log.
usage: python tools/layers_bitident.py LIB_A LIB_B"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import warnings

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "movie-recommender-demo_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROW_CHUNK = 262144
TOWER_CASES = [("default", (1, 257, 1025, 4096, 4097, 9001)), ("single_linear", (4097, 9001, ROW_CHUNK + 1)),
               ("past_ts_width", (17, 4097, 9001)), ("eight_layers", (4097, 9001)), ("no_numerical", (4097, 9001))]
RANKER_CASES = ["default", "narrow", "minimal", "wide_embed", "past_param_edge", "six_layers", "no_numerical"]
RANKER_ROWS = (17, 4097, 9001)
BROADCAST = [(3, 500), (65, 160)]
N_ADS = 5000
CHILD_SECONDS = 420


def child(out_path):
    from amdrec import _lib, synth
    from amdrec.ranker import TransformerRanker
    from amdrec.towers import TwoTowerModel
    from tests import cases
    dev = torch.device("cuda:0")
    tensors, tags = {}, {}
    t = lambda sd: {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}         # noqa: E731
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                 # noqa: E731

    def run(key, fn):
        _lib.profile_enable(True)
        try:
            with torch.no_grad(), warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                out = fn()
            torch.cuda.synchronize()
            rep = _lib.profile_report()
        finally:
            _lib.profile_enable(False)
        tags[key] = sorted([k, int(v["launches"]), float(v["flops"]), float(v["bytes"])] for k, v in rep.items())
        for name, v in (out.items() if isinstance(out, dict) else [("out", out)]):
            tensors[f"{key}/{name}"] = v.detach().cpu()

    for name, row_counts in TOWER_CASES:
        if name == "default":
            user, ad, nnum, sd, _ = cases.two_tower_case("demo")
            args = cases.arch("demo")["tt"]
        else:
            user, ad, nnum, sd = cases.surface_tower_case(name)
            args = cases.TOWER_SURFACE[name][0]
        m = TwoTowerModel(dict(user), dict(ad), nnum, **args)
        m.load_state_dict(t(sd))
        m = m.to(dev).eval()
        for rows in row_counts:
            uc, un = synth.user_batch(user, nnum, rows, seed=rows)
            ac = synth.ad_features(ad, rows, seed=rows + 1)
            run(f"tower/{name}/rows{rows}/user", lambda: m.get_user_embeddings(cu(uc), cu(un)))
            run(f"tower/{name}/rows{rows}/ad", lambda: m.get_ad_embeddings(cu(ac)))

    def ranker(name, engine):
        if name == "default":
            user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
            args = cases.arch("demo")["rk"]
        else:
            user, ad, nnum, sd = cases.surface_ranker_case(name, "scaled")
            args = cases.RANKER_SURFACE[name][0]
        m = TransformerRanker(dict(user), dict(ad), nnum, **args)
        m.load_state_dict(t(sd))
        m.gemm_engine = engine
        return m.to(dev).eval(), (user, ad, nnum)

    for name in RANKER_CASES:
        for engine, row_counts in (("fp32", RANKER_ROWS), ("bf16x6", RANKER_ROWS), ("f16x3", (500,) if name == "default" else ())):
            if not row_counts:
                continue
            m, (user, ad, nnum) = ranker(name, engine)
            n = max(row_counts)
            uc, un = synth.user_batch(user, nnum, n, seed=81)
            ac = synth.ad_features(ad, n, seed=82)
            for rows in row_counts:
                run(f"ranker/{name}/{engine}/rows{rows}", lambda: m(cu(uc[:rows]), cu(ac[:rows]), cu(un[:rows])))

    for name, engine in (("wide_embed", "fp32"), ("default", "f16x3")):
        for U, k in BROADCAST:
            m, (user, ad, nnum) = ranker(name, engine)
            uc, un = synth.user_batch(user, nnum, U, seed=U)
            table = cu(synth.ad_features(ad, N_ADS, seed=U + 1))
            cand = cu(np.random.default_rng(U + 2).integers(0, N_ADS, (U, k)))
            key = f"score_candidates/{name}/{engine}/U{U}k{k}"
            run(f"{key}/uncached", lambda: m.score_candidates(cu(uc), cu(un), cand, table, check_indices=True))

            def caches():
                m.ensure_ad_cache(table)
                hid = m._hidden_cache_for(table)
                return {"proj": m._cache_for(table), **({} if hid is None else {"hidden": hid})}
            run(f"{key}/ensure_ad_cache", caches)
            run(f"{key}/cached", lambda: m.score_candidates(cu(uc), cu(un), cand, table, check_indices=True))
    torch.save({"tensors": tensors, "tags": tags}, out_path)


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    libs = sys.argv[1:3]
    saved = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(libs):
            path = os.path.join(tmp, f"layers_bitident_{i}.pt")
            r = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child", path],
                               env={**os.environ, "AMDREC_LIB_PATH": os.path.abspath(lib)})
            if r.returncode != 0:
                print(json.dumps({"lib": lib, "exit": r.returncode, "result": "child failed: nothing more was started"}))
                return 1
            saved.append(torch.load(path))
    (a, ta), (b, tb) = ((s["tensors"], s["tags"]) for s in saved)
    assert sorted(a) == sorted(b) and sorted(ta) == sorted(tb)
    differ = [k for k in sorted(a) if not torch.equal(a[k], b[k])]
    tags_differ = [k for k in sorted(ta) if ta[k] != tb[k]]
    finite = all(torch.isfinite(v).all().item() for v in a.values())
    sha = [hashlib.sha256(b"".join(d[k].contiguous().view(torch.uint8).numpy().tobytes() for k in sorted(d))).hexdigest() for d in (a, b)]
    for k in sorted(ta):
        outs = [o for o in sorted(a) if o.startswith(k + "/")]
        print(f"{'equal ' if not any(o in differ for o in outs) else 'DIFFER'} {'tags equal ' if k not in tags_differ else 'TAGS DIFFER'} {k} "
              f"{[tuple(a[o].shape) for o in outs]} " + " ".join(f"{t[0]}x{t[1]}" for t in ta[k]))
        if k in tags_differ:
            print(f"    other library: {tb[k]}")
    print(json.dumps({"libs": libs, "cases": len(ta), "tensors": len(a), "differ": differ, "tags_differ": tags_differ,
                      "all_finite": finite, "sha256": sha,
                      "result": "bit-identical, same launches" if not differ and not tags_differ else "DIFFERENT"}))
    return 1 if differ or tags_differ or not finite else 0


if __name__ == "__main__":
    sys.exit(main())
