"""GPU: gemm_engine "f16" - the row-owner 16-row kernels with ONE fp16 product per MAC (csrc/rowowner16.hpp "SINGLE
PRODUCT") - held to the numpy model of its arithmetic (tests/f16_model.py).  The rule of this file: the kernel's error
against float64 is at most TWICE the model's on the same rows.  The two differ in the order of fp32 sums and in the rare
fp16 rounding such a difference flips, which move the error by percents; what a bug does - a lost k-step, a low fragment
set read for a high one, a stale plane, a hidden tile of the wrong row - moves it by orders of magnitude.  The factor is
not fitted.  Shapes: 53 rows (the 64-row workgroup shape, ragged) and 16685 rows (the 128-row shape with the paired FFN:
two full workgroups beyond 16384 plus a ragged one)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle
from amdrec import _lib, synth, weights
from tests import cases, f16_model

pytestmark = pytest.mark.gpu

ROWS_64, ROWS_128 = 16 * 3 + 5, 16384 + 128 * 2 + 45
TAG_64, TAG_128, TAG_WIN = "ranker_rowowner16_64_f16", "ranker_rowowner16_128_f16", "ranker_winner_heads_f16"


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _t(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _case(name, cross):
    if name in cases.CASES:
        user, ad, nnum, sd, _ = cases.ranker_case(name, cross)
        return user, ad, nnum, sd, cases.arch(name)["rk"]
    user, ad, nnum, sd = cases.surface_ranker_case(name, cross)
    return user, ad, nnum, sd, cases.RANKER_SURFACE[name][0]


def _model(name, cross, engine="f16", sd=None):
    from amdrec.ranker import TransformerRanker
    user, ad, nnum, sd0, args = _case(name, cross)
    sd = sd0 if sd is None else sd
    m = TransformerRanker(dict(user), dict(ad), nnum, **args)
    m.load_state_dict(_t(sd))
    m.gemm_engine = engine
    return m.cuda().eval(), sd, (user, ad, nnum)


def _projected_rows(sd, dims, rows, seed):
    user, ad, nnum = dims
    uc, un = synth.user_batch(user, nnum, rows, seed=seed)
    ac = synth.ad_features(ad, rows, seed=seed + 1)
    feats = oracle.ranker.embed_features(sd, uc, ac, un)
    return (feats @ sd["feature_projection.weight"].T + sd["feature_projection.bias"]
            + sd["positional_encoding"][0, 0]).astype(np.float32)


def _prefix(m, X, n_phases):
    """amdrec_ranker_x3_prefix under the model's engine -> (rows, logits, profile tags)."""
    lib = _lib.load()
    dev = X.device
    params, tasks = m._pack(dev)
    assert params.x3.products == (1 if m.gemm_engine == "f16" else 0)
    rows = X.shape[0]
    x_out = torch.full((rows, 256), float("nan"), dtype=torch.float32, device=dev)
    logits = torch.full((len(tasks), rows), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.empty(((rows + 127) // 128) * 128 * 1024, dtype=torch.uint8, device=dev)
    _lib.profile_enable(True)
    try:
        _lib.check(lib.amdrec_ranker_x3_prefix(C.byref(params), _lib.ptr(X), X.stride(0), rows, n_phases, _lib.ptr(x_out),
                                               x_out.stride(0), _lib.ptr(logits), logits.stride(0), _lib.ptr(ws), ws.numel(),
                                               _lib.stream_ptr(dev)))
        torch.cuda.synchronize()
        tags = [t for t in _lib.profile_report() if t.startswith("ranker_")]
    finally:
        _lib.profile_enable(False)
    return x_out.cpu().numpy(), logits.cpu().numpy(), tags


def _tag(rows):
    return TAG_64 if rows <= 16384 else TAG_128


# ---- 1. the exact case ---------------------------------------------------------------------------------------------------
def _exact_state(sd):
    """W_v = I, b_v = 0, W_o = integers of magnitude <= 2047 times 2^-9 in layer 1: with integer rows every operand of the
    first phase's GEMM is exact in one fp16 plane."""
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    p = "transformer_layers.0.self_attention."
    rng = np.random.default_rng(7)
    sd[p + "W_v.weight"] = np.eye(256, dtype=np.float32)
    sd[p + "W_v.bias"] = np.zeros(256, dtype=np.float32)
    wo = rng.integers(-2047, 2048, (256, 256)).astype(np.float32)
    wo[0, 0], wo[255, 255] = 2047.0, -2047.0
    sd[p + "W_o.weight"] = wo * np.float32(2.0 ** -9)
    return sd


@pytest.mark.parametrize("rows", [ROWS_64, ROWS_128])
def test_exact_operands_make_f16_and_f16x3_the_same_arithmetic(rows):
    """Every low plane is zero, so the three-product kernel adds zeros where the single-product kernel adds nothing: the
    first phase (attention + LN1, the fold off) must come out BIT-IDENTICAL from both engines."""
    sd = _exact_state(cases.ranker_case("demo", "scaled")[3])
    # the premise, checked on the host: the packed low fragment sets of that matrix are all zero
    wov = weights.ranker_chain(sd).layers[0]["wov"].astype(np.float32).astype(np.float64)
    assert np.array_equal(wov, sd["transformer_layers.0.self_attention.W_o.weight"].astype(np.float64))
    fr = weights.x3b_frags(wov, weights.x3_pow2_scale(np.abs(wov).max()))
    assert fr[:, :, 0].any() and not fr[:, :, 1].any()
    X = np.random.default_rng(rows).integers(-2047, 2048, (rows, 256)).astype(np.float32)
    X[0], X[1, :] = 0.0, 0.0
    X[1, 5], X[2, 0] = 1.0, 2047.0
    s, _ = f16_model.row_scale(X)
    assert not f16_model.planes(X * s)[1].any()
    Xd = _cu(X)
    out = {}
    for engine in ("f16", "f16x3"):
        m, _, _ = _model("demo", "scaled", engine, sd=sd)
        m.fold_first_attention = False
        x, _, tags = _prefix(m, Xd, 1)
        assert np.isfinite(x).all()
        if engine == "f16":
            assert tags == [_tag(rows)], tags
        out[engine] = x
    assert np.array_equal(out["f16"].view(np.uint32), out["f16x3"].view(np.uint32)), np.abs(out["f16"] - out["f16x3"]).max()


# ---- 2. every prefix of the chain ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [ROWS_64, ROWS_128])
@pytest.mark.parametrize("cross", ["scaled", "randn"])
@pytest.mark.parametrize("name", ["demo", "x3_one_layer", "x3_param_edge"])
def test_every_prefix_stays_within_twice_the_models_error(name, cross, rows, accuracy):
    m, sd, dims = _model(name, cross)
    assert m.gemm_engine_for(rows) == "f16"
    X = _projected_rows(sd, dims, rows, seed=41)
    truth = oracle.ranker.chain_states(sd, X, dtype=np.float64)
    chain = f16_model.Chain(sd, fold=True)
    model = chain.states(X)
    names = f16_model.phase_names(len(m.transformer_layers))
    assert len(truth) == len(model) == len(names) and chain.fold and m.fold_first_attention
    # Phase 1 is LayerNorm alone (layer 1's attention is folded): no fp16 operand, its whole error is the fp32 fold in front of
    # it, so there the model has to form z in the device's order - done for the first and the last rows of the launch
    sub = np.r_[0:min(rows, 64), max(rows - 45, 0):rows]
    ln_model = chain.ln(chain.fold_rows(X[sub], fma_chain=True), 0)[0]
    Xd = _cu(X)
    for n, pname in enumerate(names, start=1):
        x, logits, tags = _prefix(m, Xd, n)
        assert tags == [_tag(rows)], tags
        if n < len(names):
            assert np.isfinite(x).all(), pname
            if n == 1:
                rms, mx = f16_model.rel_errors(x[sub], truth[0][sub])
                rms_m, mx_m = f16_model.rel_errors(ln_model, truth[0][sub])
            else:
                rms, mx = f16_model.rel_errors(x, truth[n - 1])
                rms_m, mx_m = f16_model.rel_errors(model[n - 1], truth[n - 1])
            accuracy(f"f16_prefix/{name}_{cross}/rows{rows}/{pname}", "f16", max(rms / (2 * rms_m), mx / (2 * mx_m)),
                     rms_rel_err_vs_float64=rms, max_rel_err_vs_float64=mx, model_rms_rel_err_vs_float64=rms_m,
                     model_max_rel_err_vs_float64=mx_m, rms_ratio=rms / rms_m, max_ratio=mx / mx_m)
            assert rms <= 2 * rms_m, (pname, rms, rms_m)
            assert mx <= 2 * mx_m, (pname, mx, mx_m)
        else:
            for ti, t in enumerate(oracle.ranker.TASKS):
                e = float(np.abs(logits[ti].astype(np.float64) - truth[-1][t]).max())
                e_m = float(np.abs(model[-1][ti].astype(np.float64) - truth[-1][t]).max())
                accuracy(f"f16_prefix/{name}_{cross}/rows{rows}/heads/{t}", "f16", e / (2 * e_m), abs_err_vs_float64=e,
                         model_abs_err_vs_float64=e_m, logit_scale=float(np.abs(truth[-1][t]).max()))
                assert np.isfinite(logits[ti]).all() and e <= 2 * e_m, (t, e, e_m)


# ---- 3. the reference's golden batches through forward() ---------------------------------------------------------------
@pytest.mark.parametrize("cross", ["scaled", "randn"])
def test_golden_batches_through_forward(cross, accuracy):
    from tests.conftest import load_golden
    m, sd, _ = _model("demo", cross)
    g = load_golden(f"ranker_demo_{cross}.npz")
    chain = f16_model.Chain(sd, fold=True)
    for B in (1, 7, 64):
        assert m.gemm_engine_for(B) == "f16"
        uc, ac, un = g[f"B{B}_user_cat"], g[f"B{B}_ad_cat"], g[f"B{B}_user_num"]
        pred = m(_cu(uc), _cu(ac), _cu(un))
        feats = oracle.ranker.embed_features(sd, uc, ac, un).astype(np.float64)
        X = feats @ sd["feature_projection.weight"].astype(np.float64).T + sd["feature_projection.bias"] + \
            sd["positional_encoding"][0, 0]
        truth = oracle.ranker.chain_states(sd, X, dtype=np.float64)[-1]
        model = chain.states(X)[-1]
        for ti, t in enumerate(oracle.ranker.TASKS):
            e = float(np.abs(pred[t].cpu().numpy().astype(np.float64) - truth[t]).max())
            e_m = float(np.abs(model[ti].astype(np.float64) - truth[t]).max())
            accuracy(f"f16_golden/demo_{cross}/B{B}/{t}", "f16", e / (2 * e_m), abs_err_vs_float64=e, model_abs_err_vs_float64=e_m)
            assert e <= 2 * e_m, (B, t, e, e_m)


# ---- 4. robustness -----------------------------------------------------------------------------------------------------
def test_rows_spanning_sixty_binades_stay_finite():
    """tests/test_x3_gpu.py test_x3_extreme_rows_do_not_overflow's rows: the per-row scaling keeps the one plane in range."""
    m, sd, dims = _model("demo", "scaled")
    m.fold_first_attention = False
    X = _projected_rows(sd, dims, 256, seed=43)
    X[0] = 0.0
    X[1] *= 1e-30
    X[2] *= 1e6
    X[3, :] = 0.0
    X[3, 17] = 5e4
    truth = oracle.ranker.chain_states(sd, X, dtype=np.float64)
    model = f16_model.Chain(sd, fold=False).states(X)
    n = len(truth)
    x, logits, _ = _prefix(m, _cu(X), n)
    assert np.isfinite(x).all() and np.isfinite(logits).all()
    rms, _ = f16_model.rel_errors(x, truth[-2])
    rms_m, _ = f16_model.rel_errors(model[-2], truth[-2])
    assert rms <= 2 * rms_m, (rms, rms_m)


@pytest.mark.parametrize("rows", [ROWS_64, ROWS_128])
def test_nan_and_infinite_rows_leave_nan_logits_and_disturb_no_neighbour(rows):
    """A NaN in one row and an infinity in another: their logits are NaN in every task (x3_common.hpp keep_nan), and the 15
    other rows of their waves - and every other row - keep their bits."""
    m, sd, dims = _model("demo", "scaled")
    X = _projected_rows(sd, dims, rows, seed=45)
    bad = X.copy()
    r_nan, r_inf = 21, rows - 3
    bad[r_nan, 100] = np.nan
    bad[r_inf, 7] = np.inf
    n = len(f16_model.phase_names(3))
    _, clean, _ = _prefix(m, _cu(X), n)
    _, got, tags = _prefix(m, _cu(bad), n)
    assert tags == [_tag(rows)]
    assert np.isfinite(clean).all()
    assert np.isnan(got[:, [r_nan, r_inf]]).all()
    keep = np.ones(rows, dtype=bool)
    keep[[r_nan, r_inf]] = False
    assert np.array_equal(got[:, keep].view(np.uint32), clean[:, keep].view(np.uint32))
    for r in (r_nan, r_inf):                                             # the wave's other rows, named
        tile = np.arange(r // 16 * 16, min(r // 16 * 16 + 16, rows))
        tile = tile[tile != r]
        assert len(tile) >= 4 and np.array_equal(got[:, tile].view(np.uint32), clean[:, tile].view(np.uint32))


# ---- 5-8. the pipeline ---------------------------------------------------------------------------------------------------
SEED = 57


@functools.lru_cache(maxsize=None)
def _world():
    from amdrec.towers import TwoTowerModel
    user, ad, nnum = cases.small_dims()
    tt = TwoTowerModel(dict(user), dict(ad), nnum)
    tt.load_state_dict(_t(synth.two_tower_state(user, ad, nnum, seed=SEED)))
    rk_sd = synth.ranker_state(user, ad, nnum, seed=SEED + 1, cross_scale=cases.CROSS["scaled"])
    return dict(user=user, ad=ad, nnum=nnum, tt=tt.cuda().eval(), rk_sd=rk_sd, table=synth.ad_features(ad, 8192, seed=SEED + 2))


@functools.lru_cache(maxsize=None)
def _rec(n_ads, engine):
    from amdrec.index import FAISSIndex
    from amdrec.pipeline import AdRecommenderInference
    from amdrec.ranker import TransformerRanker
    w = _world()
    rk = TransformerRanker(dict(w["user"]), dict(w["ad"]), w["nnum"])
    rk.load_state_dict(_t(w["rk_sd"]))
    table = w["table"][:n_ads]
    idx = FAISSIndex(256, index_type="Flat")
    with torch.no_grad():
        idx.add(w["tt"].get_ad_embeddings(_cu(table)))
    rec = AdRecommenderInference(two_tower_model=w["tt"], transformer_ranker=rk, faiss_index=idx, ad_features=np.array(table),
                                 ranker_engine=engine)
    assert rec.transformer_ranker.gemm_engine == engine
    return rec


def _users(n, seed=31):
    w = _world()
    uc, un = synth.user_batch(w["user"], w["nnum"], n, seed=seed)
    return uc, un


def _clone(out):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _profiled(run):
    _lib.profile_enable(True)
    try:
        out = run()
        torch.cuda.synchronize()
        rep = _lib.profile_report()
    finally:
        _lib.profile_enable(False)
    return out, rep


def test_ctr_first_equals_all_heads_under_f16():
    B, k1, top_k = 3, 64, 10
    rec = _rec(1024, "f16")
    uc, un = (_cu(a) for a in _users(B))
    want = _clone(rec.recommend_device(uc, un, top_k, k1, heads="all"))
    got, rep = _profiled(lambda: _clone(rec.recommend_device(uc, un, top_k, k1, heads="ctr_first")))
    assert TAG_64 in rep and TAG_WIN in rep and not [t for t in rep if t.endswith("_x3")], list(rep)
    assert got["logits"].shape == (1, B * k1) and want["logits"].shape == (3, B * k1)
    assert torch.equal(got["ad_ids"], want["ad_ids"])
    assert torch.equal(got["logits"][0], want["logits"][0])
    assert torch.equal(got["scores"], want["scores"]) and got["scores"].shape == (3, B, top_k)      # the winners' other heads too
    assert bool(torch.isfinite(got["scores"]).all())


@functools.lru_cache(maxsize=None)
def _big_batch():
    """B = 40 users x 500 candidates of 8192 ads (20 000 rows: the 128-row shape) under f16 (cached and uncached first FFN)
    and f16x3, with float64 truth and the model on the same candidate rows, computed once."""
    B, k1, top_k = 40, 500, 10
    w = _world()
    uc, un = _users(B, seed=33)
    d_uc, d_un = _cu(uc), _cu(un)
    rec = _rec(8192, "f16")
    rk = rec.transformer_ranker
    assert rk.cache_first_ffn
    cached, rep_c = _profiled(lambda: _clone(rec.recommend_device(d_uc, d_un, top_k, k1)))
    rk.cache_first_ffn = False
    try:
        plain, rep_p = _profiled(lambda: _clone(rec.recommend_device(d_uc, d_un, top_k, k1)))
    finally:
        rk.cache_first_ffn = True
    x3 = _clone(_rec(8192, "f16x3").recommend_device(d_uc, d_un, top_k, k1))
    cand = cached["candidate_ids"].cpu().numpy()
    assert (cand >= 0).all() and np.array_equal(cand, x3["candidate_ids"].cpu().numpy())
    sd = w["rk_sd"]
    feats = oracle.ranker.embed_features(sd, np.repeat(uc, k1, axis=0), w["table"][cand.reshape(-1)], np.repeat(un, k1, axis=0))
    X = feats.astype(np.float64) @ sd["feature_projection.weight"].astype(np.float64).T + sd["feature_projection.bias"] + \
        sd["positional_encoding"][0, 0]
    truth = oracle.ranker.chain_states(sd, X, dtype=np.float64)[-1]
    model = f16_model.Chain(sd, fold=True).states(X)[-1]
    e_model = [float(np.abs(model[ti].astype(np.float64) - truth[t]).max()) for ti, t in enumerate(oracle.ranker.TASKS)]
    return dict(B=B, k1=k1, top_k=top_k, cached=cached, plain=plain, x3=x3, rep_c=rep_c, rep_p=rep_p, truth=truth, e_model=e_model)


def test_hidden_cache_under_f16(accuracy):
    b = _big_batch()
    rows = b["B"] * b["k1"]
    # the profile entry prices the program that ran: the cached one multiplies 256 x 1024 weight elements fewer per row
    assert b["rep_c"][TAG_128]["launches"] == b["rep_p"][TAG_128]["launches"] == 1
    assert b["rep_c"][TAG_128]["flops"] == b["rep_p"][TAG_128]["flops"] - 2.0 * rows * 256 * 1024, (b["rep_c"], b["rep_p"])
    assert not [t for t in list(b["rep_c"]) + list(b["rep_p"]) if t.endswith("_x3")]
    lc, lp = b["cached"]["logits"].cpu().numpy(), b["plain"]["logits"].cpu().numpy()
    assert lc.shape == (3, rows) and not np.array_equal(lc, lp)
    for ti, t in enumerate(oracle.ranker.TASKS):
        d = float(np.abs(lc[ti].astype(np.float64) - lp[ti]).max())
        e = float(np.abs(lc[ti].astype(np.float64) - b["truth"][t]).max())
        accuracy(f"f16_hidden_cache/rows{rows}/{t}", "f16", d / (2 * b["e_model"][ti]), cached_vs_uncached=d,
                 cached_abs_err_vs_float64=e, model_abs_err_vs_float64=b["e_model"][ti])
        assert d <= 2 * b["e_model"][ti], (t, d, b["e_model"][ti])
        assert e <= 2 * b["e_model"][ti], (t, e, b["e_model"][ti])


def test_pipeline_winners_against_f16x3(accuracy):
    """A condition on ids, not a recall threshold: every f16 winner's f16x3 CTR logit is at least the tenth f16x3 logit
    minus 2 e, e = the largest |f16 - f16x3| CTR logit of that user's candidates; and e stays under twice the model's worst
    logit error."""
    b = _big_batch()
    B, k1, top_k = b["B"], b["k1"], b["top_k"]
    l16 = b["cached"]["logits"][0].cpu().numpy().reshape(B, k1).astype(np.float64)
    l3 = b["x3"]["logits"][0].cpu().numpy().reshape(B, k1).astype(np.float64)
    cand = b["cached"]["candidate_ids"].cpu().numpy()
    ids16, ids3 = b["cached"]["ad_ids"].cpu().numpy(), b["x3"]["ad_ids"].cpu().numpy()
    e_all, same = 0.0, 0
    for u in range(B):
        e = float(np.abs(l16[u] - l3[u]).max())
        e_all = max(e_all, e)
        tenth = np.sort(l3[u])[-top_k]
        pos = {int(c): j for j, c in enumerate(cand[u])}
        for i in ids16[u]:
            assert l3[u][pos[int(i)]] >= tenth - 2 * e, (u, int(i), l3[u][pos[int(i)]], tenth, e)
        same += len(set(ids16[u].tolist()) & set(ids3[u].tolist()))
    accuracy(f"f16_pipeline/B{B}x{k1}/ctr", "f16", e_all / (2 * b["e_model"][0]), max_abs_diff_vs_f16x3=e_all,
             model_abs_err_vs_float64=b["e_model"][0], winners_shared_with_f16x3=same / (B * top_k))
    assert e_all <= 2 * b["e_model"][0], (e_all, b["e_model"][0])


def test_graph_capture_replays_the_eager_result():
    B, k1, top_k = 3, 64, 10
    rec = _rec(1024, "f16")
    graph = rec.capture(batch_size=B, top_k=top_k, stage1_k=k1)
    for seed in (41, 43):
        uc, un = (_cu(a) for a in _users(B, seed=seed))
        got = _clone(graph(uc, un))
        want = rec.recommend_device(uc, un, top_k, k1)
        for key in ("ad_ids", "scores", "logits", "candidate_ids", "candidate_scores"):
            assert torch.equal(got[key], want[key]), key
