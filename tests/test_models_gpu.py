"""Parity of the HIP tower / ranker forward (through the C ABI, via the nn.Module drop-ins)
against the golden vectors captured from the reference modules and against the CPU oracle."""
import numpy as np
import pytest
import torch

import oracle
from amdrec import synth
from tests import cases
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


def _t(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _two_tower(name):
    from amdrec.towers import TwoTowerModel
    user, ad, nnum, sd, batches = cases.two_tower_case(name)
    m = TwoTowerModel(dict(user), dict(ad), nnum, **cases.arch(name)["tt"])
    m.load_state_dict(_t(sd))
    return m.cuda().eval(), sd, (user, ad, nnum), batches


def _ranker(name, cross):
    from amdrec.ranker import TransformerRanker
    user, ad, nnum, sd, batches = cases.ranker_case(name, cross)
    m = TransformerRanker(dict(user), dict(ad), nnum, **cases.arch(name)["rk"])
    m.load_state_dict(_t(sd))
    return m.cuda().eval(), sd, (user, ad, nnum), batches


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_two_tower_matches_reference_golden(name):
    m, sd, _, batches = _two_tower(name)
    g = load_golden(f"two_tower_{name}.npz")
    for B in batches:
        uc, un, ac = _cu(g[f"B{B}_user_cat"]), _cu(g[f"B{B}_user_num"]), _cu(g[f"B{B}_ad_cat"])
        with torch.no_grad():
            ue, ae = m(uc, un, ac)
            ps = m.predict_scores(uc, un, ac)
        assert ue.dtype == torch.float32 and ue.shape == (B, cases.arch(name)["tt"].get("output_dim", 256)) and ue.is_cuda
        assert np.abs(ue.cpu().numpy() - g[f"B{B}_user_emb"]).max() <= cases.EMB_ATOL
        assert np.abs(ae.cpu().numpy() - g[f"B{B}_ad_emb"]).max() <= cases.EMB_ATOL
        assert np.abs(ps.cpu().numpy() - g[f"B{B}_scores"]).max() <= cases.EMB_ATOL
        assert np.abs(m.get_user_embeddings(uc, un).cpu().numpy() - g[f"B{B}_user_emb"]).max() <= cases.EMB_ATOL
        assert np.abs(m.get_ad_embeddings(ac).cpu().numpy() - g[f"B{B}_ad_emb"]).max() <= cases.EMB_ATOL


def test_towers_large_batch_vs_oracle_crosses_row_passes():
    m, sd, (user, ad, nnum), _ = _two_tower("ragged")
    B = 300_001                                  # > one 262144-row pass, ragged tail
    uc, un = synth.user_batch(user, nnum, B, seed=5)
    ac = synth.ad_features(ad, B, seed=6)
    ue = m.get_user_embeddings(_cu(uc.astype(np.int32)), _cu(un)).cpu().numpy()   # any int dtype (.long())
    ae = m.get_ad_embeddings(_cu(ac)).cpu().numpy()
    assert np.abs(ue - oracle.towers.user_tower(sd, uc, un)).max() <= cases.EMB_ATOL
    assert np.abs(ae - oracle.towers.ad_tower(sd, ac)).max() <= cases.EMB_ATOL
    assert np.abs(np.linalg.norm(ae, axis=1) - 1).max() <= 1e-5


@pytest.mark.parametrize("rows", [300, 511, 701, 2000])
def test_demo_towers_mid_batches_vs_oracle(rows):
    """The reference tower shapes between the golden batches (<= 64 rows) and the large-batch test: the GEMV kernel with 2 and 4
    rows per workgroup (257 .. 1024 rows, ragged tails) and the pipelined 16-row MFMA kernel (.. 4096), user tower
    (K0 = 128) and ad tower (K0 = 384)."""
    m, sd, (user, ad, nnum), _ = _two_tower("demo")
    uc, un = synth.user_batch(user, nnum, rows, seed=rows)
    ac = synth.ad_features(ad, rows, seed=rows + 1)
    ue = m.get_user_embeddings(_cu(uc), _cu(un)).cpu().numpy()
    ae = m.get_ad_embeddings(_cu(ac)).cpu().numpy()
    assert np.abs(ue - oracle.towers.user_tower(sd, uc, un)).max() <= cases.EMB_ATOL
    assert np.abs(ae - oracle.towers.ad_tower(sd, ac)).max() <= cases.EMB_ATOL


@pytest.mark.parametrize("name", ["demo", "ragged"])
@pytest.mark.parametrize("rows", [1, 2, 7, 301, 512, 701, 5000])
def test_tower_renormalize_equals_a_separate_l2_normalize_launch(name, rows):
    """``encode(..., renormalize=True)`` - the serving path's tower launch that also applies the search's query
    normalisation (faiss_retrieval.py:147) - against ``encode()`` followed by ``amdrec_l2_normalize``: the same bits, on the
    GEMV kernel (<= 1024 rows: 1, 2 or 4 rows per workgroup), the 16-row kernels (<= 4096) and the tiled-GEMM path (beyond)."""
    from amdrec import _lib
    m, sd, (user, ad, nnum), _ = _two_tower(name)
    uc, un = synth.user_batch(user, nnum, rows, seed=rows)
    uc, un = _cu(uc), _cu(un)
    plain = m.user_tower.encode(uc, un)
    fused = m.user_tower.encode(uc, un, renormalize=True)
    ref = torch.empty_like(plain)
    _lib.check(_lib.load().amdrec_l2_normalize(_lib.ptr(plain), plain.stride(0), _lib.ptr(ref), ref.stride(0), rows,
                                               plain.shape[1], _lib.stream_ptr(plain.device)))
    torch.cuda.synchronize()
    assert torch.equal(fused, ref)
    assert torch.equal(m.user_tower.encode(uc, un), plain)           # the flag does not stick to the packed parameters
    assert (fused.norm(dim=1) - 1).abs().max() < 1e-6


@pytest.mark.parametrize("name", list(cases.CASES))
@pytest.mark.parametrize("engine", ["f16x3", "fp32", "bf16x6"])
@pytest.mark.parametrize("cross", list(cases.CROSS))
def test_ranker_matches_reference_golden(name, cross, engine, accuracy):
    """The reference's own outputs (tests/golden, generated from the imported transformer_ranker.py) against EVERY
    engine: the default row-owner kernel (f16x3 takes every batch since x3_min_rows = 1), the strict fp32-MFMA engine
    (it had lost its golden coverage when the default engine took the small batches) and bf16x6,
    whose passes of <= 8192 rows are fp32-MFMA small shapes."""
    m, sd, _, batches = _ranker(name, cross)
    m.gemm_engine = engine
    g = load_golden(f"ranker_{name}_{cross}.npz")
    # the row-owner engine is written for the reference's DEFAULT architecture (d_model 256, heads 256 -> 64); any other -
    # the tutorial's d_model 128 / 4 heads / 2 layers / d_ff 512 - takes the generic tile GEMMs, and says so (VERDICT r3
    # item 3: the fallback must be visible, and it must have a golden).  Each case states its reason in tests/cases.py.
    x3 = engine == "f16x3" and cases.x3_reason(name) is None
    assert m.x3_fallback_reason() == cases.x3_reason(name)
    for B in batches:
        assert m.gemm_engine_for(B) == ("f16x3" if x3 else "fp32")
        with torch.no_grad():
            pred = m(_cu(g[f"B{B}_user_cat"]), _cu(g[f"B{B}_ad_cat"]), _cu(g[f"B{B}_user_num"]))
        assert list(pred) == ["ctr", "engagement", "revenue"]
        scale = cases.logit_scale({t: g[f"B{B}_{t}"] for t in pred})
        for t in pred:
            assert pred[t].shape == (B,) and pred[t].dtype == torch.float32
            ok, err = cases.logit_close(pred[t].cpu().numpy(), g[f"B{B}_{t}"], cross, scale=scale)
            accuracy(f"golden/{name}_{cross}/B{B}/{t}", engine if engine != "bf16x6" else "bf16x6(small=fp32)", err)
            assert ok, (name, cross, engine, B, t, err)


@pytest.mark.parametrize("cross", ["scaled", "randn"])
def test_ranker_large_batch_vs_oracle(cross, accuracy):
    m, sd, (user, ad, nnum), _ = _ranker("demo", cross)
    B = 270_003                                  # crosses the 262144-row pass, ragged tail
    uc, un = synth.user_batch(user, nnum, B, seed=7)
    ac = synth.ad_features(ad, B, seed=8)
    pred = m(_cu(uc), _cu(ac), _cu(un))
    # oracle on both ends of the batch (incl. the rows around the pass boundary)
    sel = np.r_[0:20_000, 262_144 - 5_000:B]
    ref = oracle.ranker.forward(sd, uc[sel], ac[sel], un[sel])
    scale = cases.logit_scale(ref)
    for t in ref:
        ok, err = cases.logit_close(pred[t].cpu().numpy()[sel], ref[t], cross, scale=scale)
        accuracy(f"oracle/demo_{cross}/B{B}/{t}", m.gemm_engine_for(B), err)
        assert ok, (cross, t, err)


def test_ranker_unfused_attention_matches_too():
    """fuse_attention=False runs W_v and W_o as two GEMMs in the reference's order."""
    m, sd, _, batches = _ranker("demo", "scaled")
    m.fuse_attention = False
    g = load_golden("ranker_demo_scaled.npz")
    B = 64
    pred = m(_cu(g[f"B{B}_user_cat"]), _cu(g[f"B{B}_ad_cat"]), _cu(g[f"B{B}_user_num"]))
    scale = cases.logit_scale({t: g[f"B{B}_{t}"] for t in pred})
    for t in pred:
        ok, err = cases.logit_close(pred[t].cpu().numpy(), g[f"B{B}_{t}"], "scaled", scale=scale)
        assert ok, (t, err)


@pytest.mark.parametrize("name,U,k", [("ragged", 7, 500), ("demo", 1, 500), ("demo", 64, 100), ("demo", 65, 100)])
def test_ranker_score_candidates_broadcast_and_gather(name, U, k):
    """The hoisted form: user half of the projection once per user (<= 64 users: csrc/layers.hip user_proj_small_kernel,
    beyond: the tile GEMM), candidate half gathered from the resident ad table."""
    m, sd, (user, ad, nnum), _ = _ranker(name, "scaled")
    N = 5000
    uc, un = synth.user_batch(user, nnum, U, seed=9)
    table = synth.ad_features(ad, N, seed=10)
    rng = np.random.default_rng(11)
    cand = rng.integers(0, N, (U, k))
    pred = m.score_candidates(_cu(uc), _cu(un), _cu(cand), _cu(table), check_indices=True)
    ref = oracle.ranker.forward(sd, np.repeat(uc, k, axis=0), table[cand.reshape(-1)], np.repeat(un, k, axis=0))
    scale = cases.logit_scale(ref)
    for t in ref:
        ok, err = cases.logit_close(pred[t].cpu().numpy(), ref[t], "scaled", scale=scale)
        assert ok, (t, err)


@pytest.mark.parametrize("name,cross", [("demo", "scaled"), ("demo", "randn"), ("ragged", "scaled")])
def test_ranker_large_pass_engines_vs_float64_truth(name, cross, accuracy):
    """Passes of more than 8192 rows run a split 16-bit-MFMA GEMM engine (the default) instead of the fp32 MFMA.
    Every engine is held to the same oracle tolerance, and - the sharper statement - its error against a FLOAT64
    evaluation of the network is at most 4x the fp32-MFMA engine's own error against the same truth (VERDICT r1
    item 2: an error-compensated engine must sit at the fp32 rounding level, not merely inside the blanket bound)."""
    m, sd, (user, ad, nnum), _ = _ranker(name, cross)
    U, k, N = 24, 500, 30_000                                            # 12000 rows
    uc, un = synth.user_batch(user, nnum, U, seed=29)
    table = synth.ad_features(ad, N, seed=30)
    cand = np.random.default_rng(31).integers(0, N, (U, k))
    args = (np.repeat(uc, k, axis=0), table[cand.reshape(-1)], np.repeat(un, k, axis=0))
    ref = oracle.ranker.forward(sd, *args)
    truth = oracle.ranker.forward(sd, *args, dtype=np.float64)
    scale = cases.logit_scale(ref)
    got, err64 = {}, {}
    for eng in m.ENGINES:
        m.gemm_engine = eng
        assert m.gemm_engine_for(U * k) == eng
        got[eng] = m.score_candidates(_cu(uc), _cu(un), _cu(cand), _cu(table), check_indices=True)
        e64 = 0.0
        for t in ref:
            ok, err = cases.logit_close(got[eng][t].cpu().numpy(), ref[t], cross, scale=scale)
            assert ok, (eng, t, err)
            e64 = max(e64, float(np.abs(got[eng][t].cpu().numpy().astype(np.float64) - truth[t]).max()))
            accuracy(f"oracle/{name}_{cross}/rows{U * k}/{t}", eng, err)
        err64[eng] = e64
    oracle64 = max(float(np.abs(ref[t].astype(np.float64) - truth[t]).max()) for t in ref)
    for eng in m.ENGINES:
        accuracy(f"float64_truth/{name}_{cross}/rows{U * k}", eng, err64[eng] / max(err64["fp32"], 1e-30),
                 abs_err_vs_float64=err64[eng], fp32_engine_abs_err_vs_float64=err64["fp32"],
                 numpy_oracle_abs_err_vs_float64=oracle64, batch_logit_scale=scale)
        assert err64[eng] <= 4.0 * err64["fp32"] + 1e-7 * max(1.0, scale), (eng, err64)
        if eng != "fp32":
            assert not torch.equal(got[eng]["ctr"], got["fp32"]["ctr"])  # it really is a different code path


def test_ranker_ad_projection_cache_is_bit_identical_and_invalidates():
    """cache_ad_projection: the cached (row-gather) form of the candidate half of the projection returns exactly the
    logits of the GEMM form; a weight update or another table drops it (the GEMM form runs again)."""
    m, sd, (user, ad, nnum), _ = _ranker("demo", "scaled")
    U, k, N = 9, 500, 20_000
    uc, un = synth.user_batch(user, nnum, U, seed=19)
    table = _cu(synth.ad_features(ad, N, seed=20))
    cand = _cu(np.random.default_rng(21).integers(0, N, (U, k)))
    base = m.score_candidates(_cu(uc), _cu(un), cand, table)
    cache = m.cache_ad_projection(table)
    assert cache.shape == (N, 256) and m._cache_for(table) is cache
    hit = m.score_candidates(_cu(uc), _cu(un), cand, table)
    for t in base:
        assert torch.equal(base[t], hit[t]), t
    other = table.clone()
    assert m._cache_for(other) is None                                   # not the table it was built from
    with torch.no_grad():
        m.feature_projection.weight.mul_(1.5)                            # weight update -> repack -> cache dropped
    upd = m.score_candidates(_cu(uc), _cu(un), cand, table)
    assert m._cache_for(table) is None and not torch.equal(upd["ctr"], base["ctr"])
    m.ensure_ad_cache(table)
    again = m.score_candidates(_cu(uc), _cu(un), cand, table)
    for t in upd:
        assert torch.equal(upd[t], again[t]), t


def test_bad_index_raises_like_torch_and_no_cpu_fallback():
    m, sd, (user, ad, nnum), _ = _two_tower("demo")
    uc, un = synth.user_batch(user, nnum, 4, seed=1)
    uc[2, 1] = 100                                # card is 100
    with pytest.raises(IndexError):
        m.get_user_embeddings(_cu(uc), _cu(un))
    uc[2, 1] = -1
    with pytest.raises(IndexError):
        m.get_user_embeddings(_cu(uc), _cu(un))
    r, rsd, (user, ad, nnum), _ = _ranker("demo", "scaled")
    ucr, unr = synth.user_batch(user, nnum, 4, seed=1)
    acr = synth.ad_features(ad, 4, seed=2)
    acr[3, 19] = 200
    with pytest.raises(IndexError):
        r(_cu(ucr), _cu(acr), _cu(unr))
    r.train()
    with pytest.raises(NotImplementedError):                   # score_candidates is the eval-mode HIP pipeline entry only
        r.score_candidates(_cu(ucr[:1]), _cu(unr[:1]), _cu(np.zeros((1, 4), np.int64)), _cu(acr))
    from amdrec import _lib
    with pytest.raises(_lib.AmdrecError):
        m.eval().get_ad_embeddings(torch.zeros((2, 20), dtype=torch.int64))   # CPU tensor: no fallback


def test_checkpoint_dict_and_weight_update_invalidate_packing():
    m, sd, (user, ad, nnum), _ = _two_tower("demo")
    ac = synth.ad_features(ad, 5, seed=4)
    a0 = m.get_ad_embeddings(_cu(ac)).cpu().numpy()
    sd2 = synth.two_tower_state(user, ad, nnum, seed=77)
    ckpt = {"epoch": 3, "model_state_dict": _t(sd2)}            # inference.py:99-106 accepts both forms
    m.load_state_dict(ckpt["model_state_dict"])
    a1 = m.get_ad_embeddings(_cu(ac)).cpu().numpy()
    assert np.abs(a1 - oracle.towers.ad_tower(sd2, ac)).max() <= cases.EMB_ATOL
    assert np.abs(a1 - a0).max() > 1e-3


@pytest.mark.parametrize("rows", [300, 2000, 9001])
def test_tutorial_architecture_batches_vs_oracle(rows, accuracy):
    """the reference's second usage example (tutorial.ipynb cells 10, 19: towers [256, 128] -> 128,
    ranker embedding 16 / d_model 128 / 4 heads / 2 layers / d_ff 512) beyond the golden batch sizes, on every generic path
    those shapes take: tower GEMV / 16-row / tiled kernels are instantiated for the default shapes only, the ranker runs the
    fp32-MFMA small shapes up to 8192 rows and the bf16x6 tiles beyond.  Against the oracle (pinned to the reference's own
    outputs for this architecture by tests/test_oracle_golden.py)."""
    import warnings
    m, sd, (user, ad, nnum), _ = _two_tower("tutorial")
    uc, un = synth.user_batch(user, nnum, rows, seed=rows)
    ac = synth.ad_features(ad, rows, seed=rows + 1)
    ue = m.get_user_embeddings(_cu(uc), _cu(un)).cpu().numpy()
    ae = m.get_ad_embeddings(_cu(ac)).cpu().numpy()
    assert ue.shape == (rows, 128)
    assert np.abs(ue - oracle.towers.user_tower(sd, uc, un)).max() <= cases.EMB_ATOL
    assert np.abs(ae - oracle.towers.ad_tower(sd, ac)).max() <= cases.EMB_ATOL
    for cross in ("scaled", "randn"):
        r, rsd, _, _ = _ranker("tutorial", cross)
        assert r.gemm_engine == "f16x3" and r.gemm_engine_for(rows) == ("bf16x6" if rows > r.SMALL_ROWS else "fp32")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            pred = r(_cu(uc), _cu(ac), _cu(un))
        assert any(f"not available for these weights ({cases.x3_reason('tutorial')})" in str(x.message) for x in w)   # not silent
        ref = oracle.ranker.forward(rsd, uc, ac, un)
        scale = cases.logit_scale(ref)
        for t in ref:
            ok, err = cases.logit_close(pred[t].cpu().numpy(), ref[t], cross, scale=scale)
            accuracy(f"tutorial_{cross}/rows{rows}/{t}", r.gemm_engine_for(rows), err)
            assert ok, (cross, rows, t, err)
