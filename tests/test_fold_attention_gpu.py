"""GPU: the row-owner engine on the folded program (TransformerRanker.fold_first_attention: encoder layer 1's attention
block folded into the feature projection, the chain starting with LN1 alone) against float64 truth, the unfolded
program and the strict fp32-MFMA engine; the column-split kernel against the 16-row kernel on it; the candidate-side
projection cache in the folded form."""
import numpy as np
import pytest
import torch

import oracle
from amdrec import _lib, synth
from tests import cases

pytestmark = pytest.mark.gpu


def _model(cross, name="demo"):
    from amdrec.ranker import TransformerRanker
    user, ad, nnum, sd, _ = cases.ranker_case(name, cross)
    m = TransformerRanker(dict(user), dict(ad), nnum, **cases.arch(name)["rk"])
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.cuda().eval(), sd, (user, ad, nnum)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _folded(m):
    params, _ = m._pack(torch.device("cuda:0"))
    return bool(params.x3.fold_attn1)


@pytest.mark.parametrize("U", [8, 24])                  # 4000 rows: column-split kernel; 12000: 64-row workgroups
@pytest.mark.parametrize("cross", ["scaled", "randn"])
def test_folded_logits_vs_float64_truth(cross, U, accuracy):
    """The fold removes one fp32-level GEMM from every row (z is ONE rounding of W_p' f + b_p' instead of x0 rounded, then
    x0 + W_ov x0 + b_ov on the split engine): its logits must stay within the oracle tolerance, within 4x the fp32-MFMA
    engine's error against float64 (the bound every engine is held to) and, on the stable statistic - the RMS over all
    logits - not be further from float64 than the unfolded program's (5 % of slack).  The two MAXIMA are recorded; their
    ratio moves by tens of percent with the seed (tests/test_x3_gpu.py), so it is not asserted beyond the 4x bound."""
    m, sd, (user, ad, nnum) = _model(cross)
    k, N = 500, 30_000
    uc, un = synth.user_batch(user, nnum, U, seed=61)
    table = synth.ad_features(ad, N, seed=62)
    cand = np.random.default_rng(63).integers(0, N, (U, k))
    args = (np.repeat(uc, k, axis=0), table[cand.reshape(-1)], np.repeat(un, k, axis=0))
    ref = oracle.ranker.forward(sd, *args)
    truth = oracle.ranker.forward(sd, *args, dtype=np.float64)
    scale = cases.logit_scale(ref)
    err64, rms64 = {}, {}
    for label, engine, fold in (("folded", "f16x3", True), ("unfolded", "f16x3", False), ("fp32", "fp32", True)):
        m.gemm_engine, m.fold_first_attention = engine, fold
        assert _folded(m) == (label == "folded")
        got = m.score_candidates(_cu(uc), _cu(un), _cu(cand), _cu(table), check_indices=True)
        e, sq = 0.0, []
        for t in ref:
            g = got[t].cpu().numpy()
            ok, err = cases.logit_close(g, ref[t], cross, scale=scale)
            assert ok, (label, t, err)
            d = g.astype(np.float64) - truth[t]
            e = max(e, float(np.abs(d).max()))
            sq.append(d * d)
        err64[label], rms64[label] = e, float(np.sqrt(np.mean(np.concatenate(sq))))
    accuracy(f"float64_truth/fold/demo_{cross}/rows{U * k}", "f16x3 folded", err64["folded"] / max(err64["fp32"], 1e-30),
             abs_err_vs_float64=err64["folded"], unfolded_abs_err_vs_float64=err64["unfolded"],
             fp32_engine_abs_err_vs_float64=err64["fp32"], rms_err_vs_float64=rms64["folded"],
             unfolded_rms_err_vs_float64=rms64["unfolded"], batch_logit_scale=scale)
    assert err64["folded"] <= 4.0 * err64["fp32"] + 1e-7 * max(1.0, scale), err64
    assert rms64["folded"] <= 1.05 * rms64["unfolded"], (rms64, err64)


def test_folded_extreme_rows_stay_finite_and_match_float64():
    """Projected rows spanning 60 binades (all-zero, 1e-30, 1e+6 scales, one lone 5e4 element) through the folded chain:
    amdrec_ranker_x3_prefix forms z = x0 + W_ov x0 + b_ov of them and runs LN1 alone, the FFN, ... the heads."""
    m, sd, (user, ad, nnum) = _model("scaled")
    m.x3_variant = 16
    assert _folded(m)
    uc, un = synth.user_batch(user, nnum, 256, seed=43)
    ac = synth.ad_features(ad, 256, seed=44)
    feats = oracle.ranker.embed_features(sd, uc, ac, un)
    X = (feats @ sd["feature_projection.weight"].T + sd["feature_projection.bias"]
         + sd["positional_encoding"][0, 0]).astype(np.float32)
    X[0] = 0.0
    X[1] *= 1e-30
    X[2] *= 1e6
    X[3, :] = 0.0
    X[3, 17] = 5e4
    truth = oracle.ranker.chain_states(sd, X, dtype=np.float64)
    from tests.test_x3_gpu import _prefix
    Xd = _cu(X)
    for n in (1, 2):
        x, _ = _prefix(m, Xd, n)
        ref = truth[n - 1]
        assert np.isfinite(x).all() and (np.abs(x - ref) / np.abs(ref).max(axis=1, keepdims=True)).max() <= 2e-5, n
    _, logits = _prefix(m, Xd, len(truth))
    assert np.isfinite(logits).all()
    scale = cases.logit_scale(truth[-1])
    for ti, t in enumerate(oracle.ranker.TASKS):
        ok, err = cases.logit_close(logits[ti], truth[-1][t], "scaled", scale=scale)
        assert ok, (t, err)


@pytest.mark.parametrize("rows", [1, 500, 4096])
def test_column_split_kernel_is_bit_identical_on_the_folded_program(rows):
    """rowowner16c.hpp against rowowner16.hpp on the folded program: whole forwards (the folded projection GEMM, then the
    chain from LN1 alone) and every prefix of the chain (z formed from x0 by the prefix entry) must be EQUAL."""
    m, sd, (user, ad, nnum) = _model("randn")
    m.x3_variant = 16
    assert _folded(m)
    uc, un = synth.user_batch(user, nnum, rows, seed=rows + 7)
    ac = synth.ad_features(ad, rows, seed=rows + 8)
    lib = _lib.load()

    def run(cs, fn):
        m.x3_cs_max_rows = 0 if cs else -1
        _lib.check(lib.amdrec_profile_enable(1))
        out = fn()
        torch.cuda.synchronize()
        tags = list(_lib.profile_report())
        _lib.check(lib.amdrec_profile_enable(0))
        assert ("ranker_colsplit16_x3" in tags) == cs, tags
        return out

    fwd = lambda: {k: v.clone() for k, v in m(_cu(uc), _cu(ac), _cu(un)).items()}     # noqa: E731
    ref, cs = run(False, fwd), run(True, fwd)
    for t in ref:
        assert torch.isfinite(ref[t]).all() and torch.equal(ref[t], cs[t]), t
    from tests.test_x3_gpu import _prefix
    feats = oracle.ranker.embed_features(sd, uc, ac, un)
    X = _cu((feats @ sd["feature_projection.weight"].T + sd["feature_projection.bias"]
             + sd["positional_encoding"][0, 0]).astype(np.float32))
    for n in range(1, 11):
        x_ref, l_ref = run(False, lambda: _prefix(m, X, n))
        x_cs, l_cs = run(True, lambda: _prefix(m, X, n))
        if n < 10:
            assert np.array_equal(x_ref, x_cs), (n, np.abs(x_ref - x_cs).max())
        else:
            assert np.isfinite(l_ref).all() and np.array_equal(l_ref, l_cs)


def test_folded_ad_projection_cache_is_bit_identical_and_follows_the_engine():
    """The cached form (row gather of W_p'[:, ad] . emb + the user half) returns exactly the GEMM form's logits on the
    folded program; switching to the strict fp32 engine (unfolded projection) and back never serves a cache built for the
    other form - each switch rebuilds it, and each cached result equals that engine's GEMM form."""
    m, sd, (user, ad, nnum) = _model("scaled")
    U, k, N = 9, 500, 20_000
    uc, un = _cu(synth.user_batch(user, nnum, U, seed=19)[0]), _cu(synth.user_batch(user, nnum, U, seed=19)[1])
    table = _cu(synth.ad_features(ad, N, seed=20))
    cand = _cu(np.random.default_rng(21).integers(0, N, (U, k)))
    score = lambda: {t: v.clone() for t, v in m.score_candidates(uc, un, cand, table).items()}    # noqa: E731
    assert _folded(m)
    base = score()                                                       # GEMM form (no cache yet)
    cache = m.cache_ad_projection(table)
    assert m._cache_for(table) is cache
    hit = score()
    for t in base:
        assert torch.equal(base[t], hit[t]), t
    m.gemm_engine = "fp32"
    assert not _folded(m) and m._cache_for(table) is None                 # the folded cache is not served to fp32
    fp32_gemm = score()
    m.ensure_ad_cache(table)
    fp32_cache = m._cache_for(table)
    assert fp32_cache is not None and not torch.equal(fp32_cache, cache)   # rebuilt: the unfolded ad half
    fp32_hit = score()
    for t in base:
        assert torch.equal(fp32_gemm[t], fp32_hit[t]), t
        assert not torch.equal(fp32_hit[t], hit[t]), t                   # really another engine
    m.gemm_engine = "f16x3"
    assert _folded(m) and m._cache_for(table) is None                     # nor the unfolded cache to the folded program
    m.ensure_ad_cache(table)
    assert torch.equal(m._cache_for(table), cache)                        # same weights, same form: the same cache bits
    again = score()
    for t in base:
        assert torch.equal(base[t], again[t]), t
