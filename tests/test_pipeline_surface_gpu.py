"""The serving pipeline when stage 1 returns fewer candidates than asked (tests/pipeline_oracle.py has the contract): a slot
with a negative stage-1 position is not a candidate - it ranks after every real one and is reported, only where fewer than
``top_k`` real candidates exist, as ad id -1 with probability 0.0 - on every entry point, index type and ranker path.

Every case takes the GPU's own stage-1 list as given (stage 1 has its own suites) and checks, per user: the filled slots'
logits against the float64 ranker (cases.logit_close, strict rule: the weights are the benchmark's, cross weights / 16);
``ad_ids`` exactly, the -1 / 0.0 tail exactly and the real probabilities within cases.SCORE_ATOL of the oracle's selection
applied to the GPU's own logits (an fp32 sigmoid in (0, 1]: expf, one add and one division are a few ulp of at most 6e-8
each, the oracle's own rounding to float32 one more); agreement with the float64 selection up to a near-tie at the last
reported place (2 * cases.LOGIT_STRICT_RTOL, test_pipeline_gpu's allowance); the reported real ads distinct and all from
filled slots; ``candidate_ids`` in the search's ``id_map[-1]`` convention and finite logits in the unfilled slots."""
import functools

import numpy as np
import pytest
import torch

import oracle
from amdrec import synth
from tests import cases
from tests import pipeline_oracle as po

pytestmark = pytest.mark.gpu

TOP_K, K1 = 10, 500
SEED = 21


def _t(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _world():
    """Seeded models of the default architecture on cases.small_dims(), shared by every case (the modules are not changed
    by a case; the ranker's per-ad caches follow the table they are asked about)."""
    from amdrec.ranker import TransformerRanker
    from amdrec.towers import TwoTowerModel
    user, ad, nnum = cases.small_dims()
    tt_sd = synth.two_tower_state(user, ad, nnum, seed=SEED)
    rk_sd = synth.ranker_state(user, ad, nnum, seed=SEED + 1, cross_scale=cases.CROSS["scaled"])
    tt = TwoTowerModel(dict(user), dict(ad), nnum)
    tt.load_state_dict(_t(tt_sd))
    rk = TransformerRanker(dict(user), dict(ad), nnum)
    rk.load_state_dict(_t(rk_sd))
    uc, un = synth.user_batch(user, nnum, 5, seed=31)
    return dict(user=user, ad=ad, nnum=nnum, rk_sd=rk_sd, tt=tt.cuda().eval(), rk=rk.cuda().eval(), uc=uc, un=un)


@functools.lru_cache(maxsize=None)
def _table(n_ads):
    """[n_ads, 20] ad features whose row 0 - the row every clamped gather reads for an unfilled slot - is, by its float64 ctr
    logit, inside the top 10 of each of the five users over the whole table: the table's rows are searched on the CPU for
    the one whose worst rank over the users is best, and it changes places with row 0.  -> (table, that worst rank); tables
    of more than 300 rows are taken as they are (-> (table, None))."""
    w = _world()
    table = synth.ad_features(w["ad"], n_ads, seed=SEED + 2)
    if n_ads > 300:
        table.setflags(write=False)
        return table, None
    ctr = oracle.ranker.forward(w["rk_sd"], np.repeat(w["uc"], n_ads, axis=0), np.tile(table, (5, 1)),
                                np.repeat(w["un"], n_ads, axis=0), dtype=np.float64)["ctr"].reshape(5, n_ads)
    worst = (-ctr).argsort(axis=1).argsort(axis=1).max(axis=0)
    r = int(worst.argmin())
    table[[0, r]] = table[[r, 0]]
    table.setflags(write=False)
    return table, int(worst[r])


def _ids(scheme, n):
    return None if scheme == "identity" else np.arange(n) * 3 + 11          # custom: the remap path


def _rec(table, ids=None, **kind):
    from amdrec.index import FAISSIndex
    from amdrec.pipeline import AdRecommenderInference
    w = _world()
    idx = FAISSIndex(256, **kind)
    with torch.no_grad():
        emb = w["tt"].get_ad_embeddings(_dev(table))
    idx.add(emb, None if ids is None else ids.tolist())
    return AdRecommenderInference(two_tower_model=w["tt"], transformer_ranker=w["rk"], faiss_index=idx,
                                  ad_features=np.array(table))


def _clone(out):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _positions(out, id_map, fill):
    """Stage 1's positions from what the call returns: filled slots have finite candidate_scores and (unique ids) their id
    names the row; the unfilled ones carry the index type's fill score."""
    cs = out["candidate_scores"].cpu().numpy()
    cand = out["candidate_ids"].cpu().numpy()
    filled = np.isfinite(cs)
    assert (cs[~filled] == fill).all()
    inv = np.full(int(id_map.max()) + 1, -1, dtype=np.int64)
    inv[id_map] = np.arange(len(id_map))
    pos = np.where(filled, inv[cand], -1)
    assert (pos[filled] >= 0).all()
    return pos


def _check(out, pos, table, id_map, uc, un, top_k, ids_are_positions=False):
    """The contract, for every user of one call.  -> (ad_ids, scores) as numpy."""
    rk_sd = _world()["rk_sd"]
    B, k1 = pos.shape
    filled = pos >= 0
    cand = out["candidate_ids"].cpu().numpy()
    logits = out["logits"].cpu().numpy().reshape(3, B, k1)
    ids, sc = out["ad_ids"].cpu().numpy(), out["scores"].cpu().numpy()
    assert ids.shape == (B, top_k) and sc.shape == (3, B, top_k)
    # 2. today's layout: the search's id_map[-1] for an unfilled slot, a finite logit there for a finite user
    assert np.array_equal(cand, po.candidate_ids(pos, id_map, ids_are_positions))
    assert np.isfinite(logits[:, np.isfinite(un).all(axis=1)]).all()
    # the filled slots' logits against float64
    ref = po.logits64(rk_sd, uc, un, pos, table)
    for ti, t in enumerate(oracle.ranker.TASKS):
        ok, err = cases.logit_close(logits[ti][filled], ref[t][filled], "scaled")
        print(f"logits {t}: {int(filled.sum())} filled slots, max err / bound {err:.3f}")
        assert ok, (t, err)
    # 1. exactly the oracle's selection of the GPU's own logits
    e_ids, e_sc, e_slots = po.expected(pos, cand, logits, top_k)
    real = e_slots >= 0
    assert np.array_equal(ids, e_ids), (ids, e_ids)
    assert (sc[:, ~real] == 0).all()
    if real.any():
        d = float(np.abs(sc[:, real] - e_sc[:, real]).max())
        print(f"probabilities: max |d| {d:.2e}")
        assert d <= cases.SCORE_ATOL
    # and the float64 selection's, up to a near-tie at the last reported place
    r_ids, _, r_slots = po.expected(pos, cand, np.stack([ref[t] for t in oracle.ranker.TASKS]), top_k)
    for b in range(B):
        n_real = min(top_k, int(filled[b].sum()))
        got = ids[b, :n_real].tolist()
        assert (ids[b, n_real:] == -1).all() and -1 not in got
        assert len(set(got)) == n_real and set(got) <= set(cand[b][filled[b]].tolist())
        miss = set(r_ids[b, :n_real].tolist()) - set(got)
        if miss:
            kth = ref["ctr"][b, r_slots[b, n_real - 1]]
            for i in miss:
                li = ref["ctr"][b, int(np.nonzero(filled[b] & (cand[b] == i))[0][0])]
                assert abs(li - kth) <= 2 * cases.LOGIT_STRICT_RTOL * max(1.0, abs(kth)), (b, i, li, kth)
    return ids, sc


def _run(rec, table, uc, un, top_k=TOP_K, k1=K1, fill=-np.inf, exclude=None, check_indices=False, out=None):
    """One recommend_device call (or ``out``, a call's result) through the whole check.  -> (out, pos, ad_ids, scores)."""
    id_map = np.asarray(rec.faiss_index.id_map, dtype=np.int64)
    if out is None:
        x = None if exclude is None else _dev(exclude)
        out = rec.recommend_device(_dev(uc), _dev(un), top_k, k1, check_indices=check_indices, exclude_ad_ids=x)
    out = _clone(out)
    pos = _positions(out, id_map, fill)
    ids, sc = _check(out, pos, table, id_map, uc, un, top_k)
    return out, pos, ids, sc


# ---- 1. a corpus shorter than the request ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["identity", "custom"])
@pytest.mark.parametrize("n_ads", [1, 6, 10, 300])
def test_corpus_shorter_than_stage1_k(n_ads, scheme):
    """stage1_k = 500 over 1 / 6 / 10 / 300 ads, Flat with both prefilters, B = 1 and 5, identity ids and ids 3 i + 11: slots
    n_ads .. 499 are unfilled; the clamped gathers give them row 0's logits, which are inside every user's top 10 (_table),
    and the id behind them is ad n - 1's.  Before the selection was handed the positions this returned, for the first user
    of n_ads = 6 with identity ids, ad_ids [0 5 5 5 5 5 5 5 5 5] where [0 5 3 2 1 4 -1 -1 -1 -1] is due, and for n_ads = 300
    [0 299 299 ...] (ad 299 under ad 0's logit, nine times).  The reference API's entry points and TwoStageRetriever return
    the device call's lists."""
    from amdrec.pipeline import TwoStageRetriever
    w = _world()
    table, worst = _table(n_ads)
    assert worst < TOP_K                                              # row 0 is in every user's float64 top 10
    for prefilter in ("bf16", "fp32"):
        rec = _rec(table, _ids(scheme, n_ads), index_type="Flat", prefilter=prefilter)
        for B in (1, 5):
            uc, un = w["uc"][:B], w["un"][:B]
            out, pos, ids, sc = _run(rec, table, uc, un, check_indices=B == 5)
            assert ((pos >= 0).sum(axis=1) == n_ads).all()
            n_tail = max(0, TOP_K - n_ads)                           # n_ads = 6: exactly four -1 / 0.0 entries per user
            assert ((ids == -1).sum(axis=1) == n_tail).all() and ((sc == 0).sum(axis=2) == n_tail).all()
            res = rec.recommend_tensors(torch.from_numpy(uc), torch.from_numpy(un), TOP_K, K1)
            assert [r["ad_ids"] for r in res] == ids.tolist()
            assert all(r["scores"][t] == sc[ti, b].tolist() for b, r in enumerate(res)
                       for ti, t in enumerate(oracle.ranker.TASKS))
        if n_ads == 6:
            r = TwoStageRetriever(w["tt"], w["rk"], rec.faiss_index)
            got, ctr = r.retrieve_and_rank(torch.from_numpy(w["uc"][:1]), torch.from_numpy(w["un"][:1]), K1, TOP_K,
                                           ad_features_lookup=_dev(table))
            assert got == ids[0].tolist() and ctr == sc[0, 0].tolist() and got[6:] == [-1] * 4 and ctr[6:] == [0.0] * 4


# ---- 2. narrow probes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ivf", "ivfpq", "ivfpq_refine"])
def test_narrow_probes_leave_most_slots_unfilled(kind):
    """nlist = 64, nprobe = 1 over 3 000 ads: one list of ~47 ads per user fills a tenth of the 500 slots."""
    w = _world()
    table, _ = _table(3000)
    kw = {"ivf": dict(index_type="IVF"), "ivfpq": dict(index_type="IVFPQ"),
          "ivfpq_refine": dict(index_type="IVFPQ", refine="fp32")}[kind]
    rec = _rec(table, None, nlist=64, nprobe=1, **kw)
    out, pos, ids, sc = _run(rec, table, w["uc"], w["un"], fill=-np.inf if kind == "ivf" else np.inf)
    n_filled = (pos >= 0).sum(axis=1)
    print("filled slots per user:", n_filled.tolist())
    assert (n_filled < K1 // 2).all() and (n_filled > 0).any()        # most slots really are unfilled


# ---- 3. exclusion lists that empty the candidate list ------------------------------------------------------------------------
def _exclusion_case(scheme):
    """40 ads, stage1_k = 30; the three users' lists leave 0, 3 and 30 eligible ads, and the lists of the last two name ad
    n - 1's id (what an unfilled slot reads as its id) and ad row 0's (whose features it is scored with)."""
    from amdrec.pipeline import Preprocessor
    from tests.test_exclude_gpu import _users
    w = _world()
    n = 40
    table, _ = _table(n)
    ids = _ids(scheme, n)
    rec = _rec(table, ids, index_type="Flat")
    classes = {c: [f"cat_{j}" for j in range(card)] for c, card in w["user"].items()}
    rec.preprocessor = Preprocessor(classes, [f"I{i}" for i in range(1, 14)], np.zeros(13), np.ones(13))
    id_map = np.arange(n) if ids is None else ids
    rng = np.random.default_rng(8)
    inner = rng.permutation(np.arange(1, n - 1))
    lists = [id_map.tolist(),
             id_map[np.r_[n - 1, 0, inner[:35]]].tolist(),
             id_map[np.r_[inner[:8], 0, n - 1]].tolist()]
    users = _users(w["user"], 3, 5)
    return rec, table, users, lists


@pytest.mark.parametrize("scheme", ["identity", "custom"])
def test_exclusion_lists_that_empty_the_candidate_list(scheme):
    from amdrec import exclude
    rec, table, users, lists = _exclusion_case(scheme)
    uc, un = rec.preprocess_batch(users)
    uc, un = uc.cpu().numpy(), un.cpu().numpy()
    blk = exclude.pad_exclusions(lists, width=40)
    out, pos, ids, sc = _run(rec, table, uc, un, k1=30, exclude=blk)
    assert (pos >= 0).sum(axis=1).tolist() == [0, 3, 30]
    assert (ids[0] == -1).all() and (sc[:, 0] == 0).all()
    assert (ids[1, 3:] == -1).all() and (ids[2] != -1).all()
    for b in range(3):
        assert not set(ids[b].tolist()) & set(lists[b]), (b, ids[b])
    res = rec.batch_recommend(users, TOP_K, 30, exclude_ad_ids=lists)
    assert [r["ad_ids"] for r in res] == ids.tolist()
    for b, r in enumerate(res):
        assert all(len(v) == TOP_K for v in r["scores"].values())
        assert all(r["scores"][t] == sc[ti, b].tolist() for ti, t in enumerate(oracle.ranker.TASKS))
        one = rec.recommend_ads(users[b], TOP_K, 30, exclude_ad_ids=lists[b])
        assert one["ad_ids"] == ids[b].tolist() and one["scores"]["ctr"] == sc[0, b].tolist()


# ---- 4. a NaN user -------------------------------------------------------------------------------------------------------------
def test_nan_user_gets_nothing_and_disturbs_nobody():
    """One user of five has a NaN numerical feature.  The user tower keeps the NaN through its hidden layers' ReLU (as
    torch.relu does), so that user's query is NaN, the search fills none of its slots and its result is all -1 / 0.0; the
    other users' embeddings and results are those of the batch without it."""
    w = _world()
    table, _ = _table(300)
    rec = _rec(table, None, index_type="Flat")
    uc, un = w["uc"], w["un"].copy()
    un[2, 4] = np.nan
    emb = w["tt"].user_tower.encode(_dev(uc), _dev(un), check_indices=False, renormalize=True)
    good = w["tt"].user_tower.encode(_dev(uc), _dev(w["un"]), check_indices=False, renormalize=True)
    assert bool(torch.isnan(emb[2]).all()) and torch.equal(emb[[0, 1, 3, 4]], good[[0, 1, 3, 4]])
    out, pos, ids, sc = _run(rec, table, uc, un)
    assert (pos[2] == -1).all() and (ids[2] == -1).all() and (sc[:, 2] == 0).all()
    keep = [0, 1, 3, 4]
    out4, pos4, ids4, sc4 = _run(rec, table, uc[keep], un[keep])
    assert np.array_equal(ids[keep], ids4) and (ids4 != -1).all()


# ---- 5. the live corpus --------------------------------------------------------------------------------------------------------
def test_live_corpus_shrinks_below_top_k_and_grows_back():
    w = _world()
    table, _ = _table(12)
    rec = _rec(table, None, index_type="Flat")
    uc, un = w["uc"], w["un"]
    gone = [0, 2, 3, 5, 6, 8, 10, 11]                                 # ad row 0 and ad n - 1 among them
    assert rec.remove_ads(gone) == 8
    t4 = rec.ad_features.cpu().numpy()
    assert t4.shape[0] == 4 and np.array_equal(t4, table[[1, 4, 7, 9]])
    out, pos, ids, sc = _run(rec, t4, uc, un)
    assert ((ids != -1).sum(axis=1) == 4).all() and not np.isin(ids, gone).any()
    assert all(sorted(r[:4].tolist()) == [1, 4, 7, 9] for r in ids)
    new = synth.ad_features(w["ad"], 8, seed=SEED + 9)
    with torch.no_grad():
        emb = w["tt"].get_ad_embeddings(_dev(new))
    rec.add_ads(emb, new, list(range(100, 108)))
    t12 = rec.ad_features.cpu().numpy()
    assert t12.shape[0] == 12 == rec.faiss_index.index.ntotal and np.array_equal(t12[4:], new)
    out, pos, ids, sc = _run(rec, t12, uc, un)
    assert ((pos >= 0).sum(axis=1) == 12).all() and (ids != -1).all() and not np.isin(ids, gone).any()


# ---- 6. a captured graph -------------------------------------------------------------------------------------------------------
KEYS = ("ad_ids", "scores", "candidate_ids", "candidate_scores", "logits")


@pytest.mark.parametrize("B", [1, 5])
def test_captured_graph_replays_short_lists(B):
    w = _world()
    table, _ = _table(300)
    rec = _rec(table, None, index_type="Flat")
    uc, un = w["uc"][:B], w["un"][:B]
    eager, pos, ids, sc = _run(rec, table, uc, un)
    g = rec.capture(B, TOP_K, K1)
    out = g(_dev(uc), _dev(un))
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.equal(out[key], eager[key]), key
    _run(rec, table, uc, un, out=out)


def test_captured_graph_replays_emptying_exclusions():
    from amdrec import exclude
    rec, table, users, lists = _exclusion_case("identity")
    uc, un = rec.preprocess_batch(users)
    x = _dev(exclude.pad_exclusions(lists, width=40))
    eager = _clone(rec.recommend_device(uc, un, TOP_K, 30, exclude_ad_ids=x))
    g = rec.capture(3, TOP_K, 30, max_exclude=40)
    out = g(uc, un, exclude=x)
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.equal(out[key], eager[key]), key
    ids = out["ad_ids"].cpu().numpy()
    assert (ids[0] == -1).all() and (ids[1, 3:] == -1).all() and (ids[1, :3] != -1).all() and (ids[2] != -1).all()
    for b in range(3):
        assert not set(ids[b].tolist()) & set(lists[b])
    _run(rec, table, uc.cpu().numpy(), un.cpu().numpy(), k1=30, out=out)


# ---- 7. positions as ids (the sharded path) ------------------------------------------------------------------------------------
def test_stage2_with_positions_as_ids():
    """HipEngine.rank's call: ``_stage2(..., ids_are_positions=True)`` on hand-made positions with -1 in the first slot, in
    scattered slots, in a whole row and in all but three slots."""
    w = _world()
    n, k1 = 300, 50
    table, _ = _table(n)
    rec = _rec(table, None, index_type="Flat")
    rng = np.random.default_rng(3)
    pos = np.stack([rng.permutation(n)[:k1] for _ in range(5)]).astype(np.int64)
    pos[0, 0] = -1
    pos[1, rng.random(k1) < 0.35] = -1
    pos[1, [1, k1 - 1]] = -1
    pos[2, :] = -1
    pos[4, :] = -1
    pos[4, [7, 20, 33]] = [0, n - 1, 17]
    uc, un = w["uc"], w["un"]
    out = _clone(rec._stage2(_dev(uc), _dev(un), _dev(pos), TOP_K, False, ids_are_positions=True))
    ids, sc = _check(out, pos, table, np.arange(n), uc, un, TOP_K, ids_are_positions=True)
    assert (ids[2] == -1).all() and sorted(ids[4, :3].tolist()) == [0, 17, n - 1] and (ids[4, 3:] == -1).all()
    assert (ids[[0, 1, 3]] != -1).all()


# ---- 8. row independence on every ranker path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [100, 900, 3277])
@pytest.mark.parametrize("engine", ["f16x3", "fp32", "bf16x6"])
def test_negative_rows_leave_every_other_row_alone(engine, k):
    """score_candidates over a 2 000-ad table, 5 users x k = 500 / 4 500 / 16 385 rows (f16x3: the column-split, 64-row and
    128-row kernels, the last with the hidden cache when cache_first_ffn is on; the other engines: the small fp32 shapes and,
    at 16 385 rows, the wide fp32 / x6 tiles), with and without the ad-projection cache: a tenth of the slots negative
    against the same slots holding row 7 - every other logit is bit-identical, and every logit is finite.  With
    check_indices a negative row passes and a row one past the table raises."""
    from amdrec.ranker import TransformerRanker
    w = _world()
    n = 2000
    table = _dev(_table(n)[0])
    rk = TransformerRanker(dict(w["user"]), dict(w["ad"]), w["nnum"])
    rk.load_state_dict(_t(w["rk_sd"]))
    rk = rk.cuda().eval()
    rk.gemm_engine = engine
    uc, un = _dev(w["uc"]), _dev(w["un"])
    rng = np.random.default_rng(k)
    cand = rng.integers(0, n, size=(5, k))
    hole = rng.random((5, k)) < 0.1
    hole[0, 0] = hole[4, k - 1] = True
    neg, seven = _dev(np.where(hole, -1, cand)), _dev(np.where(hole, 7, cand))
    keep = _dev(~hole.reshape(-1))
    for ffn_cache in (True, False):
        rk.cache_first_ffn = ffn_cache
        for cached in (True, False):
            if cached:
                rk.ensure_ad_cache(table)
                assert rk._cache_for(table) is not None
            else:
                rk.cache_ad_projection(None)
            _, a = rk.score_candidates(uc, un, neg, table, check_indices=True, raw=True)      # (a negative row passes)
            _, b = rk.score_candidates(uc, un, seven, table, raw=True)
            _, c = rk.score_candidates(uc, un, neg, table, raw=True)
            assert torch.equal(a, c)
            assert torch.equal(a[:, keep], b[:, keep]), (ffn_cache, cached)
            assert bool(torch.isfinite(a).all())
            if engine != "bf16x6" and k == 100 and ffn_cache:
                past = seven.clone()
                past[3, 5] = n                                        # (clamped to the last row by every gather)
                with pytest.raises(IndexError):
                    rk.score_candidates(uc, un, past, table, check_indices=True)
                rk.score_candidates(uc, un, past, table)              # without the flag nothing changes: no error
