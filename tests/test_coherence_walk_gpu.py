"""Long-lived objects under seeded call sequences (tests/coherence.py has the generator, the corpus model and the twins).

Index walk: one long-lived FAISSIndex per kind goes through adds (1, 37, 1500 and once 12 000 rows; custom, repeating and
string ids; with and without tags, groups, bids), removals (subsets with absent ids and duplicates, once everything, once with set_tags in the same step),
set_tags / set_groups / set_bids, nprobe changes and a save / load in mid-life.  After EVERY step the fixed probe set - (nq, k)
in {(1, 10), (33, 500), (512, 100), (3, 2000)}, each plain, with an exclusion block, with masks, with max_per_group = 2 and
with all three - runs on it and on a fresh index given the corpus model's rows in one add: ids, positions and scores are
torch.equal and id_map is equal.  At the end a Flat walk is held to the float64 flat oracle and the IVF walk to the IVF one.

Pipeline walk: an AdRecommenderInference over a Flat and over an IVF index of 3000 ads goes through remove_ads, add_ads,
in-place weight updates, load_state_dict, heads-mode toggles, set_bids, set_groups and graph captures; after every step
recommend_device at B in {1, 6, 36} (plain, with exclusions, by eCPM under a cap) and at B = 96 (19 200 candidate rows: the
pass that reads the hidden cache) equals a fresh pipeline built from the state dicts and the corpus model, in every output
tensor; every captured graph keeps returning what the twin of its capture step returned.

Every input is valid: ids, feature rows and candidate rows stay inside their tables; nothing here provokes a fault."""
import numpy as np
import pytest
import torch

import oracle
from amdrec import synth
from tests import cases
from tests import coherence as co
from tests import flat_oracle as fo
from tests import ivf_oracle as io
from tests import pipeline_oracle as po
from tests.test_exclude_gpu import KINDS
from tests.test_ivfpq_gpu import _clustered

pytestmark = pytest.mark.gpu

D = co.D
_WALKS = {(seed, scheme): co.walk(seed, co.INDEX_RULES, n, scheme) for seed, scheme, n in co.INDEX_WALKS}
_POOL_ROWS = max(co.pool_rows(s) for s in _WALKS.values())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def pool():
    """(the row pool every walk draws its adds from - the clustered generator of test_live_corpus_gpu -, 512 queries)"""
    return _clustered(_POOL_ROWS, D, 40, 71).astype(np.float32), _clustered(512, D, 40, 72).astype(np.float32)


# ---- the index walk ----------------------------------------------------------------------------------------------------------
def _attrs(args):
    tags, groups, bids = co.row_attrs(args["vseed"], args["m"])[:3]
    return dict(tags=tags if args["tags"] else None, groups=groups if args["groups"] else None,
                bids=bids if args["bids"] else None)


def _apply_index(rule, args, live, model, xb, kinds, kind, tmp_path, step):
    from amdrec.index import FAISSIndex
    if rule == "add":
        rows, kw = xb[args["start"]:args["start"] + args["m"]], _attrs(args)
        live.add(rows, list(args["ids"]), **kw)
        model.add(rows, args["ids"], **kw)
    elif rule in ("remove", "remove_all", "remove_set_tags"):
        removed = live.remove_ids(list(args["ids"]))
        assert removed == model.remove(args["ids"]) == args["removed"]
        if rule == "remove_set_tags":                            # at once: no search has run on the compacted index yet
            vals = co.row_attrs(args["vseed"], model.n)[0]
            live.set_tags(vals)
            model.set_tags(vals)
    elif rule in ("set_tags", "set_groups", "set_bids"):
        vals = co.row_attrs(args["vseed"], model.n)[("set_tags", "set_groups", "set_bids").index(rule)]
        getattr(live, rule)(vals)
        getattr(model, rule)(vals)
    elif rule == "nprobe":
        live.nprobe = model.nprobe = args["value"]
    elif rule == "reload":
        path = str(tmp_path / f"mid_life_{step}.bin")
        live.save(path)
        live = FAISSIndex(D, **kinds[kind])
        live.load(path)
    else:
        raise ValueError(rule)
    return live


def _variant_kw(variant, nq, blk):
    kw = {}
    if variant in ("exclude", "all"):
        kw["exclude"] = blk
    if variant in ("masks", "all"):
        ma, my = co.query_masks(nq)
        kw["require_all"], kw["require_any"] = _dev(ma), _dev(my)
    if variant in ("cap", "all"):
        kw["max_per_group"] = 2
    return kw


def _exclusion_block(ids_plain):
    """int64 [nq, E] from each query's own plain result (so that entries hit), with padding and ids that no row has."""
    nq, k = ids_plain.shape
    blk = torch.full((nq, co.EXCLUDE_WIDTH), -1, dtype=torch.int64, device=ids_plain.device)
    w = min(k, co.EXCLUDE_WIDTH)
    blk[:, :w] = ids_plain[:, :w]
    blk[:, 3] = -1
    blk[:, 4] = 10**12 + 7
    blk[:, 5] = blk[:, 0]                                    # a duplicate
    return blk


def _probe_ints(live, twin, qn):
    for nq, k in co.PROBES:
        q = qn[:nq]
        blk = _exclusion_block(live.search_device(q, k, normalize=False)[0])
        for variant in co.VARIANTS:
            kw = _variant_kw(variant, nq, blk)
            for positions in (False, True):
                a = live.search_device(q, k, normalize=False, return_positions=positions, **kw)
                b = twin.search_device(q, k, normalize=False, return_positions=positions, **kw)
                assert torch.equal(a[0], b[0]), (nq, k, variant, "positions" if positions else "ids")
                assert torch.equal(a[1], b[1]), (nq, k, variant, "scores")


def _probe_strings(live, twin, qn, xq):
    """String ids live on the host: the ids come from the numpy entry point (whose exclusion lists go through the host id
    map), the positions and scores from the device one."""
    for nq, k in co.PROBES:
        q = qn[:nq]
        plain, _ = live.search(xq[:nq], k)
        lists = [list(plain[i][:min(k, co.EXCLUDE_WIDTH) - 2]) + ["no-such-ad", plain[i][0]] for i in range(nq)]
        if live.index.ntotal == 0:
            lists = None                                     # (no id to name: the result rows hold positions)
        for variant in co.VARIANTS:
            kw = _variant_kw(variant, nq, None)
            kw.pop("exclude", None)
            a = live.search_device(q, k, normalize=False, return_positions=True, **kw)
            b = twin.search_device(q, k, normalize=False, return_positions=True, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (nq, k, variant, "positions")
            hk = {n: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for n, v in kw.items()}
            if variant in ("exclude", "all"):
                hk["exclude"] = lists
            ia, da = live.search(xq[:nq], k, **hk)
            ib, db = twin.search(xq[:nq], k, **hk)
            assert np.array_equal(ia, ib) and np.array_equal(da, db), (nq, k, variant, "ids")
            if lists is not None and variant == "exclude":
                for i in (0, nq - 1):
                    assert not set(ia[i][np.isfinite(da[i])].tolist()) & set(lists[i])


def _check_flat_oracle(live, qn):
    n, k = live.index.ntotal, 500
    rows = live._xb[:n].cpu().numpy()
    q = qn[:33].cpu().numpy()
    rD, rI = fo.reference(rows, q, k)
    pos, Dg = live.search_device(qn[:33], k, normalize=False, return_positions=True)
    q64 = q.astype(np.float64)
    oracle.search.check_topk(rD, rI, Dg.cpu().numpy(), pos.cpu().numpy(), tau=fo.topk_tau(),
                             score_tol=fo.score_tol(D, 1.0, "mixed" if live._mixed else "fp32"),
                             scores_of=lambda qi, which: (rows[np.asarray(which)].astype(np.float64) @ q64[qi]).astype(np.float32))


def _check_ivf_oracle(live, qn):
    n, k = live.index.ntotal, 500
    xbn, assign = live._xb[:n].cpu().numpy(), live._ivf.assign.cpu().numpy()
    q = qn[:33].cpu().numpy()
    nprobe = min(max(1, live.nprobe), live.nlist)
    probes = live._ivf.coarse_probes(qn[:33], nprobe).cpu().numpy()
    tol = io.score_tol(D, io.max_norm(q), io.max_norm(xbn))
    rD, rI = io.ivf_search_nonfinite(xbn, assign, live.nlist, q, k, probes)
    pos, Dg = live.search_device(qn[:33], k, normalize=False, return_positions=True)
    pos, Dg = pos.cpu().numpy(), Dg.cpu().numpy()
    assert np.array_equal(pos >= 0, np.isfinite(Dg))
    x64, q64 = xbn.astype(np.float64), q.astype(np.float64)
    oracle.search.check_topk(rD, rI, Dg, pos, tau=2 * tol, score_tol=tol,
                             scores_of=lambda qi, ids: (x64[ids] @ q64[qi]).astype(np.float32))


@pytest.mark.parametrize("seed,scheme,n_steps", co.INDEX_WALKS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_index_walk(kind, seed, scheme, n_steps, pool, tmp_path):
    from amdrec.index import FAISSIndex
    xb, xq = pool
    kinds = co.index_kinds()
    steps = _WALKS[(seed, scheme)]
    live = FAISSIndex(D, **kinds[kind])
    live.train(xb[:co.N0])
    trained = str(tmp_path / "trained_empty.bin")
    live.save(trained)                                       # the trained state every twin loads: no retraining per step
    model = co.CorpusModel(D)
    live = _apply_index("add", co.initial_step(scheme), live, model, xb, kinds, kind, tmp_path, -1)
    qn = live._normalize_(_dev(xq))
    strings = scheme == "strings"
    for step, (rule, args) in enumerate(steps):
        live = _apply_index(rule, args, live, model, xb, kinds, kind, tmp_path, step)
        assert live.index.ntotal == model.n == args["n_after"], (step, rule)
        twin = co.fresh_index(kind, model, trained, kinds=kinds)
        assert live.id_map == twin.id_map == model.ids, (step, rule)
        try:
            if strings:
                _probe_strings(live, twin, qn, xq)
            else:
                _probe_ints(live, twin, qn)
        except AssertionError as e:
            raise AssertionError(f"{kind}, seed {seed}: after step {step} of {[r for r, _ in steps[:step + 1]]}: {e}") from e
    assert model.n > 500
    if live.index_type == "Flat":
        _check_flat_oracle(live, qn)
    elif kind == "ivf":
        _check_ivf_oracle(live, qn)


# ---- the pipeline walk -------------------------------------------------------------------------------------------------------
RANKER_ARCH = dict(embedding_dim=8, d_model=256, num_heads=8, num_layers=1, d_ff=128)
OUT_KEYS = ("ad_ids", "scores", "candidate_ids", "candidate_scores", "logits")
BATCHES, BIG_BATCH, TOP_K, STAGE1_K = (1, 6, 36), 96, 10, 200
PIPE_KINDS = {"Flat": dict(index_type="Flat", prefilter="bf16"),
              "IVF": dict(index_type="IVF", nlist=co.NLIST, nprobe=10, list_tags=True)}


def _t(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _delta(p, seed, scale=0.02):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (scale * torch.randn(p.shape, generator=g)).to(device=p.device, dtype=p.dtype)


def _clone(out):
    return {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}


def _assert_outputs(got, want, what):
    assert set(k for k, v in got.items() if isinstance(v, torch.Tensor)) == set(want) >= set(OUT_KEYS), what
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (what, k)


def _requests(rec, users, exclude_from=None):
    """Every request of the per-step set on ``rec`` -> {name: outputs}.  ``exclude_from``: the results whose candidates the
    exclusion blocks are drawn from (the long-lived pipeline's own)."""
    uc, un = users
    outs = {}
    for B in BATCHES:
        plain = _clone(rec.recommend_device(uc[:B], un[:B], TOP_K, STAGE1_K))
        outs[f"B{B}/plain"] = plain
        src = (exclude_from or outs)[f"B{B}/plain"]["candidate_ids"]
        blk = torch.cat([src[:, :6], torch.full((B, 2), -1, dtype=torch.int64, device=src.device)], dim=1)
        outs[f"B{B}/exclude"] = _clone(rec.recommend_device(uc[:B], un[:B], TOP_K, STAGE1_K, exclude_ad_ids=blk))
        outs[f"B{B}/ecpm_cap"] = _clone(rec.recommend_device(uc[:B], un[:B], TOP_K, STAGE1_K, rank_by="ecpm", max_per_group=2))
    outs[f"B{BIG_BATCH}/plain"] = _clone(rec.recommend_device(uc[:BIG_BATCH], un[:BIG_BATCH], TOP_K, STAGE1_K))
    return outs


@pytest.mark.parametrize("index_type", list(co.PIPELINE_WALKS))
def test_pipeline_walk(index_type, tmp_path):
    from amdrec.index import FAISSIndex
    from amdrec.pipeline import AdRecommenderInference
    from amdrec.ranker import TransformerRanker
    from amdrec.towers import TwoTowerModel
    seed, n_steps = co.PIPELINE_WALKS[index_type]
    steps = co.walk(seed, co.PIPELINE_RULES, n_steps, "unique", n0=co.PIPELINE_ADS, add_sizes=co.PIPELINE_ADD_SIZES, bulk=0)
    first = co.initial_step("unique", co.PIPELINE_ADS)
    user, ad, nnum = cases.small_dims()
    make_tower = lambda: TwoTowerModel(dict(user), dict(ad), nnum)                       # noqa: E731
    make_ranker = lambda: TransformerRanker(dict(user), dict(ad), nnum, **RANKER_ARCH)   # noqa: E731
    tt, rk = make_tower(), make_ranker()
    tt.load_state_dict(_t(synth.two_tower_state(user, ad, nnum, seed=seed)))
    rk.load_state_dict(_t(synth.ranker_state(user, ad, nnum, seed=seed + 1, cross_scale=1.0 / 16, **RANKER_ARCH)))
    tt, rk = tt.cuda().eval(), rk.cuda().eval()
    feat_pool = synth.ad_features(ad, co.pool_rows(steps, co.PIPELINE_ADS), seed=seed + 2)
    users = tuple(_dev(a) for a in synth.user_batch(user, nnum, BIG_BATCH, seed=seed + 3))

    def embed(feats):
        with torch.no_grad():
            return tt.get_ad_embeddings(_dev(feats))

    def attrs(args):
        tags, groups, bids = co.row_attrs(args["vseed"], args["m"])[:3]
        return dict(tags=tags if args["tags"] else None, groups=groups if args["groups"] else None,
                    bids=bids if args["bids"] else None)

    # the long-lived pipeline: index trained on the first ads, saved empty for the twins, then the first add
    feats0 = feat_pool[:co.PIPELINE_ADS]
    emb0 = embed(feats0)
    idx = FAISSIndex(256, **PIPE_KINDS[index_type])
    idx.train(emb0)
    trained = str(tmp_path / "trained_empty.bin")
    idx.save(trained)
    model = co.CorpusModel(256, n_feat=feats0.shape[1])
    idx.add(emb0, list(first["ids"]), **attrs(first))
    model.add(emb0.cpu().numpy(), first["ids"], feats=feats0, **attrs(first))
    rec = AdRecommenderInference(two_tower_model=tt, transformer_ranker=rk, faiss_index=idx, ad_features=feats0)
    knobs = dict(make_tower=make_tower, make_ranker=make_ranker, kind=index_type, kinds=PIPE_KINDS, trained_file=trained,
                 heads="all")
    _requests(rec, users)                                    # every cache filled before the first step
    assert rk._hidden_cache_for(rec.ad_features) is not None and rk.x3_fallback_reason() is None
    graphs = []                                              # (step, replayer, what the twin of that step returned)
    for step, (rule, args) in enumerate(steps):
        if rule == "remove_ads":
            assert rec.remove_ads(list(args["ids"])) == model.remove(args["ids"]) == args["removed"]
        elif rule == "add_ads":
            feats = feat_pool[args["start"]:args["start"] + args["m"]]
            emb = embed(feats)
            rec.add_ads(emb, feats, list(args["ids"]), **attrs(args))
            model.add(emb.cpu().numpy(), args["ids"], feats=feats, **attrs(args))
        elif rule == "tower_update":
            with torch.no_grad():
                p = tt.user_tower.mlp[4].weight
                p.add_(_delta(p, args["vseed"]))
        elif rule == "ranker_update":
            with torch.no_grad():
                for p in (rk.feature_projection.weight, list(rk.ad_embeddings.values())[3].weight,
                          rk.transformer_layers[0].feed_forward.fc1.weight):
                    p.add_(_delta(p, args["vseed"]))
        elif rule == "load_state_dict":
            mod = rk if args["vseed"] % 2 else tt
            sd = {k: (v.detach().cpu() + _delta(v.detach().cpu(), args["vseed"] + i, 0.01)
                      if v.is_floating_point() and not k.endswith("running_var") else v.detach().cpu().clone())
                  for i, (k, v) in enumerate(mod.state_dict().items())}
            mod.load_state_dict(sd)
        elif rule == "heads":
            rec.heads_mode = knobs["heads"] = args["mode"]
        elif rule in ("set_bids", "set_groups"):
            vals = co.row_attrs(args["vseed"], model.n)[2 if rule == "set_bids" else 1]
            getattr(rec.faiss_index, rule)(vals)
            getattr(model, rule)(vals)
        assert rec.faiss_index.index.ntotal == model.n == rec.ad_features.shape[0] == args["n_after"], (step, rule)
        twin = co.fresh_pipeline(model, tt.state_dict(), rk.state_dict(), knobs)
        got = _requests(rec, users)
        want = _requests(twin, users, exclude_from=got)
        history = [r for r, _ in steps[:step + 1]]
        for name in want:
            _assert_outputs(got[name], want[name], f"seed {seed}: after step {step} of {history}: {name}")
        if rule == "capture":
            g = rec.capture(6, TOP_K, STAGE1_K)
            graphs.append((step, g, want["B6/plain"]))
        for s0, g, snapshot in graphs:                        # stale, consistent; a new capture: the current twin's result
            _assert_outputs(_clone(g(users[0][:6], users[1][:6])), snapshot,
                            f"seed {seed}: the graph of step {s0} replayed after step {step} of {history}")
    assert graphs and knobs["heads"] in ("all", "ctr_first")
    # the end state against float64: one request, all heads
    B = 6
    out = rec.recommend_device(users[0][:B], users[1][:B], TOP_K, STAGE1_K, heads="all")
    cand_ids, cs = out["candidate_ids"].cpu().numpy(), out["candidate_scores"].cpu().numpy()
    where = {x: p for p, x in enumerate(model.ids)}
    cand_pos = np.array([[where[int(i)] if np.isfinite(s) else -1 for i, s in zip(ri, rs)] for ri, rs in zip(cand_ids, cs)])
    rk_sd = {k: v.detach().cpu().numpy() for k, v in rk.state_dict().items()}
    uc_h, un_h = users[0][:B].cpu().numpy(), users[1][:B].cpu().numpy()
    l64 = po.logits64(rk_sd, uc_h, un_h, cand_pos, model.feats)
    logits = out["logits"].cpu().numpy().reshape(3, B, STAGE1_K)
    filled = cand_pos >= 0
    assert filled.sum() >= B * STAGE1_K // 2
    for i, t in enumerate(oracle.ranker.TASKS):
        ok, err = cases.logit_close(logits[i][filled], l64[t][filled], "scaled")
        assert ok, (t, err)
    ids_e, scores_e, _ = po.expected(cand_pos, cand_ids, logits, TOP_K)
    assert np.array_equal(out["ad_ids"].cpu().numpy(), ids_e)
    assert np.abs(out["scores"].cpu().numpy() - scores_e).max() <= 1e-6
