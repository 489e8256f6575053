"""Every device entry runs on the stream it was called on: the delayed producer of tests/streams.py.

Every other GPU test calls the library on torch's default stream; graph capture would reject a launch on the null stream,
but only for the few captured shapes.  Here each call is made on a side stream behind a 50 ms delay kernel, with its inputs
written behind that delay too (over benign poison), and its outputs are compared bit for bit with the same call on the
default stream.  A launch, memset or copy that the library issues on another stream than the given one runs before its
inputs exist and shows as a difference; ``test_the_method_sees_a_stray_*`` show that the method detects exactly that.

Objects follow the fresh-twin pattern of tests/coherence.py: the reference result comes from one object on the default
stream, the delayed call is made on a twin built the same way.  Unless a test says otherwise the twin is warmed once on the
default stream (packed weights, caches), so that the delayed call is the steady-state one; the first-call tests leave
the twin cold, and its lazy state is then built on the side stream, behind the delay.

HOST_SYNCING lists the calls that wait for the device internally: they cannot be enqueued behind a delay (the helper's
busy flag would be false).  They run under the side stream without the delay, the object then serves on the side
stream, and the results are compared with a twin that did the same on the default stream: these are checked for
stream-independence of their results only.

One stream at a time: the process-wide workspace is one buffer per device, so two streams with library work in flight at
once are outside the contract and not tested here.
"""
import numpy as np
import pytest
import torch

from amdrec import _lib
from tests import ivf_oracle as io
from tests import merge_oracle as mo
from tests import streams
from tests.serving_world import World

pytestmark = pytest.mark.gpu

HOST_SYNCING = ("FAISSIndex.train", "FAISSIndex.add (IVF, IVFPQ: the list assignment is read back; Flat: the non-finite check)",
                "FAISSIndex.remove_ids", "AdRecommenderInference.remove_ads", "AdRecommenderInference.add_ads",
                "AdRecommenderInference.batch_recommend", "AdRecommenderInference.recommend_tensors")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def world():
    return World()


def _users(world, n, seed):
    uc, un = world.tensor_users(n, seed, "cuda")
    return uc, un


def _unit(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return _dev(x / np.linalg.norm(x, axis=1, keepdims=True))


def _warm_then_check(call, ref_call, real, poison):
    """The twin's lazy state is built by one call on the default stream (on the poison: valid inputs), then the delayed call."""
    call(**poison)
    torch.cuda.synchronize()
    return streams.check_delayed(call, ref_call, real, poison)


# ---- the method -----------------------------------------------------------------------------------------------------------------
def test_the_method_sees_a_stray_read_on_the_default_stream():
    real = {"x": torch.arange(1000, dtype=torch.float32, device="cuda")}
    poison = {"x": torch.full((1000,), -5.0, device="cuda")}
    out, busy, seen = streams.delayed(lambda x: x * 2, real, poison, stray=lambda bufs: bufs["x"])
    assert busy
    assert torch.equal(out, real["x"] * 2)                           # work on the side stream sees the real inputs
    assert torch.equal(seen, poison["x"])                            # ... and the default stream, at the same time, the poison


def test_the_method_sees_a_stray_launch_inside_a_call():
    """A call that does one of its steps on the default stream gives another result than on the default stream alone."""
    def leaky(x):
        with torch.cuda.stream(torch.cuda.default_stream()):
            y = x + 1                                                # (the stray step: reads its input before it exists)
        return y * 2
    real = {"x": torch.arange(1000, dtype=torch.float32, device="cuda")}
    poison = {"x": torch.full((1000,), -5.0, device="cuda")}
    ref = leaky(**real).clone()
    out, busy, _ = streams.delayed(leaky, real, poison)
    assert busy and streams.first_difference(out, ref) is not None
    assert torch.equal(out, (poison["x"] + 1) * 2)


# ---- towers ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tower_twins(world):
    return world.modules()[0].cuda().eval(), world.modules()[0].cuda().eval()


@pytest.mark.parametrize("rows", [257, 4096, 4097])              # the fused 16-row kernel up to 4096 rows, tiled GEMMs past it
def test_towers(world, tower_twins, rows):
    ref_tt, tt = tower_twins
    uc, un = _users(world, rows, 400 + rows)
    puc, pun = _users(world, rows, 500 + rows)
    for renorm in (False, True):
        _warm_then_check(lambda cat, num: tt.user_tower.encode(cat, num, check_indices=False, renormalize=renorm),
                         lambda cat, num: ref_tt.user_tower.encode(cat, num, check_indices=False, renormalize=renorm),
                         {"cat": uc, "num": un}, {"cat": puc, "num": pun})
    ads = _dev(world.table)
    real, poison = ads[torch.arange(rows, device="cuda") % len(ads)], ads[(torch.arange(rows, device="cuda") * 7 + 3) % len(ads)]
    _warm_then_check(lambda cat: tt.ad_tower.encode(cat, check_indices=False),
                     lambda cat: ref_tt.ad_tower.encode(cat, check_indices=False), {"cat": real}, {"cat": poison})


# ---- flat search ----------------------------------------------------------------------------------------------------------------
def _flat(world, prefilter):
    from amdrec.index import FAISSIndex
    idx = FAISSIndex(256, index_type="Flat", prefilter=prefilter)
    idx.add(world.rec.faiss_index._xb[:world.rec.faiss_index._n].clone(), tags=world.tags, groups=world.groups, boosts=world.boosts)
    return idx


@pytest.fixture(scope="module")
def flat_twins(world):
    return {p: (_flat(world, p), _flat(world, p)) for p in ("bf16", "fp32")}


@pytest.mark.parametrize("prefilter", ["bf16", "fp32"])
@pytest.mark.parametrize("nq", [1, 32, 512])                     # the fused finalize, the general one, the 512-query kernels
def test_flat_search(world, flat_twins, nq, prefilter):
    ref_idx, idx = flat_twins[prefilter]
    k, E = 100, 16
    q, pq = _unit(nq, 256, 600 + nq), _unit(nq, 256, 700 + nq)
    rng = np.random.default_rng(800 + nq)
    plain = ref_idx.search_device(q, k, normalize=False)[0]
    require_all = rng.integers(0, 2, nq).astype(np.int64)
    require_all[0] = 1                                               # (at least one query is constrained, also at nq = 1)
    real = {"q": q, "excl": plain[:, ::6][:, :E].contiguous(), "all_": _dev(require_all),
            "any_": _dev(rng.choice(np.array([0, 6, 12], dtype=np.int64), nq)), "w": _dev(rng.uniform(0.5, 2.0, nq).astype(np.float32))}
    poison = {"q": pq, "excl": _dev(rng.integers(0, 3000, (nq, E)).astype(np.int64)),
              "all_": torch.full((nq,), 8, dtype=torch.int64, device="cuda"), "any_": torch.full((nq,), 1, dtype=torch.int64, device="cuda"),
              "w": torch.full((nq,), -3.0, device="cuda")}
    options = {"plain": lambda i, a: i.search_device(a["q"], k, normalize=False, return_positions=True),
               "normalize": lambda i, a: i.search_device(a["q"], k),
               "exclude": lambda i, a: i.search_device(a["q"], k, normalize=False, exclude=a["excl"]),
               "masks": lambda i, a: i.search_device(a["q"], k, normalize=False, require_all=a["all_"], require_any=a["any_"]),
               "boost": lambda i, a: i.search_device(a["q"], k, normalize=False, boost_weight=a["w"]),
               "stage1_cap": lambda i, a: i.search_device(a["q"], k, normalize=False, max_per_group=2, exclude=a["excl"])}
    results = {}
    for name, fn in options.items():
        results[name] = _warm_then_check(lambda fn=fn, **a: fn(idx, a), lambda fn=fn, **a: fn(ref_idx, a), real, poison)
    for name in ("exclude", "masks", "boost", "stage1_cap"):         # every option changes the result
        assert not torch.equal(results[name][0], results["normalize"][0]), name


# ---- IVF and IVFPQ --------------------------------------------------------------------------------------------------------------
NLIST = 32


def _ivf(dim=64):
    from amdrec.index import FAISSIndex
    xb, centres = io.surface_corpus(dim, "long", NLIST)
    idx = FAISSIndex(dim, index_type="IVF", nlist=NLIST, nprobe=8)
    idx.set_trained_centroids(centres)
    idx.add(xb)
    return idx, centres


def _scan_tags(fn):
    _lib.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {t for t, e in _lib.profile_report().items() if e["launches"] and (t.startswith("ivf_scan") or t == "ivf_filter_bounds")}
    finally:
        _lib.profile_enable(False)


def test_ivf_on_every_scan_path(monkeypatch):
    """The per-pair, grouped, two-phase fp32 and two-phase bf16-prefiltered scans, forced as tests/test_ivf_surface_gpu.py
    forces them and recognised by their profile tags (read on the reference index)."""
    from amdrec import ivf
    (ref_idx, centres), (idx, _) = _ivf(), _ivf()
    k = 50

    def queries(nq, seed):
        rng = np.random.default_rng(seed)
        x = centres[rng.integers(0, NLIST, nq)] + 0.35 * rng.standard_normal((nq, centres.shape[1])).astype(np.float32)
        return _dev((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
    monkeypatch.setenv("AMDREC_IVF_QTILE", "64")
    for path, nq, nprobe, mixed in (("pairs", 3, 5, None), ("grouped", 48, 8, None), ("two_phase", 48, 16, "0"), ("mixed", 48, 16, "1")):
        if mixed is not None:
            monkeypatch.setenv("AMDREC_IVF_MIXED", mixed)
        ref_idx.index.nprobe = idx.index.nprobe = nprobe
        assert ivf.use_grouped_scan(nq, nprobe, NLIST) == (path != "pairs") and (nprobe >= ivf.TWO_PHASE_MIN_PROBES) == (mixed is not None)
        q, pq = queries(nq, 900 + nq + nprobe), queries(nq, 950 + nq + nprobe)
        tags = _scan_tags(lambda: ref_idx.search_device(q, k, normalize=False, return_positions=True))
        assert ("ivf_scan_pairs" in tags) == (path == "pairs") and ("ivf_filter_bounds" in tags) == (path == "mixed"), (path, tags)
        assert any("bf16" in t for t in tags) == (path == "mixed"), (path, tags)
        _warm_then_check(lambda q: idx.search_device(q, k, normalize=False, return_positions=True),
                         lambda q: ref_idx.search_device(q, k, normalize=False, return_positions=True), {"q": q}, {"q": pq})


@pytest.mark.parametrize("refine", [None, "fp32"])
def test_ivfpq_with_and_without_refine(refine, tmp_path):
    from amdrec.index import FAISSIndex
    dim = 64
    xb = io.clustered(3000, dim, NLIST, 1001)
    kw = dict(index_type="IVFPQ", nlist=NLIST, nprobe=8, pq_m=8, refine=refine)
    ref_idx = FAISSIndex(dim, **kw)
    ref_idx.add(xb)
    ref_idx.save(str(tmp_path / "pq.bin"))
    idx = FAISSIndex(dim, **kw)                                     # the twin: the same trained state and codes, loaded
    idx.load(str(tmp_path / "pq.bin"))
    q, pq = _dev(io.clustered(40, dim, NLIST, 1002)), _dev(io.clustered(40, dim, NLIST, 1003))
    _warm_then_check(lambda q: idx.search_device(q, 50, normalize=False, return_positions=True),
                     lambda q: ref_idx.search_device(q, 50, normalize=False, return_positions=True), {"q": q}, {"q": pq})


# ---- ranker ---------------------------------------------------------------------------------------------------------------------
def _ranker(world, engine, cached):
    rk = world.modules()[1]
    rk.gemm_engine = engine
    rk = rk.cuda().eval()
    table = _dev(world.table)
    if cached:
        rk.ensure_ad_cache(table)
    return rk, table


def _ranker_inputs(world, users, k, seed):
    uc, un = _users(world, users, seed)
    cand = _dev(np.random.default_rng(seed).integers(0, len(world.table), (users, k)).astype(np.int64))
    return {"uc": uc, "un": un, "cand": cand}


@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("users", [1, 16, 40])                   # 500, 8000 and 20 000 rows: column-split, 64-row, 128-row
def test_ranker_f16x3_score_candidates(world, users, cached):
    """With the per-ad caches (``cached``: the projection cache and the first-FFN hidden cache, whose program runs past
    16 384 rows) and without."""
    (ref_rk, ref_table), (rk, table) = _ranker(world, "f16x3", cached), _ranker(world, "f16x3", cached)
    assert (rk._hidden_cache_for(table) is not None) == cached
    real, poison = _ranker_inputs(world, users, 500, 1100 + users), _ranker_inputs(world, users, 500, 1200 + users)
    _warm_then_check(lambda uc, un, cand: rk.score_candidates(uc, un, cand, table, raw=True)[1],
                     lambda uc, un, cand: ref_rk.score_candidates(uc, un, cand, ref_table, raw=True)[1], real, poison)


@pytest.mark.parametrize("engine", ["fp32", "bf16x6", "f16"])
def test_ranker_other_engines_score_candidates(world, engine):
    (ref_rk, ref_table), (rk, table) = _ranker(world, engine, True), _ranker(world, engine, True)
    for users in (1, 16):
        real, poison = _ranker_inputs(world, users, 500, 1300 + users), _ranker_inputs(world, users, 500, 1400 + users)
        _warm_then_check(lambda uc, un, cand: rk.score_candidates(uc, un, cand, table, raw=True)[1],
                         lambda uc, un, cand: ref_rk.score_candidates(uc, un, cand, ref_table, raw=True)[1], real, poison)


def test_ranker_ctr_first_and_winner_scores(world):
    (ref_rk, ref_table), (rk, table) = _ranker(world, "f16x3", True), _ranker(world, "f16x3", True)
    users, k, top_k = 4, 500, 10
    assert rk.ctr_first_ready(table, users * k, users * top_k) and ref_rk.ctr_first_ready(ref_table, users * k, users * top_k)

    def two_passes(r, t):
        def call(uc, un, cand, slots):
            ctr, trunk = r.score_ctr_first(uc, un, cand, t, _ready=True)
            scores = torch.zeros((3, users, top_k), dtype=torch.float32, device="cuda")
            r.winner_scores(trunk, slots, k, scores)
            return ctr, scores
        return call
    rng = np.random.default_rng(1500)
    real, poison = _ranker_inputs(world, users, k, 1501), _ranker_inputs(world, users, k, 1502)
    real["slots"] = _dev(rng.integers(0, k, (users, top_k)).astype(np.int32))
    poison["slots"] = _dev(rng.integers(0, k, (users, top_k)).astype(np.int32))
    _warm_then_check(two_passes(rk, table), two_passes(ref_rk, ref_table), real, poison)


# ---- selection and merge --------------------------------------------------------------------------------------------------------
def _selection_inputs(n_users, k_c, n_rows, seed):
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, n_rows, (n_users, k_c)).astype(np.int64)
    pos[rng.random(pos.shape) < 0.1] = -1
    return {"logits": _dev(rng.standard_normal((3, n_users * k_c)).astype(np.float32)), "ids": _dev(np.where(pos >= 0, pos * 3 + 1, 10 ** 6)),
            "pos": _dev(pos), "reserve": _dev(rng.uniform(0.0, 0.5, n_users).astype(np.float32))}


@pytest.mark.parametrize("entry", ["plain", "capped", "auction", "diverse"])
def test_selection_entries(entry):
    lib = _lib.load()
    n_users, k_c, top_k, n_rows, dim = 5, 513, 33, 3000, 64
    rng = np.random.default_rng(1600)
    group_of, bid_of = _dev(rng.integers(-1, 40, n_rows).astype(np.int64)), _dev(rng.uniform(0.1, 5.0, n_rows).astype(np.float32))
    rows = _unit(n_rows, dim, 1601)

    def call(logits, ids, pos, reserve):
        out_ids = torch.empty((n_users, top_k), dtype=torch.int64, device="cuda")
        scores = torch.empty((3, n_users, top_k), dtype=torch.float32, device="cuda")
        slots = torch.empty((n_users, top_k), dtype=torch.int32, device="cuda")
        extra = [torch.empty((n_users, top_k), dtype=torch.float32, device="cuda") for _ in range({"auction": 2, "diverse": 1}.get(entry, 0))]
        head = (_lib.ptr(logits), logits.stride(0), 3, 0, _lib.ptr(ids), _lib.ptr(pos), n_users, k_c, top_k)
        outs = (_lib.ptr(out_ids), _lib.ptr(scores), _lib.ptr(slots))
        if entry == "plain":
            _lib.check(lib.amdrec_select_topk(*head, *outs, _lib.stream_ptr("cuda")))
        elif entry == "capped":
            _lib.check(lib.amdrec_select_topk_capped(*head, *outs, _lib.ptr(group_of), n_rows, 2, _lib.stream_ptr("cuda")))
        elif entry == "auction":
            _lib.check(lib.amdrec_select_topk_auction(*head, _lib.ptr(bid_of), n_rows, _lib.ptr(reserve), _lib.ptr(group_of), n_rows, 2,
                                                      *outs, _lib.ptr(extra[0]), _lib.ptr(extra[1]), _lib.stream_ptr("cuda")))
        else:
            _lib.check(lib.amdrec_select_topk_diverse(*head, _lib.ptr(rows), n_rows, rows.stride(0), dim, 0.5, 64, _lib.ptr(group_of),
                                                      n_rows, 2, *outs, _lib.ptr(extra[0]), _lib.stream_ptr("cuda")))
        return [out_ids, scores, slots] + extra
    streams.check_delayed(call, call, _selection_inputs(n_users, k_c, n_rows, 1602), _selection_inputs(n_users, k_c, n_rows, 1603))


def test_cross_shard_merge_entry():
    lib = _lib.load()
    n_lists, list_k, k, nq = 8, 128, 500, 9

    def packed(seed):
        S, P = mo.build_case(n_lists, list_k, nq, seed, "tails")
        host, s_off, p_off, stride = mo.pack_host(S, P, nq)
        return _dev(host), s_off, p_off, stride
    buf, s_off, p_off, stride = packed(1700)
    poison = packed(1701)[0]

    def call(buf):
        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(lib.amdrec_topk_merge_partial(_lib.C.c_void_p(buf.data_ptr() + s_off), _lib.C.c_void_p(buf.data_ptr() + p_off), n_lists,
                                                 list_k, stride, 0, nq, k, _lib.ptr(D), _lib.ptr(I), _lib.ptr(cnt), _lib.stream_ptr("cuda")))
        return D, I, cnt
    D, I, cnt = streams.check_delayed(call, call, {"buf": buf}, {"buf": poison})
    S, P = mo.build_case(n_lists, list_k, nq, 1700, "tails")
    rD, rI, inexact = mo.merge_reference(S, P, k)
    assert np.array_equal(I.cpu().numpy(), rI) and int(cnt) == int(inexact.sum())


# ---- the pipeline: eager, replayed, and cold ------------------------------------------------------------------------------------
OUT_KEYS = ("ad_ids", "scores", "candidate_ids", "candidate_scores", "logits")


def _device_result(out):
    return {k: out[k] for k in OUT_KEYS + ("ecpm", "prices", "diversity_values") if k in out}


@pytest.fixture(scope="module")
def rec_twins(world):
    return world.build(index_tower=world.tower)[0], world.build(index_tower=world.tower)[0]


@pytest.mark.parametrize("options", [{}, dict(rank_by="ecpm", max_per_group=2), dict(diversity=0.5), dict(heads="ctr_first"),
                                     dict(stage1_max_per_group=3)], ids=lambda o: "-".join(o) or "plain")
def test_recommend_device_eager(world, rec_twins, options):
    ref_rec, rec = rec_twins
    for B in (1, 8):
        uc, un = _users(world, B, 1800 + B)
        puc, pun = _users(world, B, 1900 + B)
        _warm_then_check(lambda uc, un: _device_result(rec.recommend_device(uc, un, 10, 200, **options)),
                         lambda uc, un: _device_result(ref_rec.recommend_device(uc, un, 10, 200, **options)),
                         {"uc": uc, "un": un}, {"uc": puc, "un": pun})


def test_graphed_recommender_replayed_on_the_side_stream(world, rec_twins):
    """The replayer's input copies and the graph launch both go to the stream of the call."""
    ref_rec, rec = rec_twins
    B = 4
    g = rec.capture(B, 10, 200, max_exclude=8)
    uc, un = _users(world, B, 2000)
    puc, pun = _users(world, B, 2001)
    ref = ref_rec.recommend_device(uc, un, 10, 200)
    excl, pexcl = ref["ad_ids"][:, :8].contiguous(), ref["candidate_ids"][:, 20:28].contiguous()
    eager = _device_result(ref_rec.recommend_device(uc, un, 10, 200, exclude_ad_ids=excl))
    out = streams.check_delayed(lambda uc, un, ex: _device_result(g(uc, un, exclude=ex)),
                                lambda uc, un, ex: _device_result(g(uc, un, exclude=ex)),
                                {"uc": uc, "un": un, "ex": excl}, {"uc": puc, "un": pun, "ex": pexcl})
    assert torch.equal(out["ad_ids"], eager["ad_ids"]) and torch.equal(out["scores"], eager["scores"])


def test_first_call_on_the_side_stream(world):
    """A never-called recommender - no packed weights (the fold is part of the ranker's pack), no ad caches - makes its first
    call on the side stream, behind the delay: everything it builds on the way is built there.  (Its Flat index built its
    bf16 shadow rows inside add(), which waits for the device; the shadow rows that ARE built lazily, an IVF index's, are
    built behind the delay in test_first_search_of_a_loaded_ivf_index_on_the_side_stream[mixed].)"""
    cold = world.build(index_tower=world.tower)[0]
    assert cold.transformer_ranker._packed is None and cold.two_tower_model.user_tower._packed is None
    assert cold.transformer_ranker._ad_cache is None
    uc, un = _users(world, 3, 2100)
    puc, pun = _users(world, 3, 2101)
    streams.check_delayed(lambda uc, un: _device_result(cold.recommend_device(uc, un, 10, 200)),
                          lambda uc, un: _device_result(world.rec.recommend_device(uc, un, 10, 200)),
                          {"uc": uc, "un": un}, {"uc": puc, "un": pun})
    assert cold.transformer_ranker._packed is not None and cold.transformer_ranker._ad_cache is not None


@pytest.mark.parametrize("path", ["grouped", "mixed"])
def test_first_search_of_a_loaded_ivf_index_on_the_side_stream(tmp_path, monkeypatch, path):
    """A loaded IVF index lays out its lists at the first search, and the first search on the bf16-prefiltered two-phase
    scan ("mixed": nprobe 16, forced on) also builds the bf16 shadow rows of the lists (IVFState._list_shadow,
    amdrec_bf16_rows).  Here that search is made behind the delay, on an index that was never searched and is not warmed:
    layout and shadow are built on the side stream, and read there by the scan that follows them."""
    from amdrec import ivf
    from amdrec.index import FAISSIndex
    nprobe = 16 if path == "mixed" else 8
    monkeypatch.setenv("AMDREC_IVF_QTILE", "64")
    monkeypatch.setenv("AMDREC_IVF_MIXED", "1" if path == "mixed" else "0")
    assert ivf.use_grouped_scan(48, nprobe, NLIST) and (nprobe >= ivf.TWO_PHASE_MIN_PROBES) == (path == "mixed")
    ref_idx, centres = _ivf()
    ref_idx.save(str(tmp_path / "ivf.bin"))
    idx = FAISSIndex(64, index_type="IVF", nlist=NLIST, nprobe=nprobe)
    idx.load(str(tmp_path / "ivf.bin"))
    ref_idx.index.nprobe = idx.index.nprobe = nprobe
    q, pq = _dev(io.clustered(48, 64, NLIST, 2200)), _dev(io.clustered(48, 64, NLIST, 2201))
    tags = _scan_tags(lambda: ref_idx.search_device(q, 50, normalize=False, return_positions=True))
    assert ("ivf_filter_bounds" in tags and any("bf16" in t for t in tags)) == (path == "mixed"), tags
    assert idx._ivf.lists is None and idx._ivf._shadow is None       # never searched: no list layout, no shadow
    streams.check_delayed(lambda q: idx.search_device(q, 50, normalize=False, return_positions=True),
                          lambda q: ref_idx.search_device(q, 50, normalize=False, return_positions=True), {"q": q}, {"q": pq})
    assert idx._ivf.lists is not None and (idx._ivf._shadow is not None) == (path == "mixed")


# ---- calls that synchronise with the host: stream-independence of results only ---------------------------------------------------
def _serve(rec, world):
    uc, un = _users(world, 4, 2300)
    return _device_result(rec.recommend_device(uc, un, 10, 200))


@pytest.mark.parametrize("kind", ["Flat", "IVF", "IVFPQ"])
def test_index_build_add_and_remove_under_the_side_stream(kind):
    """train + add, enable_list_tags, a second add, remove_ids, then searches - all under the side stream (no delay: these calls wait for the
    device, HOST_SYNCING) - against a twin that did the same on the default stream."""
    from amdrec.index import FAISSIndex
    dim = 64
    xb = io.clustered(3300, dim, NLIST, 2400)
    q = _dev(io.clustered(40, dim, NLIST, 2401))

    def life():
        idx = FAISSIndex(dim, index_type=kind, nlist=NLIST, nprobe=8)
        idx.add(xb[:3000], list(range(10, 3010)), tags=np.arange(3000) % 16)
        first = idx.search_device(q, 50, normalize=False)
        idx.enable_list_tags()                                       # (the list-order tags of a built index)
        idx.add(xb[3000:], list(range(5000, 5300)))
        removed = idx.remove_ids(list(range(100, 400)))
        assert removed == 300
        mask = torch.full((40,), 1, dtype=torch.int64, device="cuda")
        return first, idx.search_device(q, 50, normalize=False), idx.search_device(q, 50, normalize=False, require_all=mask)
    ref = streams.tree_map(torch.clone, life())
    torch.cuda.synchronize()
    why = streams.first_difference(streams.on_stream(life), ref)
    assert why is None, why


def test_reference_api_and_live_corpus_under_the_side_stream(world):
    """batch_recommend / recommend_tensors, remove_ads and add_ads under the side stream (HOST_SYNCING), then the object
    serves on the side stream; against a twin that did the same on the default stream."""
    users = world.dict_users(5, 2500)
    uc, un = world.tensor_users(5, 2501)
    emb = _unit(40, 256, 2502)
    feats = world.table[:40]

    def life(rec):
        def run():
            a = rec.batch_recommend(users, top_k=10, stage1_k=200)
            b = rec.recommend_tensors(uc, un, top_k=10, stage1_k=200, rank_by="ecpm")
            removed = rec.remove_ads(list(range(50, 250)))
            rec.add_ads(emb, feats, ad_ids=list(range(9000, 9040)))
            c = rec.recommend_tensors(uc, un, top_k=10, stage1_k=200)
            strip = lambda rs: [{k: v for k, v in r.items() if k != "timing"} for r in rs]     # noqa: E731
            return strip(a), strip(b), removed, strip(c), _serve(rec, world)
        return run
    ref = life(world.build(index_tower=world.tower)[0])()
    torch.cuda.synchronize()
    why = streams.first_difference(streams.on_stream(life(world.build(index_tower=world.tower)[0])), ref)
    assert why is None, why
