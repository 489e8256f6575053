"""GPU: non-finite and out-of-range numerical feature rows (tests/envelope.py) through everything they reach - the request
side's amdrec_prep_numerical, the user tower on each of its kernels, the ranker on each engine and kernel shape, the
broadcast and CTR-first paths, and the serving pipeline above the tower's small-batch threshold.

The contract, pinned to the reference by tests/golden/envelope_<case>.npz (tests/test_feature_envelope_cpu.py): a row with
a NaN or an infinity in a numerical feature leaves the tower as a NaN embedding and the ranker as NaN logits in every task,
on every path and engine, as the reference's torch.relu keeps a NaN where a bare fmaxf would return 0; every finite row -
scaled by 2^20 or 2^40, with a single 2^60 feature, all zeros, 1e-30, negative zeros - meets the float64 oracle within the
project's tolerances; and a bad row changes no other row's bits.

Row counts are the smallest that reach each kernel; the planted rows sit on the tile edges of the kernels (rows 0, 15, 16,
63, 64, 79 - tile 4 is tile 0's partner in the paired FFN phase -, 127, 128 and the last row).  The float64 oracle runs on
the planted rows alone (the networks are row-wise); the ordinary rows are compared, bit for bit, with the same batch
without the planted rows."""
import functools
import warnings

import numpy as np
import pytest
import torch

import oracle
from amdrec import _lib, synth
from tests import cases, envelope

pytestmark = pytest.mark.gpu

DENORM = 2.0 ** -149
U24 = 2.0 ** -24


def _t(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _profiled(fn):
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        tags = set(_lib.profile_report())
    finally:
        _lib.profile_enable(False)
    return out, tags


def _plant(un, required, extras):
    """NONFINITE families (cycled) on the ``required`` rows, one FINITE family each on the first six free ``extras``; rows
    past the batch are dropped.  -> (planted copy, family per row, planted positions)."""
    rows = un.shape[0]
    req = sorted({p for p in required if 0 <= p < rows})
    ext = [p for p in extras if 0 <= p < rows and p not in req][:len(envelope.FINITE)]
    fams = [envelope.NONFINITE[i % len(envelope.NONFINITE)] for i in range(len(req))] + list(envelope.FINITE[:len(ext)])
    bad, fam = envelope.bad_rows(un, req + ext, fams)
    return bad, fam, np.array(req + ext)


# ---- a. amdrec_prep_numerical ------------------------------------------------------------------------------------------
def _prep(x, mean, scale):
    x, mean, scale = _cu(x), _cu(mean), _cu(scale)
    out = torch.empty_like(x)
    _lib.check(_lib.load().amdrec_prep_numerical(_lib.ptr(x), _lib.ptr(mean), _lib.ptr(scale), _lib.ptr(out),
                                                 x.shape[0], x.shape[1], _lib.stream_ptr(x.device)))
    return out.cpu().numpy()


def _prep_pool():
    """+-0, float32 denormals, +-2^e for e in -126 .. 127, the largest finite float, +-inf, NaN, negative and positive
    ordinary values."""
    f = np.float32
    pows = np.array([2.0 ** e for e in range(-126, 128)], dtype=np.float64).astype(f)
    den = np.array([2.0 ** -149, 2.0 ** -140, 3 * 2.0 ** -130, 2.0 ** -127, 2.0 ** -126 - 2.0 ** -149], dtype=np.float64).astype(f)
    odd = np.array([1e-30, 0.5, 1.0, 1.5, 3.0, 7.0, 99.5, 12345.678, 1e30, np.finfo(f).max], dtype=f)
    pool = np.concatenate([f([0.0, -0.0, np.inf, -np.inf, np.nan]), pows, -pows, den, -den, odd, -odd])
    return pool


PREP_COUNTS = (1, 255, 256, 257, 70001)
PREP_MEANS, PREP_SCALES = (0.0, 3.0, -3.0, 80.0), (1.0, 2.0 ** -10, 2.0 ** 10, 1e-3)


def _prep_rule(got, x, mean, scale):
    """The rule of the issue on one result block -> worst |d| / bound over the finite results.  3 ulp of arithmetic (log1pf
    within 2 ulp per the ROCm math tables, one correctly rounded subtraction and one division), the 8 a 2.5x margin."""
    ref = envelope.prep_reference(x, mean, scale)
    nan_in, inf_in = np.isnan(x), np.isinf(x)
    assert np.isnan(got[nan_in]).all() and not np.isnan(got[~nan_in]).any()
    assert (got[inf_in] == np.inf).all()                                  # +-inf in, +inf out (every scale is positive)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, ~(nan_in | inf_in)) and np.isfinite(got[fin]).all()
    x64 = np.abs(x.astype(np.float64))
    bound = 8 * U24 * (np.log1p(x64, where=fin, out=np.zeros_like(x64)) + np.abs(np.float32(mean).astype(np.float64))) \
        / np.abs(np.float32(scale).astype(np.float64)) + DENORM
    bound = np.broadcast_to(bound, got.shape)
    return float((np.abs(got.astype(np.float64)[fin] - ref[fin]) / bound[fin]).max()) if fin.any() else 0.0


@pytest.mark.parametrize("cols", [1, 5, 13])
def test_prep_numerical_against_float64(cols, accuracy):
    """Element counts 1, 255, 256, 257 and 70 001 (cols = 1 reaches each exactly; 5 and 13 columns take the row counts on
    either side of count / cols, so the last block of the launch is partial, full and one element long), every mean x scale
    pair on every column position, and -x against x bit for bit."""
    pool = _prep_pool()
    rng = np.random.default_rng(100 + cols)
    combos = [(m, s) for m in PREP_MEANS for s in PREP_SCALES]
    worst = 0.0
    for count in PREP_COUNTS:
        for rows in sorted({max(1, count // cols), -(-count // cols)}):
            n = rows * cols
            for shift in range(len(combos)):
                # the whole pool in a fresh order, repeated (or, in a batch shorter than the pool, a fresh draw from it)
                x = np.resize(pool[rng.permutation(pool.size)], n).reshape(rows, cols)
                mean = np.array([combos[(c + shift) % len(combos)][0] for c in range(cols)], dtype=np.float32)
                scale = np.array([combos[(c + shift) % len(combos)][1] for c in range(cols)], dtype=np.float32)
                got = _prep(x, mean, scale)
                neg = _prep(-x, mean, scale)
                assert np.array_equal(got.view(np.int32), neg.view(np.int32)), (rows, cols, shift)
                r = _prep_rule(got, x, mean, scale)
                print(f"prep rows {rows} cols {cols} shift {shift}: max |d| / bound {r:.3f}")
                worst = max(worst, r)
    accuracy(f"envelope/prep_numerical/cols{cols}", "prep_numerical", worst)
    assert worst <= 1.0, worst


# ---- shared small world (a's preprocess_batch part and e) ------------------------------------------------------------
PIPE_SEED, PIPE_ADS = 21, 2000


@functools.lru_cache(maxsize=None)
def _pipe_world():
    from amdrec.ranker import TransformerRanker
    from amdrec.towers import TwoTowerModel
    user, ad, nnum = cases.small_dims()
    tt = TwoTowerModel(dict(user), dict(ad), nnum)
    tt.load_state_dict(_t(synth.two_tower_state(user, ad, nnum, seed=PIPE_SEED)))
    rk = TransformerRanker(dict(user), dict(ad), nnum)
    rk.load_state_dict(_t(synth.ranker_state(user, ad, nnum, seed=PIPE_SEED + 1, cross_scale=cases.CROSS["scaled"])))
    table = synth.ad_features(ad, PIPE_ADS, seed=PIPE_SEED + 2)
    tt = tt.cuda().eval()
    with torch.no_grad():
        emb = tt.get_ad_embeddings(_cu(table)).clone()
    return dict(user=user, ad=ad, nnum=nnum, tt=tt, rk=rk.cuda().eval(), table=table, emb=emb)


def _pipe_rec(**kind):
    from amdrec.index import FAISSIndex
    from amdrec.pipeline import AdRecommenderInference
    w = _pipe_world()
    idx = FAISSIndex(256, **kind)
    idx.add(w["emb"])
    return AdRecommenderInference(two_tower_model=w["tt"], transformer_ranker=w["rk"], faiss_index=idx,
                                  ad_features=np.array(w["table"]))


def test_preprocess_batch_raw_python_values():
    """Raw values of 1e30, 2**40, -7, NaN and a missing key: the device transform against the host's float64 one under the
    rule of test_prep_numerical_against_float64."""
    from amdrec.pipeline import Preprocessor
    w = _pipe_world()
    rec = _pipe_rec(index_type="Flat")
    cols = [f"I{i}" for i in range(1, 14)]
    mean, scale = np.linspace(-3, 3, 13), np.array([1.0, 2.0 ** -10, 2.0 ** 10, 1e-3, 0.7] * 3)[:13]
    classes = {c: [f"cat_{j}" for j in range(card - 1)] + ["rare"] for c, card in w["user"].items()}
    rec.preprocessor = Preprocessor(classes, cols, mean, scale)
    raw = [1e30, 2 ** 40, -7, float("nan")]
    users = []
    for u in range(5):
        num = {c: raw[(i + u) % 4] if (i + u) % 5 else 1.25 * (i + 1) for i, c in enumerate(cols)}
        users.append({"categorical": {f"C{i}": f"cat_{(3 * u + i) % 40}" for i in range(1, 7)}, "numerical": num})
    del users[2]["numerical"]["I7"]                                       # -> 0 (inference.py:188)
    cat_d, num_d = rec.preprocess_batch(users)
    host = [rec.preprocess_user_features(u) for u in users]
    assert torch.equal(cat_d.cpu(), torch.cat([h[0] for h in host]))
    got, want = num_d.cpu().numpy(), torch.cat([h[1] for h in host]).numpy()
    x = np.array([[float(u["numerical"].get(c, 0)) for c in cols] for u in users], dtype=np.float32)
    assert np.isnan(x).sum() >= 4 and (x == np.float32(1e30)).any() and (x == -7).any() and x[2, 6] == 0
    assert np.array_equal(np.isnan(got), np.isnan(x)) and np.array_equal(np.isnan(want), np.isnan(x))
    worst = _prep_rule(got, x, mean.astype(np.float32), scale.astype(np.float32))
    assert worst <= 1.0, worst
    fin = ~np.isnan(x)
    bound = 8 * U24 * (np.log1p(np.abs(x.astype(np.float64)), where=fin, out=np.zeros(x.shape)) + np.abs(mean)) / scale + DENORM
    assert (np.abs(got.astype(np.float64) - want)[fin] <= bound[fin]).all()


# ---- b. towers --------------------------------------------------------------------------------------------------------------
TOWER_MODELS = ("demo", "tutorial", "single_linear")
TOWER_ROWS = (1, 1024, 1025, 4096, 4097)
TS_GEMV_MAX_ROWS, TS_MAX_ROWS = 1024, 4096


@functools.lru_cache(maxsize=None)
def _tower(name):
    from amdrec.towers import TwoTowerModel
    if name == "single_linear":
        user, ad, nnum, sd = cases.surface_tower_case(name)
        args = cases.TOWER_SURFACE[name][0]
    else:
        user, ad, nnum, sd, _ = cases.two_tower_case(name)
        args = cases.arch(name)["tt"]
    m = TwoTowerModel(dict(user), dict(ad), nnum, **args)
    m.load_state_dict(_t(sd))
    return m.cuda().eval(), sd, user, nnum


def _tower_kernel(name, rows):
    """The tag of the one-launch kernels (csrc/tower_small.hip), None for the tiled GEMMs past TS_MAX_ROWS."""
    if rows > TS_MAX_ROWS:
        return None
    if name == "demo":                                                   # the reference's widths: GEMV, then the pipelined kernel
        return "tower_gemv_1row" if rows <= TS_GEMV_MAX_ROWS else "tower_pipe_16rows"
    return "tower_fused_16rows"


def _check_tower_batch(name, rows, uc, un0, un, fam, pos, accuracy):
    m, sd, _, _ = _tower(name)
    want_tag = _tower_kernel(name, rows)
    fam_p = [fam[p] for p in pos]
    with np.errstate(all="ignore"):
        e64 = oracle.towers.user_tower(sd, uc[pos], un[pos], dtype=np.float64)
        e32 = oracle.towers.user_tower(sd, uc[pos], un[pos])
    bad64 = ~np.isfinite(e64)
    assert np.array_equal(bad64.all(axis=1), envelope.rows_of(fam_p, envelope.NONFINITE)) and \
        np.array_equal(bad64.any(axis=1), bad64.all(axis=1))            # the oracle's mask: whole rows, the NONFINITE families
    ordinary = envelope.rows_of(fam, envelope.ORDINARY)
    d_uc, d_un, d_un0 = _cu(uc), _cu(un), _cu(un0)
    for renorm in (False, True):
        if renorm:
            run = lambda x: m.user_tower.encode(d_uc, x, check_indices=False, renormalize=True)   # noqa: E731
            r64 = oracle.towers.l2_normalize(e64, dtype=np.float64)
            r32 = oracle.towers.l2_normalize(e32)
        else:
            run = lambda x: m.get_user_embeddings(d_uc, x)   # noqa: E731
            r64, r32 = e64, e32
        with torch.no_grad():
            got_t, tags = _profiled(lambda: run(d_un).clone())
            clean_t = run(d_un0).clone()
        tower_tags = {t for t in tags if t.startswith("tower_")}
        if want_tag is None:
            assert not tower_tags and any(t.startswith("l2norm") for t in tags), tags
        else:
            assert tower_tags == {want_tag}, (name, rows, tags)
        got = got_t.cpu().numpy()
        # 1. the non-finite mask is the float64 oracle's
        mask = ~np.isfinite(got)
        want_mask = np.zeros_like(mask)
        want_mask[pos] = bad64
        assert np.array_equal(mask, want_mask), (name, rows, renorm, sorted(set(np.nonzero(mask != want_mask)[0].tolist()))[:8])
        # 2. the finite planted rows, sized by the float32 oracle's own error on that row (8x between
        #    two realised maxima)
        for i, p in enumerate(pos):
            if fam_p[i] not in envelope.FINITE:
                continue
            err = float(np.abs(got[p] - r64[i]).max())
            own = float(np.abs(r32[i].astype(np.float64) - r64[i]).max())
            tol = max(cases.EMB_ATOL, 8 * own)
            print(f"tower {name} rows {rows} renorm {renorm} row {p} {fam_p[i]}: err {err:.3e} oracle32 {own:.3e} ratio {err / tol:.3f}")
            accuracy(f"envelope/tower_{name}/{fam_p[i]}", want_tag or "tiles", err / tol, rows=rows)
            assert err <= tol, (name, rows, renorm, p, fam_p[i], err, tol)
        # 3. the ordinary rows do not know about the planted ones
        keep = torch.from_numpy(np.nonzero(ordinary)[0]).cuda()
        assert torch.equal(_bits(got_t[keep]), _bits(clean_t[keep])), (name, rows, renorm)
        assert bool(torch.isfinite(clean_t).all())


@pytest.mark.parametrize("rows", TOWER_ROWS)
@pytest.mark.parametrize("name", TOWER_MODELS)
def test_user_tower_envelope(name, rows, accuracy):
    _, _, user, nnum = _tower(name)
    uc, un0 = synth.user_batch(user, nnum, rows, seed=900 + rows)
    if rows == 1:                                                        # one row: every family in its turn
        for f in envelope.FAMILIES:
            un, fam = envelope.bad_rows(un0, [0], [f])
            _check_tower_batch(name, rows, uc, un0, un, fam, np.array([0]), accuracy)
        return
    un, fam, pos = _plant(un0, (0, 15, 16, 4096, rows - 1), (1, 17, 14, 18, 31, 32))
    assert set(fam) == set(envelope.FAMILIES) | {envelope.ORDINARY}
    _check_tower_batch(name, rows, uc, un0, un, fam, pos, accuracy)


# ---- c. rankers, dense forward --------------------------------------------------------------------------------------------
RANKER_ARCHS = {"demo_scaled": ("demo", "scaled"), "demo_randn": ("demo", "randn"), "tutorial": ("tutorial", "scaled"),
                "x3_one_layer": ("x3_one_layer", "scaled")}
# engine, rows -> what the default architecture runs there: column-split; the 64-row shape; the 128-row shape with the paired
# FFN; the fp32 small shapes; the bf16x6 tiles
ENGINE_ROWS = (("f16x3", 21), ("f16x3", 4097), ("f16x3", 16385), ("fp32", 53), ("bf16x6", 8193))
MAX_ROWS = 16385
SMALL_ROWS, X3C_MAX_ROWS, X3B4_MAX_ROWS = 8192, 4096, 16384
REQUIRED = (0, 15, 16, 63, 64, 79, 127, 128)
EXTRAS = (1, 17, 65, 80, 126, 129, 2, 3, 4, 5, 6, 7)


@functools.lru_cache(maxsize=None)
def _ranker(arch):
    from amdrec.ranker import TransformerRanker
    name, cross = RANKER_ARCHS[arch]
    if name == "x3_one_layer":
        user, ad, nnum, sd = cases.surface_ranker_case(name, cross)
        args = cases.RANKER_SURFACE[name][0]
    else:
        user, ad, nnum, sd, _ = cases.ranker_case(name, cross)
        args = cases.arch(name)["rk"]
    m = TransformerRanker(dict(user), dict(ad), nnum, **args)
    m.load_state_dict(_t(sd))
    uc, un = synth.user_batch(user, nnum, MAX_ROWS, seed=181)
    ac = synth.ad_features(ad, MAX_ROWS, seed=182)
    return m.cuda().eval(), sd, (uc, un, ac)


@functools.lru_cache(maxsize=None)
def _ordinary_truth(arch):
    """float64 logits of the ordinary batch (needed for the batch's logit scale, which only the randn rule uses)."""
    _, sd, (uc, un, ac) = _ranker(arch)
    return oracle.ranker.forward(sd, uc, ac, un, dtype=np.float64)


def _x3_kernel(m, rows, variant):
    if variant == 32:
        return "ranker_rowowner_128_x3"
    nl = len(m.transformer_layers)
    d_ff = m.transformer_layers[0].feed_forward.fc1.out_features if nl else 0
    if rows <= X3C_MAX_ROWS and (nl == 0 or d_ff % 128 == 0):
        return "ranker_colsplit16_x3"
    return "ranker_rowowner16_64_x3" if rows <= X3B4_MAX_ROWS else "ranker_rowowner16_128_x3"


def _check_ranker_logits(got, clean, fam, pos, p64, cross, scale, label, engine, accuracy):
    """``got`` / ``clean``: [3, rows] device logits of the planted / the ordinary batch; ``p64``: float64 logits of the planted
    rows ``pos``."""
    fam_p = [fam[p] for p in pos]
    ref = np.stack([p64[t] for t in oracle.ranker.TASKS])
    bad64 = ~np.isfinite(ref)
    assert np.array_equal(bad64.all(axis=0), envelope.rows_of(fam_p, envelope.NONFINITE)) and \
        np.array_equal(bad64.any(axis=0), bad64.all(axis=0))
    g = got.cpu().numpy()
    mask = ~np.isfinite(g)
    want_mask = np.zeros_like(mask)
    want_mask[:, pos] = bad64
    assert np.array_equal(mask, want_mask), (label, engine, sorted(set(np.nonzero(mask != want_mask)[1].tolist()))[:12])
    assert np.isnan(g[want_mask]).all()
    for f in envelope.FINITE:
        sel = np.array([i for i, x in enumerate(fam_p) if x == f], dtype=np.int64)
        if not sel.size:
            continue
        for ti, t in enumerate(oracle.ranker.TASKS):
            ok, err = cases.logit_close(g[ti, pos[sel]], ref[ti, sel], cross, scale=scale)
            print(f"{label} {engine} {f} {t}: max err / bound {err:.3f}")
            accuracy(f"envelope/{label.split('/')[0]}/{f}", engine, err)
            assert ok, (label, engine, f, t, err)
    keep = torch.from_numpy(np.nonzero(envelope.rows_of(fam, envelope.ORDINARY))[0]).cuda()
    assert torch.equal(_bits(got[:, keep]), _bits(clean[:, keep])), (label, engine)
    assert bool(torch.isfinite(clean).all())


@pytest.mark.parametrize("engine,rows", ENGINE_ROWS)
@pytest.mark.parametrize("arch", list(RANKER_ARCHS))
def test_ranker_forward_envelope(arch, engine, rows, accuracy):
    m, sd, (uc, un0, ac) = _ranker(arch)
    name, cross = RANKER_ARCHS[arch]
    why = cases.x3_reason(name) if name != "x3_one_layer" else cases.RANKER_SURFACE[name][2]
    uc, un0, ac = uc[:rows], un0[:rows], ac[:rows]
    un, fam, pos = _plant(un0, REQUIRED + (rows - 1,), EXTRAS)
    assert set(fam) == set(envelope.FAMILIES) | {envelope.ORDINARY}
    with np.errstate(all="ignore"):
        p64 = oracle.ranker.forward(sd, uc[pos], ac[pos], un[pos], dtype=np.float64)
    scale = None
    if cross == "randn":
        keep = envelope.rows_of(fam, envelope.ORDINARY)
        scale = cases.logit_scale({t: v[:rows][keep] for t, v in _ordinary_truth(arch).items()})
    x3 = engine == "f16x3" and why is None
    want = "f16x3" if x3 else ("bf16x6" if engine != "fp32" and rows > SMALL_ROWS else "fp32")
    d = [_cu(uc), _cu(ac), _cu(un), _cu(un0)]
    try:
        m.gemm_engine = engine
        assert m.x3_fallback_reason() == why and m.gemm_engine_for(rows) == want
        for variant, fold in ([(16, True), (16, False), (32, True), (32, False)] if x3 else [(16, True)]):
            m.x3_variant, m.fold_first_attention = variant, fold
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)           # (the tutorial architecture's pack: no f16x3)
                pred, tags = _profiled(lambda: torch.stack(list(m(d[0], d[1], d[2]).values())).clone())
                clean = torch.stack(list(m(d[0], d[1], d[3]).values())).clone()
            x3_tags = {t for t in tags if t.endswith("_x3")}
            if x3:
                assert x3_tags == {_x3_kernel(m, rows, variant)}, (rows, variant, tags)
            else:
                assert not x3_tags and any(t.endswith("_x6") for t in tags) == (want == "bf16x6"), tags
            label = f"ranker_{arch}/rows{rows}/v{variant}{'f' if fold else 'u'}"
            _check_ranker_logits(pred, clean, fam, pos, p64, cross, scale, label, want, accuracy)
    finally:
        m.gemm_engine, m.x3_variant, m.fold_first_attention = "f16x3", 16, True


# ---- d. rankers, broadcast paths ----------------------------------------------------------------------------------------
BC_USERS, BC_K, BC_ADS = 5, 3277, 3000            # 16 385 rows: the 128-row shape
CF_USERS, CF_K = 9, 1821                          # 16 389 rows at a list length the winners' pass accepts (<= 2048)


@functools.lru_cache(maxsize=None)
def _broadcast_inputs(users=BC_USERS, k=BC_K):
    user, ad, nnum, _, _ = cases.ranker_case("demo", "scaled")
    uc, un0 = synth.user_batch(user, nnum, users, seed=191)
    table = synth.ad_features(ad, BC_ADS, seed=192)
    cand = np.random.default_rng(193).integers(0, BC_ADS, (users, k))
    cand[0, 0], cand[-1, -1] = BC_ADS - 1, 0
    un = un0.copy()
    un[2] = envelope.plant(un0[2], "nan_one", 4)
    un[3] = envelope.plant(un0[3], "pinf_one", 9)
    return _cu(uc), _cu(un0), _cu(un), _cu(table), _cu(cand)


def _bad_users_nan_others_same(got, clean, what):
    """[tasks, users, k] planes of the batch with users 2 (a NaN feature) and 3 (an infinite one) and of the ordinary one."""
    assert bool(torch.isnan(got[:, 2:4]).all()), what
    for u in [u for u in range(got.shape[1]) if u not in (2, 3)]:
        assert torch.equal(_bits(got[:, u]), _bits(clean[:, u])), (what, u)
    assert bool(torch.isfinite(clean).all()), what


@pytest.mark.parametrize("caches", ["none", "projection", "projection+hidden"])
def test_score_candidates_envelope(caches):
    """5 users x 3277 candidates: every candidate of the two bad users is NaN in all tasks, with and without the per-ad
    caches; the other users' rows are those of the ordinary batch."""
    m, _, _ = _ranker("demo_scaled")
    uc, un0, un, table, cand = _broadcast_inputs()
    try:
        m.cache_first_ffn = caches == "projection+hidden"
        m.cache_ad_projection(None)
        if caches != "none":
            m.ensure_ad_cache(table)
        assert (m._cache_for(table) is not None) == (caches != "none")
        assert (m._hidden_cache_for(table) is not None) == (caches == "projection+hidden")
        (tasks, got), tags = _profiled(lambda: m.score_candidates(uc, un, cand, table, check_indices=True, raw=True))
        got = got.clone()
        assert {t for t in tags if t.endswith("_x3")} == {"ranker_rowowner16_128_x3"}, tags
        clean = m.score_candidates(uc, un0, cand, table, raw=True)[1].clone()
        assert list(tasks) == list(oracle.ranker.TASKS)
        _bad_users_nan_others_same(got.view(3, BC_USERS, BC_K), clean.view(3, BC_USERS, BC_K), caches)
    finally:
        m.cache_first_ffn = True
        m.cache_ad_projection(None)


def test_ctr_first_pair_envelope():
    """amdrec_ranker_forward_ctr_first + amdrec_ranker_winner_heads on every row (identity slots): the CTR logits, the stored
    trunk rows and the winners' engagement / revenue probabilities of a bad user are NaN; the other users' are those of the
    ordinary batch."""
    m, _, _ = _ranker("demo_scaled")
    uc, un0, un, table, cand = _broadcast_inputs(CF_USERS, CF_K)
    rows = CF_USERS * CF_K
    assert rows > X3B4_MAX_ROWS
    try:
        m.ensure_ad_cache(table)
        assert m.ctr_first_ready(table, rows, rows), m.ctr_first_unsupported_reason()
        ident = torch.arange(CF_K, dtype=torch.int32, device="cuda").repeat(CF_USERS, 1).contiguous()
        res = []
        for x in (un, un0):
            ctr, trunk = m.score_ctr_first(uc, x, cand, table)
            ctr = ctr.clone()
            out = torch.full((3, CF_USERS, CF_K), 0.5, dtype=torch.float32, device="cuda")
            (_, tags) = _profiled(lambda: m.winner_scores(trunk, ident, CF_K, out))
            assert "ranker_winner_heads_x3" in tags, tags
            res.append((ctr.view(1, CF_USERS, CF_K), out[1:].clone()))
        _bad_users_nan_others_same(res[0][0], res[1][0], "ctr logits")
        _bad_users_nan_others_same(res[0][1], res[1][1], "winner heads")
        assert bool(((res[1][1] > 0) & (res[1][1] < 1)).all())
        full = m.score_candidates(uc, un, cand, table, raw=True)[1].view(3, CF_USERS, CF_K)
        assert torch.equal(_bits(res[0][0][0]), _bits(full[0]))          # CTR row: the all-heads path's, NaN payload included
    finally:
        m.cache_ad_projection(None)


# ---- e. the pipeline above the tower threshold -----------------------------------------------------------------------------
PIPE_B, PIPE_K1, PIPE_TOP = 4097, 16, 4
PIPE_NAN, PIPE_INF = (0, 2048, 4096), (7,)


PIPE_KINDS = {"Flat": dict(index_type="Flat"), "IVF": dict(index_type="IVF", nlist=16, nprobe=4),
              "IVFPQ": dict(index_type="IVFPQ", nlist=16, nprobe=4)}
PIPE_KEYS = ("ad_ids", "scores", "candidate_ids", "candidate_scores", "logits")


@functools.lru_cache(maxsize=None)
def _pipe_run(kind):
    """One recommend_device call on the batch with the bad users and one on the ordinary batch -> (out, clean, bad mask)."""
    w = _pipe_world()
    rec = _pipe_rec(**PIPE_KINDS[kind])
    uc, un0 = synth.user_batch(w["user"], w["nnum"], PIPE_B, seed=231)
    un = un0.copy()
    for u in PIPE_NAN:
        un[u] = envelope.plant(un0[u], "nan_one", u % 13)
    for u in PIPE_INF:
        un[u] = envelope.plant(un0[u], "pinf_one", u % 13)
    bad = np.zeros(PIPE_B, dtype=bool)
    bad[list(PIPE_NAN + PIPE_INF)] = True
    d_uc = _cu(uc)
    emb, tags = _profiled(lambda: w["tt"].user_tower.encode(d_uc, _cu(un), check_indices=False, renormalize=True).clone())
    assert not {t for t in tags if t.startswith("tower_")}, tags         # the tile path
    assert np.array_equal(torch.isnan(emb).all(dim=1).cpu().numpy(), bad) and \
        np.array_equal((~torch.isfinite(emb)).any(dim=1).cpu().numpy(), bad)
    out = rec.recommend_device(d_uc, _cu(un), PIPE_TOP, PIPE_K1)
    out = {k: out[k].clone() for k in PIPE_KEYS}
    clean = rec.recommend_device(d_uc, _cu(un0), PIPE_TOP, PIPE_K1)
    clean = {k: clean[k].clone() for k in PIPE_KEYS}
    return out, clean, bad


@pytest.mark.parametrize("kind", list(PIPE_KINDS))
def test_pipeline_above_the_tower_threshold_bad_users_disturb_nobody(kind):
    """B = 4097 users (the tiled tower GEMMs) over 2000 ads, users 0, 2048 and 4096 with a NaN feature and user 7 with an
    infinite one: their queries are NaN, and everyone else's results are, bit for bit, those of the batch with ordinary
    users in their place (what test_nan_user_gets_nothing_and_disturbs_nobody asserts at B = 5)."""
    out, clean, bad = _pipe_run(kind)
    g = torch.from_numpy(np.nonzero(~bad)[0]).cuda()
    assert bool((clean["ad_ids"] >= 0).all()) and bool((clean["scores"] > 0).all())
    assert torch.equal(out["ad_ids"][g], clean["ad_ids"][g])
    assert torch.equal(_bits(out["scores"][:, g]), _bits(clean["scores"][:, g]))
    assert torch.equal(out["candidate_ids"][g], clean["candidate_ids"][g])
    assert torch.equal(_bits(out["candidate_scores"][g]), _bits(clean["candidate_scores"][g]))
    lo, lc = out["logits"].view(3, PIPE_B, PIPE_K1), clean["logits"].view(3, PIPE_B, PIPE_K1)
    assert torch.equal(_bits(lo[:, g]), _bits(lc[:, g]))
    # whatever the search makes of a NaN query, a bad user never reads an ordinary-looking probability
    s = out["scores"][:, torch.from_numpy(np.nonzero(bad)[0]).cuda()]
    assert bool((torch.isnan(s) | (s == 0.0)).all()), s.tolist()


# Not one of the failures this file was written for, and not a small fix: the inverted-list searches file a NaN score as the
# fill score and still return the row (csrc/invlists.hpp; the contract of a NaN corpus row, tests/test_ivf_surface_gpu.py), so
# under IVF and IVFPQ a NaN QUERY comes back with the first rows of the probed lists as filled slots - measured at B = 4097:
# ad_ids [1, 2, 3, 7] for each of the four bad users, candidate_scores -inf (IVF) / +inf (IVFPQ), and, since the ranker keeps
# the NaN, NaN in all three probabilities where the Flat index gives -1 / 0.0.  Telling a NaN query from a NaN row takes a
# change in the list scans or in what the selection counts as a candidate.
_IVF_NAN_QUERY = pytest.mark.xfail(strict=True, reason="IVF / IVFPQ return the probed lists' first rows for a NaN query "
                                                        "(filled slots at the fill score), so the user reads real ad ids "
                                                        "with NaN probabilities, not -1 / 0.0")


@pytest.mark.parametrize("kind", ["Flat", pytest.param("IVF", marks=_IVF_NAN_QUERY),
                                  pytest.param("IVFPQ", marks=_IVF_NAN_QUERY)])
def test_pipeline_above_the_tower_threshold_bad_users_get_nothing(kind):
    """... and the bad users read -1 / 0.0 throughout: the search fills none of the slots of a NaN query."""
    out, _, bad = _pipe_run(kind)
    b = torch.from_numpy(np.nonzero(bad)[0]).cuda()
    fill = float("inf") if kind == "IVFPQ" else float("-inf")
    print(kind, "bad users: ad_ids", out["ad_ids"][b].tolist(), "scores", out["scores"][:, b].tolist(),
          "candidate_scores", out["candidate_scores"][b][:, :4].tolist())
    assert bool((out["candidate_scores"][b] == fill).all())
    assert bool((out["ad_ids"][b] == -1).all()) and bool((out["scores"][:, b] == 0.0).all())
