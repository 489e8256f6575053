"""GPU: the ranker's fast engines (f16x3, the production engine, and bf16x6) inside guarded exact-size buffers.

Every pass runs (i) through ``score_candidates`` / ``forward`` under ``both_ways`` (each workspace the binding asks for served
at exactly the queried size between guard bands) and (ii) as a direct ``amdrec_ranker_forward`` call that mirrors
``TransformerRanker._run`` with ``logits`` a guarded [n_tasks, rows] tensor (ld_logits == rows, as the binding calls it:
the kernels own 16, 64 or 128 rows per workgroup, so a store past the last valid row lands in the next task's logits or
in the band) and a guarded workspace of exactly ``amdrec_ranker_workspace`` bytes.  Row counts come from the dispatch in
csrc/ranker_x3.hip (column-split kernel up to 4096 rows, 64-row workgroups up to 16 384, 128-row workgroups beyond) and
csrc/layers.hip (the first-FFN hidden cache writes [U | Q] rows of d_model + d_ff floats into the U region of rows * d_model
floats: from ceil((d_model + d_ff) / d_model) candidates per user on, filled to its last float at exactly that many).  The
kernel that ran is read from the profile tags; the logits are held to the float64 rule of tests/test_models_gpu.py: error
against a float64 evaluation at most 4x the strict fp32 engine's own + 1e-7 of the logit scale.  Users repeat with period 7
over a 300-ad table, so one float64 table of 7 x 300 pairs is the truth of every shape."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from amdrec import _lib, synth
from tests import cases
from tests.guarded import both_ways, guarded
from tests.test_ffn1_cache_gpu import TAG as TAG_128, _cached_flops

pytestmark = pytest.mark.gpu

N_ADS, BASE_USERS = 300, 7
TAG_CS, TAG_64 = "ranker_colsplit16_x3", "ranker_rowowner16_64_x3"
X3_TAGS = (TAG_CS, TAG_64, TAG_128, "ranker_rowowner_128_x3")
ENGINES = ("f16x3", "bf16x6")


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Ctx:
    def __init__(self):
        from amdrec.ranker import TransformerRanker
        user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
        self.sd = sd
        self.models = {}
        for eng in ENGINES + ("fp32",):
            m = TransformerRanker(dict(user), dict(ad), nnum, **cases.arch("demo")["rk"])
            m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
            m.gemm_engine = eng
            self.models[eng] = m.cuda().eval()
        self.uc, self.un = synth.user_batch(user, nnum, BASE_USERS, seed=91)
        self.table = synth.ad_features(ad, N_ADS, seed=92)
        args = (np.repeat(self.uc, N_ADS, axis=0), np.tile(self.table, (BASE_USERS, 1)), np.repeat(self.un, N_ADS, axis=0))
        t64 = oracle.ranker.forward(sd, *args, dtype=np.float64)
        self.tasks = list(t64)
        self.truth = np.stack([t64[t].reshape(BASE_USERS, N_ADS) for t in self.tasks])     # [task, user, ad]
        self.scale = float(np.abs(self.truth).max())
        self.d_table = _cu(self.table)
        for m in self.models.values():
            m.ensure_ad_cache(self.d_table)
        self.fp32_err = {}

    def users(self, U):
        who = np.arange(U) % BASE_USERS
        return who, _cu(self.uc[who]), _cu(self.un[who])

    def err64(self, logits, who_rows, ad_rows):
        """logits [n_tasks, rows] (the binding's task order) against the truth of rows (user who_rows[r], ad ad_rows[r])."""
        return float(np.abs(logits.cpu().numpy().astype(np.float64) - self.truth[:, who_rows, ad_rows]).max())


@pytest.fixture(scope="module")
def ctx():
    return _Ctx()


def _profiled(run):
    _lib.profile_enable(True)
    try:
        out = run()
        torch.cuda.synchronize()
        rep = _lib.profile_report()
    finally:
        _lib.profile_enable(False)
    return out, rep


def _direct(m, user_cat, numerical, rowdiv, ad_cat, rowmap, rows, use_cache):
    """amdrec_ranker_forward as TransformerRanker._run calls it, with guarded logits and a guarded exact workspace."""
    dev = ad_cat.device
    params, tasks = m._pack(dev)
    cache = m._cache_for(ad_cat) if use_cache else None
    hidden = m._hidden_cache_for(ad_cat) if cache is not None else None
    params.ad_proj_cache = cache.data_ptr() if cache is not None else None
    params.ld_ad_proj_cache = cache.stride(0) if cache is not None else 0
    params.ad_hidden_cache = hidden.data_ptr() if hidden is not None else None
    params.ld_ad_hidden_cache = hidden.stride(0) if hidden is not None else 0
    lib = _lib.load()
    logits = guarded((len(tasks), rows), torch.float32, dev, "output")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = C.c_size_t(0)
    _lib.check(lib.amdrec_ranker_workspace(C.byref(params), rows, C.byref(nbytes)))
    ws = guarded((nbytes.value,), torch.uint8, dev, "scratch")
    _lib.check(lib.amdrec_ranker_forward(
        C.byref(params), _lib.ptr(user_cat), _lib.ptr(numerical), rowdiv, _lib.ptr(ad_cat), _lib.ptr(rowmap), rows,
        _lib.ptr(logits), logits.stride(0), _lib.ptr(flag), user_cat.shape[0], ad_cat.shape[0], _lib.ptr(ws), ws.numel(),
        _lib.stream_ptr(dev)))
    logits.check()
    ws.check()
    assert int(flag.item()) == 0 and logits.stride(0) == rows
    return logits


def _hold_to_truth(ctx, engine, key, logits, fp32_logits, who_rows, ad_rows, accuracy):
    assert bool(torch.isfinite(logits).all())
    if key not in ctx.fp32_err:
        ctx.fp32_err[key] = ctx.err64(fp32_logits(), who_rows, ad_rows)
    e, e32 = ctx.err64(logits, who_rows, ad_rows), ctx.fp32_err[key]
    accuracy(f"float64_truth/guarded/{key}", engine, e / max(e32, 1e-30), abs_err_vs_float64=e,
             fp32_engine_abs_err_vs_float64=e32, batch_logit_scale=ctx.scale)
    assert e <= 4.0 * e32 + 1e-7 * max(1.0, ctx.scale), (engine, key, e, e32)


def _hidden_cache_fits(m, users, k):
    """csrc/layers.hip: [U | Q] rows share U's region of rows * d_model floats."""
    d_model, d_ff = m.d_model, m.transformer_layers[0].feed_forward.fc1.out_features
    return users * (d_model + d_ff) <= users * k * d_model


# users x candidates -> the f16x3 kernel: column-split up to 4096 rows (21: rows % 16 != 0); 64-row workgroups up to
# 16 384; 128-row workgroups beyond
SHAPES = [(1, 500, TAG_CS), (1, 1, TAG_CS), (3, 7, TAG_CS), (9, 500, TAG_64), (4097, 1, TAG_64),
          (3277, None, TAG_128),      # x K_MIN candidates: [U | Q] fills the U region exactly, one valid row in the last workgroup
          (4097, -1, TAG_128),        # x (K_MIN - 1): 16 388 rows, [U | Q] does not fit, the plain U rows
          (5, 3277, TAG_128)]


@pytest.mark.parametrize("users,k,tag", SHAPES)
@pytest.mark.parametrize("engine", ENGINES)
def test_score_candidates_in_guarded_buffers(ctx, engine, users, k, tag, accuracy):
    m = ctx.models[engine]
    d_model, d_ff = m.d_model, m.transformer_layers[0].feed_forward.fc1.out_features
    k_min = -(-(d_model + d_ff) // d_model)              # candidates per user from which [U | Q] fits U's region
    k = k_min if k is None else (k_min - 1 if k == -1 else k)
    rows = users * k
    who, uc, un = ctx.users(users)
    cand = np.random.default_rng(rows).integers(0, N_ADS, (users, k))
    cand[0, 0], cand[-1, -1] = N_ADS - 1, 0
    d_cand = _cu(cand)
    run = lambda: (m.score_candidates(uc, un, d_cand, ctx.d_table, raw=True)[1],)      # noqa: E731
    (want,), rep = _profiled(run)
    x3 = {t for t in rep if t in X3_TAGS}
    if engine == "f16x3":
        assert m.gemm_engine_for(rows) == "f16x3" and x3 == {tag}, rep.keys()
        if tag == TAG_128:
            hc = k > 1 and _hidden_cache_fits(m, users, k)
            assert hc == (k >= k_min) and m._hidden_cache_for(ctx.d_table) is not None
            flops, full, cached = _cached_flops(rep, rows)
            assert flops == (cached if hc else full), (flops, full, cached)
            if users == 3277:
                assert users * (d_model + d_ff) == rows * d_model and rows % 128 == 1      # the region filled to its last float
    else:
        assert not x3 and m.gemm_engine_for(rows) == ("bf16x6" if rows > m.SMALL_ROWS else "fp32")
    arena = both_ways(run)
    need = C.c_size_t(0)
    _lib.check(_lib.load().amdrec_ranker_workspace(C.byref(m._pack(uc.device)[0]), rows, C.byref(need)))
    assert [s[2] for s in arena.served] == [need.value]
    got = _direct(m, uc, un, k, ctx.d_table, d_cand.view(-1), rows, use_cache=True)
    assert torch.equal(got, want)
    who_rows, ad_rows = np.repeat(who, k), cand.reshape(-1)
    fp32 = lambda: ctx.models["fp32"].score_candidates(uc, un, d_cand, ctx.d_table, raw=True)[1]      # noqa: E731
    _hold_to_truth(ctx, engine, f"score_candidates/{users}x{k}", want, fp32, who_rows, ad_rows, accuracy)


# forward(): dense rows, no cache, no hoisted user rows.  300: the column-split kernel on the dense X (f16x3) / the fp32
# small shapes (bf16x6 below SMALL_ROWS); 8193: 64-row workgroups on the dense X / the bf16x6 tiles
@pytest.mark.parametrize("rows,tag", [(300, TAG_CS), (8193, TAG_64)])
@pytest.mark.parametrize("engine", ENGINES)
def test_forward_in_guarded_buffers(ctx, engine, rows, tag, accuracy):
    m = ctx.models[engine]
    who, uc, un = ctx.users(rows)
    ads = np.random.default_rng(rows).integers(0, N_ADS, rows)
    ac = _cu(ctx.table[ads])
    names = m._pack(uc.device)[1]
    run = lambda: (torch.stack([m(uc, ac, un)[t] for t in names]),)      # noqa: E731
    (want,), rep = _profiled(run)
    x3 = {t for t in rep if t in X3_TAGS}
    if engine == "f16x3":
        assert x3 == {tag}, rep.keys()
    else:
        assert not x3 and m.gemm_engine_for(rows) == ("bf16x6" if rows > m.SMALL_ROWS else "fp32")
    both_ways(run)
    got = _direct(m, uc, un, 1, ac, None, rows, use_cache=False)
    assert torch.equal(got, want)
    fp32 = lambda: torch.stack([ctx.models["fp32"](uc, ac, un)[t] for t in names])      # noqa: E731
    _hold_to_truth(ctx, engine, f"forward/{rows}", want, fp32, who, ads, accuracy)


@pytest.mark.parametrize("rows", [21, 4097])
@pytest.mark.parametrize("fold", [False, True])
def test_x3_prefix_in_guarded_buffers(ctx, fold, rows):
    """amdrec_ranker_x3_prefix, the whole chain and the chain without the heads: x_out guarded with ld_out == 256, logits
    guarded, the workspace exactly ceil(rows / 128) * 128 * 1024 bytes.  On the folded model z = x0 + W_ov x0 + b_ov is written
    into that workspace first.  Bit-equal to the same call on plain tensors; the first and the last 64 rows' logits against
    float64 (oracle.ranker.chain_states) under the golden tolerance."""
    from amdrec.ranker import TransformerRanker
    from tests.test_x3_gpu import _prefix, _projected_rows
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    m = TransformerRanker(dict(user), dict(ad), nnum, **cases.arch("demo")["rk"])
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.fold_first_attention = fold
    m = m.cuda().eval()
    params, tasks = m._pack(torch.device("cuda", torch.cuda.current_device()))
    assert bool(params.x3.fold_attn1) == fold
    X = _projected_rows(sd, (user, ad, nnum), rows, seed=43)
    Xd = _cu(X)
    n_total = 2 * len(m.transformer_layers) + 3 + 1
    lib = _lib.load()
    for n in (n_total - 1, n_total):
        x0, l0 = _prefix(m, Xd, n)
        x_out = guarded((rows, 256), torch.float32, Xd.device, "output")
        logits = guarded((len(tasks), rows), torch.float32, Xd.device, "output")
        ws = guarded((-(-rows // 128) * 128 * 1024,), torch.uint8, Xd.device, "scratch")
        _lib.check(lib.amdrec_ranker_x3_prefix(C.byref(params), _lib.ptr(Xd), Xd.stride(0), rows, n, _lib.ptr(x_out), 256,
                                               _lib.ptr(logits), rows, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(Xd.device)))
        for t in (x_out, logits, ws):
            t.check()
        assert np.array_equal(x_out.cpu().numpy().view(np.uint32), x0.view(np.uint32))
        assert np.array_equal(logits.cpu().numpy().view(np.uint32), l0.view(np.uint32))     # (NaN where the heads did not run)
    edge = np.r_[0:min(64, rows), max(0, rows - 64):rows]
    truth = oracle.ranker.chain_states(sd, X[edge], dtype=np.float64)[-1]
    scale = cases.logit_scale(truth)
    for ti, t in enumerate(oracle.ranker.TASKS):
        ok, e = cases.logit_close(l0[ti][edge], truth[t], "scaled", scale=scale)
        assert ok, (t, e)


@pytest.mark.parametrize("n_ads", [1, 77, 1000])              # none a multiple of the GEMM's row tile
def test_project_ads_in_guarded_buffers(ctx, n_ads):
    """amdrec_ranker_project_ads / _hidden: ``out`` guarded, the workspace exactly 4 * d_model + 256 / 4 * d_ff + 256 bytes.
    Bit-equal to the caches ``ensure_ad_cache`` builds for the same table (whose rows the logits above are computed from)."""
    m = ctx.models["f16x3"]
    table = _cu(synth.ad_features(dict(cases.ranker_case("demo", "scaled")[1]), n_ads, seed=93))
    m.ensure_ad_cache(table)
    proj, hid = m._cache_for(table), m._hidden_cache_for(table)
    assert proj is not None and hid is not None and n_ads % 16
    params, _ = m._pack(table.device)
    lib, d_ff = _lib.load(), int(params.d_ff)
    for fn, width, want in ((lib.amdrec_ranker_project_ads, m.d_model, proj), (lib.amdrec_ranker_project_ads_hidden, d_ff, hid)):
        out = guarded((n_ads, width), torch.float32, table.device, "output")
        ws = guarded((4 * width + 256,), torch.uint8, table.device, "scratch")
        _lib.check(fn(C.byref(params), _lib.ptr(table), n_ads, _lib.ptr(out), width, _lib.ptr(ws), ws.numel(),
                      _lib.stream_ptr(table.device)))
        out.check()
        ws.check()
        assert torch.equal(out, want)
    m.ensure_ad_cache(ctx.d_table)
