"""GPU: the ranker engines on weights whose magnitudes are spread INSIDE a matrix (tests/reparam.py).

Every other ranker test draws its weights i.i.d. from one normal distribution.  The fp16x3 engine has one power-of-two scale
per weight matrix and one hidden bound per row, so its accuracy depends on how magnitudes are distributed inside a matrix:
tests/test_x3_model_cpu.py shows on the CPU what the arithmetic implies, this file holds the kernels to the suite's own rules
on such weights.

* EXACT families (a) - (d): re-parametrisations by powers of two that a plain fp32 evaluation cannot see, so the float64
  truth and the numpy fp32 yardstick are the BASE model's, computed once per row count.  The f16x3 engine runs every prefix
  of the chain (amdrec_ranker_x3_prefix, both kernels, the row counts that reach the column-split kernel, the 64-row and the
  128-row workgroups) under the per-phase rules of tests/test_x3_gpu.py and the logit rule of cases.logit_close("scaled"),
  at spreads of +-3, +-6 and +-10 binades.  One ``score_candidates`` pass per spread runs the cached first-FFN program.
* The fp32 and bf16x6 engines at +-10: logits EQUAL to the base model's - a power of two commutes with fp32 products and
  sums, with the bf16 truncation split and with the float64-then-round folds of the host.
* STRUCTURED families (other networks; own float64 truth): logits of a whole forward within 4x the fp32 engine's error
  (the rule of tests/test_models_gpu.py), every prefix finite.
Every achieved ratio is recorded through the ``accuracy`` fixture."""
import numpy as np
import pytest
import torch

import oracle
from amdrec import _lib, synth
from tests import cases, reparam
from tests import test_ffn1_cache_gpu as hc
from tests import test_x3_gpu as x3t

pytestmark = pytest.mark.gpu

ROWS = [53,                       # the column-split kernel (variant 16): three full 16-row workgroups and a ragged one
        4096 + 64 + 13,           # 64-row workgroups, ragged tail
        16384 + 128 + 45]         # the 128-row shape, ragged tail
SPREADS = (3, 6, 10)
PHASES = [f"L{l}.{k}" for l in range(3) for k in ("attn_ln1", "ffn_ln2")] + [f"cross{c}" for c in range(3)] + ["heads"]
N_ADS, USERS, CAND = 2000, 5, 3277          # 16 385 rows: the cached first-FFN program of the 128-row shape


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _model(base, sd, variant=16, engine="f16x3"):
    from amdrec.ranker import TransformerRanker
    m = TransformerRanker(dict(base.user), dict(base.ad), base.nnum)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.x3_variant, m.gemm_engine = variant, engine
    return m.cuda().eval()


class _Base:
    """The base model ("demo", "scaled") and everything the exact families share: inputs, float64 truth, the numpy fp32
    yardstick and the other engines' logits, each computed once."""

    def __init__(self):
        self.user, self.ad, self.nnum, self.sd, _ = cases.ranker_case("demo", "scaled")
        self._chain, self._feats, self._engine, self._one = {}, {}, {}, (None, None)
        self._table = None

    def feats(self, rows):
        if rows not in self._feats:
            uc, un = synth.user_batch(self.user, self.nnum, rows, seed=41)
            self._feats[rows] = (uc, synth.ad_features(self.ad, rows, seed=42), un)
        return self._feats[rows]

    def chain(self, rows):
        """-> (X on the device, float64 states, numpy fp32 states) of the base model."""
        if rows not in self._chain:
            X = x3t._projected_rows(self.sd, (self.user, self.ad, self.nnum), rows, seed=41)
            self._chain[rows] = (_cu(X), oracle.ranker.chain_states(self.sd, X, dtype=np.float64),
                                 oracle.ranker.chain_states(self.sd, X, dtype=np.float32))
        return self._chain[rows]

    def forward(self, m, rows):
        uc, ac, un = self.feats(rows)
        out = m(_cu(uc), _cu(ac), _cu(un))
        torch.cuda.synchronize()
        return {t: v.cpu().numpy() for t, v in out.items()}

    def engine_logits(self, engine, rows):
        """The base model's logits on ``engine`` (a whole forward)."""
        if (engine, rows) not in self._engine:
            self._engine[engine, rows] = self.forward(_model(self, self.sd, engine=engine), rows)
        return self._engine[engine, rows]

    def model(self, key, build):
        """One model at a time stays packed on the device (the parameters below are ordered so that it is reused)."""
        if self._one[0] != key:
            self._one = (None, None)
            self._one = (key, build())
        return self._one[1]

    def table(self):
        """The candidate pass: users, a 2 000-ad table, candidates; float64 truth of every (user, ad) pair and the base
        model's fp32-engine logits for the candidates."""
        if self._table is None:
            uc, un = synth.user_batch(self.user, self.nnum, USERS, seed=81)
            ads = synth.ad_features(self.ad, N_ADS, seed=82)
            cand = np.random.default_rng(83).integers(0, N_ADS, (USERS, CAND))
            cand[0, 0], cand[0, 1], cand[-1, -1], cand[-1, -2] = 0, N_ADS - 1, N_ADS - 1, 0
            t64 = oracle.ranker.forward(self.sd, np.repeat(uc, N_ADS, axis=0), np.tile(ads, (USERS, 1)),
                                        np.repeat(un, N_ADS, axis=0), dtype=np.float64)
            rows = np.repeat(np.arange(USERS), CAND)
            truth = {t: v.reshape(USERS, N_ADS)[rows, cand.reshape(-1)] for t, v in t64.items()}
            self._table = dict(uc=_cu(uc), un=_cu(un), ads=_cu(ads), cand=_cu(cand), truth=truth)
            self._table["fp32"], _ = self.score(_model(self, self.sd, engine="fp32"))
        return self._table

    def score(self, m):
        t = self._table
        m.ensure_ad_cache(t["ads"])
        _lib.profile_enable(True)
        out = m.score_candidates(t["uc"], t["un"], t["cand"], t["ads"], check_indices=True)
        torch.cuda.synchronize()
        rep = _lib.profile_report()
        _lib.profile_enable(False)
        return {k: v.cpu().numpy() for k, v in out.items()}, rep


@pytest.fixture(scope="module")
def base():
    yield _Base()


def _ratios(x, ref, f32):
    scale = np.abs(ref).max(axis=1, keepdims=True)
    d, d32 = (x - ref) / scale, (f32 - ref) / scale
    return (float(np.abs(d).max()), float(np.abs(d32).max()), float(np.sqrt(np.mean(d * d))), float(np.sqrt(np.mean(d32 * d32))))


def _check_every_prefix(m, chain, case, engine, accuracy, rules):
    """tests/test_x3_gpu.py ``_check_every_prefix`` against a given truth.  ``rules``: its per-phase bounds (rms <= 4x,
    max <= 8x the numpy fp32 evaluation's error, both against float64) and cases.logit_close("scaled") on the logits;
    otherwise finite outputs alone.  Either way every ratio is recorded."""
    X, truth, f32 = chain
    assert m.gemm_engine_for(X.shape[0]) == "f16x3" and len(truth) == len(PHASES)
    for n in range(1, len(PHASES) + 1):
        x, logits = x3t._prefix(m, X, n)
        name = PHASES[n - 1]
        if n < len(PHASES):
            err, err32, rms, rms32 = _ratios(x, truth[n - 1], f32[n - 1])
            r_max, r_rms = err / max(err32, 1e-30), rms / max(rms32, 1e-30)      # (constant rows: the fp32 yardstick can be exact)
            accuracy(f"{case}/{name}", engine, r_max, rms_ratio=r_rms, rel_err_vs_float64=err, numpy_fp32_rel_err_vs_float64=err32)
            print(f"{case}/{name} {engine}: max ratio {r_max:.2f} rms ratio {r_rms:.2f}")
            assert np.isfinite(x).all(), name
            if rules:
                assert rms <= 4 * rms32, (name, rms, rms32)
                assert err <= 8 * err32, (name, err, err32)
        else:
            assert np.isfinite(logits).all()
            scale = cases.logit_scale(truth[-1])
            for ti, t in enumerate(oracle.ranker.TASKS):
                ok, e = cases.logit_close(logits[ti], truth[-1][t], "scaled", scale=scale)
                accuracy(f"{case}/heads/{t}", engine, e)
                print(f"{case}/heads/{t} {engine}: err / bound {e:.3f}")
                assert ok or not rules, (t, e)


# (family, spread, kernel) outermost, the row counts innermost: one packing serves its three row counts
EXACT_CASES = [(f, e, v, r) for f in reparam.EXACT for e in SPREADS for v in (16, 32) for r in ROWS]


@pytest.mark.parametrize("family,e,variant,rows", EXACT_CASES)
def test_exact_family_on_f16x3_meets_the_per_phase_rules(base, family, e, variant, rows, accuracy):
    """Spreads of +-3, +-6 and +-10 binades between the hidden units of one layer (or between the tasks under one shared
    scale), every prefix of the chain, on every kernel shape: the rules of tests/test_x3_gpu.py, unchanged.  Without the
    per-unit rebalancing of the packing (weights.x3_rebalance) the FFN and heads phases miss them from about +-8 on."""
    m = base.model((family, e, variant), lambda: _model(base, reparam.exact(base.sd, family, e), variant))
    _check_every_prefix(m, base.chain(rows), f"x3_reparam/{family}_e{e}/rows{rows}", f"f16x3/{variant}", accuracy, rules=True)


@pytest.mark.parametrize("family", reparam.EXACT)
@pytest.mark.parametrize("e", SPREADS)
def test_exact_family_through_the_cached_first_ffn_program(base, family, e, accuracy):
    """5 users x 3 277 candidates on a 2 000-ad table: the 128-row shape with layer 1's FFN stage 1 from the hidden cache
    (P, Q and c carry the units' factors of the stream's W_2).  cases.logit_close("scaled") against the base model's float64
    truth, and the rule every engine is held to: within 4x the fp32 engine's error."""
    t = base.table()
    m = base.model((family, e, "cand"), lambda: _model(base, reparam.exact(base.sd, family, e)))
    got, rep = base.score(m)
    flops, _, cached = hc._cached_flops(rep, USERS * CAND)
    assert hc.TAG in rep and flops == cached and m._hidden_cache_for(t["ads"]) is not None
    scale = cases.logit_scale(t["truth"])
    err = lambda o: max(float(np.abs(o[k].astype(np.float64) - t["truth"][k]).max()) for k in o)      # noqa: E731
    e_hc, e_fp32 = err(got), err(t["fp32"])
    accuracy(f"x3_reparam/{family}_e{e}/cached_ffn1/vs_fp32_engine", "f16x3/16", e_hc / max(e_fp32, 1e-30), err=e_hc, fp32_engine_err=e_fp32)
    print(f"{family} e{e} cached: |err| {e_hc:.3e}, fp32 engine {e_fp32:.3e}")
    for k in got:
        ok, r = cases.logit_close(got[k], t["truth"][k], "scaled", scale=scale)
        accuracy(f"x3_reparam/{family}_e{e}/cached_ffn1/{k}", "f16x3/16", r)
        assert np.isfinite(got[k]).all() and ok, (k, r)
    assert e_hc <= 4.0 * e_fp32 + 1e-7 * max(1.0, scale), (e_hc, e_fp32)


@pytest.mark.parametrize("family", reparam.EXACT)
@pytest.mark.parametrize("engine,rows", [("fp32", 53), ("fp32", 8192 + 77), ("bf16x6", 8192 + 77)])
def test_exact_family_is_invisible_to_the_fp32_and_bf16x6_engines(base, engine, rows, family):
    """+-10 binades: logits EQUAL to the base model's.  Times 2^k commutes with every fp32 product and sum of the tile
    GEMMs (their summation order depends on the shapes alone), with the bf16 truncation split (it cuts mantissa bits) and
    with the float64-then-round folds of the host; relu(a t) == a relu(t)."""
    m = _model(base, reparam.exact(base.sd, family, 10), engine=engine)
    assert m.gemm_engine_for(rows) == engine
    ref, got = base.engine_logits(engine, rows), base.forward(m, rows)
    for t in ref:
        assert np.isfinite(got[t]).all() and np.array_equal(ref[t], got[t]), (t, float(np.abs(ref[t] - got[t]).max()))


STRUCT_ROWS = ROWS[:2]


class _Struct:
    def __init__(self, base, family):
        self.sd = reparam.STRUCTURED[family](base.sd)
        self.chain, self.truth, self.fp32 = {}, {}, {}
        fp32 = _model(base, self.sd, engine="fp32")
        for rows in STRUCT_ROWS:
            X = x3t._projected_rows(self.sd, (base.user, base.ad, base.nnum), rows, seed=41)
            self.chain[rows] = (_cu(X), oracle.ranker.chain_states(self.sd, X, dtype=np.float64),
                                oracle.ranker.chain_states(self.sd, X, dtype=np.float32))
            self.truth[rows] = oracle.ranker.forward(self.sd, *base.feats(rows), dtype=np.float64)
            self.fp32[rows] = base.forward(fp32, rows)


@pytest.mark.parametrize("variant", [16, 32])
@pytest.mark.parametrize("family", list(reparam.STRUCTURED))
def test_structured_family_within_4x_of_the_fp32_engine(base, family, variant, accuracy):
    """Other networks: massive features, outlier units, heavy tails, one-signed weights, rows that reach the hidden bound
    itself, big biases, dead units, sparse and low-rank W_1, rows with a large mean.  Logits of a whole forward within 4x
    the fp32 engine's error against float64 (+ 1e-7 max(1, scale)), every prefix finite; the per-phase ratios are recorded."""
    s = base.model(("struct", family), lambda: _Struct(base, family))
    m = _model(base, s.sd, variant)
    for rows in STRUCT_ROWS:
        case = f"x3_reparam/{family}/rows{rows}"
        _check_every_prefix(m, s.chain[rows], case, f"f16x3/{variant}", accuracy, rules=False)
        got, truth = base.forward(m, rows), s.truth[rows]
        scale = cases.logit_scale(truth)
        err = lambda o: max(float(np.abs(o[t].astype(np.float64) - truth[t]).max()) for t in o)      # noqa: E731
        e_x3, e_fp32 = err(got), err(s.fp32[rows])
        accuracy(f"{case}/forward_vs_fp32_engine", f"f16x3/{variant}", e_x3 / max(e_fp32, 1e-30), err=e_x3, fp32_engine_err=e_fp32,
                 logit_scale=scale)
        print(f"{case} f16x3/{variant}: |err| {e_x3:.3e}, fp32 engine {e_fp32:.3e}, scale {scale:.3g}")
        assert all(np.isfinite(v).all() for v in got.values())
        assert e_x3 <= 4.0 * e_fp32 + 1e-7 * max(1.0, scale), (rows, e_x3, e_fp32, scale)
