"""GPU: the 128-row shape of the 16-row row-owner kernel runs PH_FFN_LN split by stage over pairs of waves (wave w: stage
1 of its own and of wave w + 4's row tile; wave w + 4: stage 2 and the LayerNorm of both; csrc/rowowner16_impl.hpp
phase_ffn_ln_role_a / phase_ffn_ln_role_b).  Every output element sees the MFMAs of the unpaired phase in the same order,
so a pass of more than 16 384 rows must EQUAL, bit for bit, the same rows run in slices on the 64-row shape, which keeps
the unpaired phase.

Row counts at the pairing's edges (a workgroup = 8 tiles of 16 rows, pairs = tiles (i, i + 4), 16 384 = 128 full workgroups):
16 385 one live row, its partner tile empty; 16 400 / 16 401 the last row of tile 0 / the first of tile 1; 16 449 the first
row of tile 4 - the first pair complete, the other three with their first tile past the end; 16 512 a whole workgroup.

The hidden-cache program (layer 1's FFN from the per-ad cache) exists on the 128-row shape alone and differs from the
uncached program in its bits (tests/test_ffn1_cache_gpu.py), so it has no slice-wise 64-row twin: its PH_FFN_LN phases are
the very code the uncached comparisons pin, and it is checked here for independence of a row's result from the role
(tile i < 4 or >= 4) its tile plays and for determinism; tests/test_ffn1_cache_gpu.py holds it to float64 truth."""
import ctypes as C

import numpy as np
import pytest
import torch

from amdrec import _lib, synth
from tests import cases

pytestmark = pytest.mark.gpu

TAG_128, TAG_64 = "ranker_rowowner16_128_x3", "ranker_rowowner16_64_x3"
SLICE = 16384
EDGE_ROWS = [16385, 16400, 16401, 16449, 16512]


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_MODELS = {}


def _model(name):
    """-> (model, sd, dims); one model per architecture, shared by the tests (its packs are cached per setting)."""
    if name not in _MODELS:
        from amdrec.ranker import TransformerRanker
        if name in cases.CASES:
            user, ad, nnum, sd, _ = cases.ranker_case(name, "randn")
            args = cases.arch(name)["rk"]
        else:
            user, ad, nnum, sd = cases.surface_ranker_case(name, "randn")
            args = cases.RANKER_SURFACE[name][0]
        m = TransformerRanker(dict(user), dict(ad), nnum, **args)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        m = m.cuda().eval()
        m.x3_variant, m.x3_cs_max_rows = 16, -1            # no column-split kernel: small passes run the 64-row shape
        _MODELS[name] = (m, sd, (user, ad, nnum))
    return _MODELS[name]


_ROWS = {}


def _rows(name, rows, seed=91):
    """Dense input rows of the chain's scale (the engine rescales every row itself); one array per architecture."""
    if name not in _ROWS:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((max(EDGE_ROWS), 256)).astype(np.float32)
        X *= np.exp2(rng.integers(-3, 4, (X.shape[0], 1))).astype(np.float32)
        _ROWS[name] = _cu(X)
    return _ROWS[name][:rows]


def _prefix(m, X, n_phases, tag):
    """amdrec_ranker_x3_prefix on X -> (row state, logits) on the device; the pass must have run the kernel `tag`."""
    lib = _lib.load()
    dev = X.device
    params, tasks = m._pack(dev)
    rows = X.shape[0]
    x_out = torch.full((rows, 256), float("nan"), dtype=torch.float32, device=dev)
    logits = torch.full((len(tasks), rows), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.empty(((rows + 127) // 128) * 128 * 1024, dtype=torch.uint8, device=dev)
    _lib.profile_enable(True)
    _lib.check(lib.amdrec_ranker_x3_prefix(C.byref(params), _lib.ptr(X), X.stride(0), rows, n_phases, _lib.ptr(x_out),
                                           x_out.stride(0), _lib.ptr(logits), logits.stride(0), _lib.ptr(ws), ws.numel(),
                                           _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    rep = _lib.profile_report()
    _lib.profile_enable(False)
    assert tag in rep, (tag, list(rep))
    return x_out, logits


def _prefix_sliced(m, X, n_phases):
    parts = [_prefix(m, X[a:a + SLICE], n_phases, TAG_64) for a in range(0, X.shape[0], SLICE)]
    return torch.cat([p[0] for p in parts], dim=0), torch.cat([p[1] for p in parts], dim=1)


def _n_phases(m, fold):
    return 2 * len(m.transformer_layers) + 3 + 1


def _check_every_prefix(name, fold, rows):
    m, _, _ = _model(name)
    m.fold_first_attention = fold
    X = _rows(name, rows)
    n_total = _n_phases(m, fold)
    for n in range(1, n_total + 1):
        x1, l1 = _prefix(m, X, n, TAG_128)
        x2, l2 = _prefix_sliced(m, X, n)
        if n < n_total:
            assert bool(torch.isfinite(x1).all()) and torch.equal(x1, x2), (name, fold, rows, n, float((x1 - x2).abs().max()))
        else:
            assert bool(torch.isfinite(l1).all()) and torch.equal(l1, l2), (name, fold, rows, float((l1 - l2).abs().max()))


@pytest.mark.parametrize("rows", EDGE_ROWS)
@pytest.mark.parametrize("fold", [False, True], ids=["unfolded", "folded"])
def test_every_prefix_equals_the_unpaired_64_row_kernel(fold, rows):
    """The reference architecture (3 x (attention, FFN of 32 steps) + 3 cross + heads), every prefix of the chain."""
    _check_every_prefix("demo", fold, rows)


@pytest.mark.parametrize("name", ["x3_one_layer",        # d_ff 96: 3 steps - one full step between the single-stage ones
                                  "x3_five_layers",      # d_ff 32: 1 step - no full step at all, five paired phases
                                  "x3_param_edge"])      # d_ff 1568: 49 steps, an odd count
def test_every_prefix_equals_at_other_step_counts(name):
    _check_every_prefix(name, True, 16449)
    _check_every_prefix(name, False, 16401)


def test_rows_do_not_see_their_pair_partner():
    """A NaN row in tile 0 and an inf row in tile 5 of the last workgroup: every other row - the partner tiles 4 and 1
    included - keeps the bits of the clean run, and the poisoned rows give what the 64-row kernel gives for them."""
    m, _, _ = _model("demo")
    m.fold_first_attention = True
    n = _n_phases(m, True)
    clean = _rows("demo", 16512)
    r_nan, r_inf = 16384 + 5, 16384 + 5 * 16 + 3
    X = clean.clone()
    X[r_nan, 7] = float("nan")
    X[r_inf, 200] = float("inf")
    for n_ph in (2, 4, n):                        # behind the first paired phase, behind the second, the logits
        xc, lc = _prefix(m, clean, n_ph, TAG_128)
        xp, lp = _prefix(m, X, n_ph, TAG_128)
        xs, ls = _prefix_sliced(m, X, n_ph)
        keep = torch.ones(16512, dtype=torch.bool, device="cuda")
        keep[r_nan] = keep[r_inf] = False
        if n_ph < n:
            assert torch.equal(xp[keep], xc[keep])
            assert not bool(torch.isfinite(xp[~keep]).all(dim=1).any())
            assert np.array_equal(xp[~keep].cpu().numpy(), xs[~keep].cpu().numpy(), equal_nan=True)
        else:
            assert torch.equal(lp[:, keep], lc[:, keep]) and bool(torch.isfinite(lp[:, keep]).all())
            assert np.array_equal(lp[:, ~keep].cpu().numpy(), ls[:, ~keep].cpu().numpy(), equal_nan=True)


def test_two_runs_are_bit_identical():
    m, _, _ = _model("demo")
    m.fold_first_attention = True
    X = _rows("demo", 16449)
    n = _n_phases(m, True)
    a, b = _prefix(m, X, n, TAG_128), _prefix(m, X, n, TAG_128)
    assert torch.equal(a[1], b[1])
    a, b = _prefix(m, X, n - 1, TAG_128), _prefix(m, X, n - 1, TAG_128)
    assert torch.equal(a[0], b[0])


# ---- whole forwards on the cached gather: x0 = projection cache[ad] + U[user] ----
N_ADS = 3000


class _Gather:
    def __init__(self):
        self.m, _, (user, ad, nnum) = _model("demo")
        self.table = _cu(synth.ad_features(ad, N_ADS, seed=93))
        uc, un = synth.user_batch(user, nnum, 5, seed=94)
        self.uc, self.un = _cu(uc), _cu(un)

    def score(self, cand, users, tag):
        """score_candidates(raw) on users [0, users) -> logits [3, rows]; `tag`: the ranker kernel that must have run."""
        _lib.profile_enable(True)
        _, logits = self.m.score_candidates(self.uc[:users], self.un[:users], cand, self.table, raw=True, check_indices=True)
        torch.cuda.synchronize()
        rep = _lib.profile_report()
        _lib.profile_enable(False)
        assert tag in rep, (tag, list(rep))
        return logits.clone(), rep

    def score_one(self, cand, u, tag):
        _lib.profile_enable(True)
        _, logits = self.m.score_candidates(self.uc[u:u + 1], self.un[u:u + 1], cand[u:u + 1], self.table, raw=True)
        torch.cuda.synchronize()
        rep = _lib.profile_report()
        _lib.profile_enable(False)
        assert tag in rep, (tag, list(rep))
        return logits.clone()


@pytest.fixture(scope="module")
def gather():
    g = _Gather()
    g.m.fold_first_attention = True
    g.m.ensure_ad_cache(g.table)
    yield g
    g.m.cache_first_ffn = True


def _cand(users, k, seed):
    c = np.random.default_rng(seed).integers(0, N_ADS, (users, k))
    c[0, 0], c[-1, -1] = N_ADS - 1, 0
    return _cu(c)


@pytest.mark.parametrize("users,k", [(5, 3277), (3, 5483)])          # 16 385 and 16 449 rows
def test_forward_on_the_cached_gather_equals_the_64_row_slices(gather, users, k):
    """The uncached program on gathered rows, one pass on the 128-row shape against one 64-row pass per user: all three
    tasks' logits equal; the CTR-first pass (trunk + first head) gives the same first-task logits."""
    m = gather.m
    m.cache_first_ffn = False
    m.ensure_ad_cache(gather.table)
    cand = _cand(users, k, seed=k)
    big, _ = gather.score(cand, users, TAG_128)
    small = torch.cat([gather.score_one(cand, u, TAG_64) for u in range(users)], dim=1)
    assert big.shape == (3, users * k) and bool(torch.isfinite(big).all())
    assert torch.equal(big, small), float((big - small).abs().max())
    assert m.ctr_first_ready(gather.table, users * k, users * k)
    ctr, trunk = m.score_ctr_first(gather.uc[:users], gather.un[:users], cand, gather.table)
    assert torch.equal(ctr.reshape(-1), big[0]) and bool(torch.isfinite(trunk).all())


@pytest.mark.parametrize("users,k", [(5, 3277), (3, 5483)])
def test_hidden_cache_program_under_pairing(gather, users, k):
    """The hidden-cache program (module docstring): a row's logits do not depend on the role of its tile - the candidate
    lists rotated by 64 rows swap the roles of every tile -, two runs are equal and the CTR-first pass gives the same
    first-task logits."""
    m = gather.m
    m.cache_first_ffn = True
    m.ensure_ad_cache(gather.table)
    cand = _cand(users, k, seed=k)
    got, rep = gather.score(cand, users, TAG_128)
    full = 2.0 * users * k * 2_146_496
    assert rep[TAG_128]["flops"] == full - 2.0 * users * k * 256 * 1024            # really the hidden-cache program
    again, _ = gather.score(cand, users, TAG_128)
    assert torch.equal(got, again)
    # the same (user, ad) rows 64 positions on: user u's list rotated inside its own k rows (k > 128)
    rot = torch.roll(cand, 64, dims=1)
    moved, _ = gather.score(rot, users, TAG_128)
    back = torch.roll(moved.view(3, users, k), -64, dims=2).reshape(3, -1)
    assert torch.equal(back, got)
    assert m.ctr_first_ready(gather.table, users * k, users * k)
    ctr, _ = m.score_ctr_first(gather.uc[:users], gather.un[:users], cand, gather.table)
    assert torch.equal(ctr.reshape(-1), got[0])
