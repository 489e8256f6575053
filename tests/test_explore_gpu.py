"""Exploration on the GPU.  ``amdrec_select_topk_sampled`` is compared with the numpy oracle of amdrec.explore - never with
another new kernel: ids and slots exactly, ``scores`` bit for bit with the plain selection's per-slot probabilities, the
propensities within 2 float32 ulps (both sides form them in float64 and round once).  The device's float64 ``log`` may differ
from numpy's in the last bit, so every comparison first asserts, on the CPU, that the oracle's float64 keys of the candidates
the sampled walk looks at (up to the ``top_k + 1``-th accepted one) are pairwise at least 2^-18 apart: the order then cannot
depend on that bit.  Users with temperature 0 and calls with ``greedy == top_k`` are the plain / capped selection bit for bit.
Then the draw's frequencies on the device, determinism, and the serving pipeline on Flat and IVF (both head modes, the cap,
exclusions, injections, the reference API, the captured graph).  Without the new arguments nothing runs that did not run
before."""
import math

import numpy as np
import pytest
import torch

from amdrec import _lib, explore as ex
from tests import group_cap_oracle as go
from tests.guarded import guarded
from tests.test_auction_gpu import _bits, _dev, _positions, _prob_by_slot

pytestmark = pytest.mark.gpu

F32 = np.float32
N_ROWS = 64
K_CS = [1, 7, 64, 129, 512, 513, 2048]                                   # the sorts' boundaries: 128 (network / runs), 512, 1024
TOP_KS = [1, 10, 33, 128]
N_USERS = 5
TEMPS = np.array([0.0, 0.25, 1.0, 4.0, np.inf], dtype=F32)
MIN_GAP = 2.0 ** -18
# per k_c: the base of the users' seeds (user u draws with base + u), picked so that the gap precondition holds for every
# top_k, cap and greedy of the grid below
SEED_BASE = {1: 1000, 7: 1000, 64: 1000, 129: 1000, 512: 1300, 513: 1100, 2048: 1000}


def inputs(n_users, k_c, n_tasks, seed, n_rows=N_ROWS):
    """Gaussian logits [n_tasks, n_users * k_c] with 8 % NaN and a few +-inf, positions with 10 % holes (some beyond ``n_rows``:
    no group) and the last user without a candidate, ids unique within a user, group keys."""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((n_tasks, n_users * k_c)).astype(F32)
    logits[rng.random(logits.shape) < 0.08] = np.nan
    logits[rng.random(logits.shape) < 0.02] = np.inf
    logits[rng.random(logits.shape) < 0.02] = -np.inf
    pos = rng.integers(0, n_rows + 8, size=(n_users, k_c)).astype(np.int64)
    pos[rng.random(pos.shape) < 0.1] = -1
    pos[n_users - 1] = -1
    ids = np.stack([rng.permutation(4 * k_c + 16)[:k_c] for _ in range(n_users)]).astype(np.int64) * 7 + 3
    group_of = rng.choice(np.array([-1, 3, 1 << 33, 7], dtype=np.int64), size=n_rows)
    return logits, ids, pos, group_of


def _sampled(logits, ids, pos, temp, seeds, top_k, greedy=0, group_of=None, cap=0, n_group_rows=None, rank_task=0, slots=True):
    """The entry on device tensors, every output in a guarded exact-size buffer -> dict of numpy arrays."""
    n_users, k_c = ids.shape
    n_tasks = logits.shape[0]
    out = dict(ids=guarded((n_users, top_k), torch.int64, "cuda", "output"),
               scores=guarded((n_tasks, n_users, top_k), torch.float32, "cuda", "output"),
               slots=guarded((n_users, top_k), torch.int32, "cuda", "output") if slots else None,
               propensities=guarded((n_users, top_k), torch.float32, "cuda", "output"))
    n_group_rows = (0 if group_of is None else group_of.shape[0]) if n_group_rows is None else n_group_rows
    assert logits.is_contiguous()                                          # (the stride of a single row is anybody's guess)
    _lib.check(_lib.load().amdrec_select_topk_sampled(
        _lib.ptr(logits), logits.shape[1], n_tasks, rank_task, _lib.ptr(ids), _lib.ptr(pos), n_users, k_c, top_k,
        _lib.ptr(out["ids"]), _lib.ptr(out["scores"]), _lib.ptr(out["slots"]), _lib.ptr(group_of), n_group_rows, cap,
        _lib.ptr(temp), _lib.ptr(seeds), greedy, _lib.ptr(out["propensities"]), _lib.stream_ptr("cuda")))
    res = {}
    for k, t in out.items():
        if t is not None:
            t.check()
            res[k] = t.cpu().numpy()
    return res


def _plain(logits, ids, pos, top_k, group_of=None, cap=0, rank_task=0):
    """amdrec_select_topk / _capped, which predate the feature -> (ids, scores, slots) numpy."""
    n_users, k_c = ids.shape
    n_tasks = logits.shape[0]
    out_ids = torch.empty((n_users, top_k), dtype=torch.int64, device="cuda")
    sc = torch.empty((n_tasks, n_users, top_k), dtype=torch.float32, device="cuda")
    sl = torch.empty((n_users, top_k), dtype=torch.int32, device="cuda")
    lib = _lib.load()
    head = (_lib.ptr(logits), logits.shape[1], n_tasks, rank_task, _lib.ptr(ids), _lib.ptr(pos), n_users, k_c, top_k,
            _lib.ptr(out_ids), _lib.ptr(sc), _lib.ptr(sl))
    if cap:
        _lib.check(lib.amdrec_select_topk_capped(*head, _lib.ptr(group_of), group_of.shape[0], cap, _lib.stream_ptr("cuda")))
    else:
        _lib.check(lib.amdrec_select_topk(*head, _lib.stream_ptr("cuda")))
    return out_ids.cpu().numpy(), sc.cpu().numpy(), sl.cpu().numpy()


def assert_keys_apart(want, what=""):
    """The precondition: per user, the float64 keys of the finite-logit candidates that the sampled walk looked at, up to and
    including the (top_k + 1)-th accepted candidate, are pairwise at least 2^-18 apart."""
    for u, visited in enumerate(want["visited"]):
        k = np.sort(want["keys"][u, visited])
        k = k[~np.isnan(k)]
        if len(k) > 1:
            gap = float(np.diff(k).min())
            assert gap >= MIN_GAP, f"user {u}: two perturbed keys {gap} apart {what} - pick another seed"


def assert_within_2_ulps(got, want, what=""):
    """float32 arrays, both >= 0: at most two rounding steps apart (a denormal step is one step of the bit pattern too)."""
    g, w = _bits(got).astype(np.int64), _bits(want).astype(np.int64)
    assert (g >= 0).all() and (w >= 0).all() and not np.isnan(got).any(), what
    bad = np.abs(g - w) > 2
    assert not bad.any(), (what, np.asarray(got)[bad][:5], np.asarray(want)[bad][:5])


def assert_is_oracle(got, want, table, what=""):
    assert np.array_equal(got["ids"], want["ids"]), f"ids {what}"
    if "slots" in got:
        assert np.array_equal(got["slots"], want["slots"]), f"slots {what}"
    assert np.array_equal(_bits(got["scores"]), _bits(go.scores_at(table, want["slots"]))), f"scores {what}"
    assert_within_2_ulps(got["propensities"], want["propensities"], f"propensities {what}")
    assert ((got["propensities"] == 0) == (want["slots"] < 0)).all() or (want["propensities"] == 0).any(), what


@pytest.mark.parametrize("n_tasks", [1, 3])
@pytest.mark.parametrize("k_c", K_CS)
def test_the_entry_is_the_oracle_across_shapes_caps_and_prefixes(k_c, n_tasks):
    logits_np, ids_np, pos_np, groups_np = inputs(N_USERS, k_c, n_tasks, 100 * k_c + n_tasks)
    rank_task = n_tasks - 1
    seeds_np = (SEED_BASE[k_c] + np.arange(N_USERS)).astype(np.int64)
    logits, ids, pos, group_of, temp, seeds = (_dev(a) for a in (logits_np, ids_np, pos_np, groups_np, TEMPS, seeds_np))
    z = logits_np[rank_task].reshape(N_USERS, k_c)
    table = _prob_by_slot(logits, N_USERS, k_c)
    moved = forced = 0
    for top_k in TOP_KS:
        for cap in (0, 1, 2):
            old = _plain(logits, ids, pos, top_k, group_of, cap, rank_task)
            for greedy in sorted({0, 1, top_k}):
                what = f"k_c {k_c} tasks {n_tasks} top_k {top_k} cap {cap} greedy {greedy}"
                want = ex.explore_oracle(z, ids_np, pos_np, TEMPS, seeds_np, top_k, greedy, groups_np, N_ROWS, cap)
                assert_keys_apart(want, what)
                got = _sampled(logits, ids, pos, temp, seeds, top_k, greedy, group_of if cap else None, cap, rank_task=rank_task)
                assert_is_oracle(got, want, table, what)
                # temperature 0, and every user under greedy == top_k: the plain (capped) selection bit for bit, propensity 1.0
                for u in range(N_USERS) if greedy == top_k else (0,):
                    assert np.array_equal(got["ids"][u], old[0][u]) and np.array_equal(got["slots"][u], old[2][u]), what
                    assert np.array_equal(_bits(got["scores"][:, u]), _bits(old[1][:, u])), what
                    assert (got["propensities"][u] == np.where(old[2][u] >= 0, 1.0, 0.0)).all(), what
                assert (got["propensities"][:, :greedy][got["slots"][:, :greedy] >= 0] == 1.0).all()
                assert (got["ids"][N_USERS - 1] == -1).all() and (_bits(got["propensities"][N_USERS - 1]) == 0).all()
                if greedy < top_k:
                    moved += int(not np.array_equal(got["slots"], old[2]))
                    won = got["slots"] >= 0
                    forced += int(((got["propensities"] < 1.0) & won).any())
    # the cases do exercise the rule (one candidate per user leaves nothing to draw)
    assert k_c < 7 or (moved and forced), (moved, forced)


@pytest.mark.parametrize("k_c,top_k", [(64, 10), (500, 10), (700, 40)])
def test_positions_beyond_the_group_array_no_slots_output_and_an_infinite_temperature(k_c, top_k):
    n_users, n_rows = 5, 50
    logits_np, ids_np, pos_np, _ = inputs(n_users, k_c, 2, 5, n_rows=2 * n_rows)
    pos_np[n_users - 1] = pos_np[0]                                        # (here every user has candidates)
    rng = np.random.default_rng(6)
    groups_np = rng.choice(np.array([-1, 0, 9], dtype=np.int64), size=n_rows)
    group_of = guarded((n_rows,), torch.int64, "cuda", "scratch")
    group_of.copy_(_dev(groups_np))
    temp_np = np.array([np.inf, 1.0, np.inf, 0.5, np.inf], dtype=F32)
    seeds_np = np.array([7, -1, np.iinfo(np.int64).min, 1 << 40, 12345], dtype=np.int64)       # bit patterns, the top bit included
    logits, ids, pos, temp, seeds = (_dev(a) for a in (logits_np, ids_np, pos_np, temp_np, seeds_np))
    z = logits_np[0].reshape(n_users, k_c)
    table = _prob_by_slot(logits, n_users, k_c)
    for cap in (1, 2):
        want = ex.explore_oracle(z, ids_np, pos_np, temp_np, seeds_np, top_k, 2, groups_np, n_rows, cap)
        assert_keys_apart(want, f"cap {cap}")
        got = _sampled(logits, ids, pos, temp, seeds, top_k, 2, group_of, cap, n_group_rows=n_rows)
        assert_is_oracle(got, want, table, f"cap {cap}")
        beyond = pos_np[np.arange(n_users)[:, None], np.maximum(want["slots"], 0)] >= n_rows
        assert (beyond & (want["slots"] >= 0)).any()                                         # such candidates did win
    group_of.check()
    want = ex.explore_oracle(z, ids_np, pos_np, temp_np, seeds_np, top_k)
    assert_keys_apart(want)
    got = _sampled(logits, ids, pos, temp, seeds, top_k, slots=False)
    assert "slots" not in got
    assert_is_oracle(got, want, table, "no groups, no slots")
    # a uniform draw: the r-th finite pick has propensity 1 / (finite candidates left)
    for u in (0, 2, 4):
        fin = np.isfinite(z[u]) & (pos_np[u] >= 0)
        left = int(fin.sum())
        for r, s in enumerate(want["slots"][u]):
            if s >= 0 and fin[s]:
                assert got["propensities"][u, r] == F32(1.0 / left)
                left -= 1
        assert left < int(fin.sum())


def _frequency_inputs(n, z):
    k_c = len(z)
    logits = _dev(np.tile(np.asarray(z, dtype=F32), n)[None])
    ids = _dev(np.tile(np.array([11, 5, 900, 42], dtype=np.int64)[:k_c], (n, 1)))
    pos = _dev(np.tile(np.arange(k_c, dtype=np.int64), (n, 1)))
    seeds = _dev(np.arange(n, dtype=np.int64) * 3 + 17)
    return logits, ids, pos, seeds


def test_first_pick_frequencies_on_the_device_are_the_softmax_and_the_cap_renormalises_the_second_pick():
    n, T = 4096, F32(1.5)
    z = np.array([0.0, 1.0, -0.5, 2.0], dtype=F32)
    logits, ids, pos, seeds = _frequency_inputs(n, z)
    temp = _dev(np.full(n, T, dtype=F32))
    x = z.astype(np.float64) / np.float64(T)
    w = np.exp(x - x.max())
    got = _sampled(logits, ids, pos, temp, seeds, 2)
    for i in range(4):
        p = w[i] / w.sum()
        count = int((got["slots"][:, 0] == i).sum())
        assert abs(count - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (i, count, n * p)
        assert_within_2_ulps(got["propensities"][got["slots"][:, 0] == i, 0], F32(p))
    # cap 1, candidates 0 and 1 in one group: after either of them the other is out, and the second pick is drawn from what
    # has room, with the renormalised probabilities
    group_of = _dev(np.array([5, 5, -1, -1], dtype=np.int64))
    got = _sampled(logits, ids, pos, temp, seeds, 2, 0, group_of, 1)
    cells = 0
    for first in range(4):
        rows = got["slots"][:, 0] == first
        room = [i for i in range(4) if i != first and not (first in (0, 1) and i in (0, 1))]
        assert set(got["slots"][rows, 1].tolist()) <= set(room)
        for i in room:
            p = w[i] / w[room].sum()
            trials, count = int(rows.sum()), int((got["slots"][rows, 1] == i).sum())
            assert abs(count - trials * p) <= 5 * math.sqrt(trials * p * (1 - p)), (first, i, count, trials * p)
            assert_within_2_ulps(got["propensities"][rows & (got["slots"][:, 1] == i), 1], F32(p))
            cells += 1
    assert cells == 2 + 2 + 3 + 3


@pytest.mark.parametrize("k_c,top_k,cap", [(40, 6, 0), (500, 10, 2), (1500, 33, 0)])
def test_the_draw_is_a_function_of_seed_and_ad_id_alone(k_c, top_k, cap):
    n_users = 6
    rng = np.random.default_rng(k_c)
    logits_np = rng.standard_normal((1, n_users * k_c)).astype(F32)
    pos_np = rng.integers(0, N_ROWS, size=(n_users, k_c)).astype(np.int64)
    ids_np = np.stack([rng.permutation(3 * k_c)[:k_c] for _ in range(n_users)]).astype(np.int64)
    groups_np = rng.integers(0, 30, size=N_ROWS).astype(np.int64)
    seeds_np = rng.integers(-(1 << 62), 1 << 62, size=n_users).astype(np.int64)
    temp = _dev(np.full(n_users, 1.0, dtype=F32))
    group_of = _dev(groups_np) if cap else None
    logits, ids, pos = _dev(logits_np), _dev(ids_np), _dev(pos_np)
    a = _sampled(logits, ids, pos, temp, _dev(seeds_np), top_k, 1, group_of, cap)
    b = _sampled(logits, ids, pos, temp, _dev(seeds_np), top_k, 1, group_of, cap)
    for k in a:                                                           # the same seeds twice: identical output
        assert np.array_equal(a[k].view(np.int32) if a[k].dtype == F32 else a[k], b[k].view(np.int32) if b[k].dtype == F32 else b[k])
    other = seeds_np.copy()
    other[2] += 1
    c = _sampled(logits, ids, pos, temp, _dev(other), top_k, 1, group_of, cap)
    rest = [u for u in range(n_users) if u != 2]
    assert np.array_equal(c["ids"][rest], a["ids"][rest]) and np.array_equal(_bits(c["propensities"][rest]), _bits(a["propensities"][rest]))
    assert not np.array_equal(c["ids"][2], a["ids"][2])                   # one user's seed changes that user - and only it
    # permuting a user's candidate slots changes no winner id: the noise is keyed on the ad id (the oracle's keys are apart,
    # so no float32 tie is resolved by slot; under the cap the groups travel with their candidates)
    want = ex.explore_oracle(logits_np.reshape(n_users, k_c), ids_np, pos_np, np.full(n_users, 1.0, dtype=F32), seeds_np, top_k, 1,
                             groups_np, N_ROWS, cap)
    assert_keys_apart(want)
    perm = np.stack([rng.permutation(k_c) for _ in range(n_users)])
    rows = np.arange(n_users)[:, None]
    d = _sampled(_dev(logits_np.reshape(n_users, k_c)[rows, perm].reshape(1, -1)), _dev(ids_np[rows, perm]), _dev(pos_np[rows, perm]),
                 temp, _dev(seeds_np), top_k, 1, group_of, cap)
    assert np.array_equal(d["ids"], a["ids"])
    assert_within_2_ulps(d["propensities"], a["propensities"])            # (the sums run over another slot order)
    assert np.array_equal(perm[rows, np.maximum(d["slots"], 0)][d["slots"] >= 0], a["slots"][a["slots"] >= 0])


# ---- the serving pipeline ------------------------------------------------------------------------------------------------
TOP_K, K1 = 5, 64


def _pipeline():
    from tests.test_value_gpu import KINDS, _clone, _rec, _users
    return KINDS, _clone, _rec, _users


def _check_call(out, idx, temp_np, seeds_np, groups, top_k, cap, greedy):
    """ad_ids / scores / propensities of one recommend_device result against the oracle over that call's own logits, candidate
    ids and positions."""
    pos = _positions(out, idx)
    B, k1 = pos.shape
    logits = out["logits"]
    row = list(out["logit_tasks"]).index("ctr")
    z = logits[row].cpu().numpy().reshape(B, k1)
    want = ex.explore_oracle(z, out["candidate_ids"].cpu().numpy(), pos, temp_np, seeds_np, top_k, greedy, groups, len(groups), cap)
    assert_keys_apart(want)
    assert np.array_equal(out["ad_ids"].cpu().numpy(), want["ids"])
    if logits.shape[0] == len(out["tasks"]):
        table = _prob_by_slot(logits, B, k1)
        assert np.array_equal(_bits(out["scores"]), _bits(go.scores_at(table, want["slots"])))
    assert out["propensities"].shape == (B, top_k) and out["propensities"].dtype == torch.float32
    assert_within_2_ulps(out["propensities"].cpu().numpy(), want["propensities"])
    return want


def _same(a, b, keys=("ad_ids", "scores", "propensities")):
    return all(np.array_equal(a[k].cpu().numpy().view(np.int32), b[k].cpu().numpy().view(np.int32)) for k in keys)


@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_pipeline_draws_by_the_rule_in_both_head_modes_under_caps_exclusions_and_injections(kind):
    KINDS, _clone, _rec, _users = _pipeline()
    rec, _, groups = _rec(kind)
    rec_cf, _, _ = _rec(kind, heads="ctr_first")
    rec_cf.faiss_index = idx = rec.faiss_index
    B = 5
    uc, un = _users(B)
    plain = _clone(rec.recommend_device(uc, un, TOP_K, K1))
    assert "propensities" not in plain
    temps = np.array([0.0, 0.25, 1.0, 4.0, np.inf], dtype=F32)
    seed_t = np.array([3, -9, 1 << 50, 77, 0], dtype=np.int64)
    excl = plain["ad_ids"][:, :2].contiguous()                            # each user's two best ads must not be shown ...
    incl = plain["candidate_ids"][:, -1:].contiguous().roll(1, 0)         # ... and another user's last candidate must be ranked
    moved = 0
    for kw in (dict(), dict(max_per_group=1), dict(exclude_ad_ids=excl), dict(include_ad_ids=incl, max_per_group=2)):
        for g in (0, 2):
            for e, s, t_np, s_np in ((1.5, 41, np.full(B, 1.5, dtype=F32), 41 + np.arange(B)), (_dev(temps), _dev(seed_t), temps, seed_t)):
                o = _clone(rec.recommend_device(uc, un, TOP_K, K1, explore=e, explore_seed=s, explore_from=g, **kw))
                _check_call(o, idx, t_np, s_np, groups, TOP_K, kw.get("max_per_group") or 0, g)
                cf = _clone(rec_cf.recommend_device(uc, un, TOP_K, K1, explore=e, explore_seed=s, explore_from=g, **kw))
                assert _same(o, cf)                                       # bit-identical between the head modes
                if rec_cf.heads_mode_effective()[0] == "ctr_first":
                    assert cf["logit_tasks"] == ("ctr",)
                    _check_call(cf, idx, t_np, s_np, groups, TOP_K, kw.get("max_per_group") or 0, g)
                if "exclude_ad_ids" in kw:
                    assert not (o["ad_ids"][:, :, None] == excl[:, None, :]).any()
                if not kw:
                    assert torch.equal(o["candidate_ids"], plain["candidate_ids"])
                    assert torch.equal(o["ad_ids"][:, :g], plain["ad_ids"][:, :g])
                    moved += int(not torch.equal(o["ad_ids"], plain["ad_ids"]))
    assert moved                                                         # the draw did change an answer
    # a call without the arguments returns what it returned before and launches what it launched before
    _lib.profile_enable(True)
    try:
        again = rec.recommend_device(uc, un, TOP_K, K1)
        assert not [t for t in _lib.profile_report() if "sampled" in t]
        _lib.profile_enable(True)
        rec.recommend_device(uc, un, TOP_K, K1, explore=1.0, explore_seed=1, max_per_group=2)
        rep = _lib.profile_report()
        assert rep["select_topk_sampled"]["launches"] == 1 and "select_topk_capped" not in rep
    finally:
        _lib.profile_enable(False)
    assert torch.equal(again["ad_ids"], plain["ad_ids"]) and torch.equal(again["scores"], plain["scores"])
    assert "propensities" not in again
    pos = _positions(again, idx)
    z = again["logits"][list(again["logit_tasks"]).index("ctr")].cpu().numpy().reshape(B, K1)
    cand = again["candidate_ids"].cpu().numpy()
    for u in range(B):
        assert again["ad_ids"][u].cpu().tolist() == [int(cand[u, s]) for s in go.select_order(z[u], pos[u])[:TOP_K]]


@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_captured_graph_reference_api_and_retriever_return_the_device_result(kind):
    from amdrec.pipeline import Preprocessor, TwoStageRetriever
    from tests import cases
    KINDS, _clone, _rec, _users = _pipeline()
    rec, _, groups = _rec(kind)
    idx = rec.faiss_index
    B = 5
    uc, un = _users(B)
    temps = _dev(np.array([0.0, 0.25, 1.0, 4.0, np.inf], dtype=F32))
    seed_t = _dev(np.array([3, -9, 1 << 50, 77, 0], dtype=np.int64))
    kw = dict(max_per_group=2, explore_from=1)
    eager = {k: _clone(rec.recommend_device(uc, un, TOP_K, K1, explore=e, explore_seed=s, **kw))
             for k, e, s in (("s", 2.0, 5), ("t", temps, seed_t), ("s2", 2.0, 6))}
    greedy = _clone(rec.recommend_device(uc, un, TOP_K, K1, max_per_group=2))
    assert not _same(eager["s"], eager["s2"]) and not _same(eager["s"], eager["t"])
    # the captured graph: temperatures and seeds are static inputs; zeros (every user greedy) until the replayer fills them
    g0 = rec.capture(B, TOP_K, K1, max_per_group=2)
    with pytest.raises(ValueError, match="explore=True"):
        g0(uc, un, explore=1.0, explore_seed=1)
    assert "propensities" not in g0(uc, un)
    g = rec.capture(B, TOP_K, K1, max_per_group=2, explore=True, explore_from=1)
    first = g(uc, un)
    assert _same(first, greedy, ("ad_ids", "scores")) and (first["propensities"] == (first["ad_ids"] >= 0).float()).all()
    assert _same(g(uc, un, explore=2.0, explore_seed=5), eager["s"])
    assert _same(g(uc, un), eager["s"])                                  # no new seed: the same draw again
    assert _same(g(uc, un, explore_seed=6), eager["s2"])                 # a new seed redraws
    assert _same(g(uc, un, explore=temps, explore_seed=seed_t), eager["t"])
    with pytest.raises(ValueError, match="temperature"):
        g(uc, un, explore=-1.0)
    # the reference API: the lists are the device result, propensities in the same block
    user, _, _ = cases.small_dims()
    classes = {c: [f"cat_{j}" for j in range(card)] for c, card in user.items()}
    rec.preprocessor = Preprocessor(classes, [f"I{i}" for i in range(1, 14)], np.zeros(13), np.ones(13))
    host_t, host_s = [0.0, 0.25, 1.0, 4.0, float("inf")][:4] + [8.0], [3, (1 << 64) - 9, 1 << 50, 77, 0]
    for e, s, want in ((2.0, 5, eager["s"]), (temps, seed_t, eager["t"])):
        res = rec.recommend_tensors(uc, un, TOP_K, K1, explore=e, explore_seed=s, **kw)
        for b, r in enumerate(res):
            assert r["ad_ids"] == want["ad_ids"][b].cpu().tolist() and r["scores"]["ctr"] == want["scores"][0, b].cpu().tolist()
            assert np.array_equal(_bits(r["propensities"]), _bits(want["propensities"][b]))
    want = _clone(rec.recommend_device(uc, un, TOP_K, K1, explore=_dev(np.array(host_t, dtype=F32)),
                                       explore_seed=_dev(np.array(host_s, dtype=np.uint64).view(np.int64)), **kw))
    res = rec.recommend_tensors(uc, un, TOP_K, K1, explore=host_t, explore_seed=host_s, **kw)     # one number per user
    assert [r["ad_ids"] for r in res] == want["ad_ids"].cpu().tolist()
    assert np.array_equal(_bits([r["propensities"] for r in res]), _bits(want["propensities"]))
    assert "propensities" not in rec.recommend_tensors(uc, un, TOP_K, K1)[0]
    from tests.test_exclude_gpu import _users as dict_users
    users = dict_users(user, B, 5)
    ucd, und = rec.preprocess_batch(users)
    for e, s, de, ds in ((0.75, (1 << 64) - 2, 0.75, (1 << 64) - 2),
                         (host_t, host_s, _dev(np.array(host_t, dtype=F32)), _dev(np.array(host_s, dtype=np.uint64).view(np.int64)))):
        dev = _clone(rec.recommend_device(ucd, und, TOP_K, K1, explore=de, explore_seed=ds, max_per_group=1))
        res = rec.batch_recommend(users, TOP_K, K1, explore=e, explore_seed=s, max_per_group=1)
        assert [r["ad_ids"] for r in res] == dev["ad_ids"].cpu().tolist()
        assert np.array_equal(_bits([r["propensities"] for r in res]), _bits(dev["propensities"]))
        assert np.array_equal(_bits([r["scores"]["revenue"] for r in res]), _bits(dev["scores"][list(dev["tasks"]).index("revenue")]))
    # (a single request runs the ranker at another batch shape: compare it with the device call of that shape)
    dev1 = _clone(rec.recommend_device(ucd[1:2], und[1:2], TOP_K, K1, explore=0.5, explore_seed=9, explore_from=2))
    one = rec.recommend_ads(users[1], TOP_K, K1, explore=0.5, explore_seed=9, explore_from=2)
    assert one["ad_ids"] == dev1["ad_ids"][0].cpu().tolist()
    assert np.array_equal(_bits(one["propensities"]), _bits(dev1["propensities"][0]))
    assert "propensities" not in rec.recommend_ads(users[1], TOP_K, K1)
    two = TwoStageRetriever(rec.two_tower_model, rec.transformer_ranker, idx)
    want1 = _clone(rec.recommend_device(uc[:1], un[:1], TOP_K, K1, explore=2.0, explore_seed=5, max_per_group=2))
    got = two.retrieve_and_rank(uc, un, K1, TOP_K, ad_features_lookup=rec.ad_features, explore=2.0, explore_seed=5, max_per_group=2)
    assert got[0] == want1["ad_ids"][0].cpu().tolist() and got[1] == want1["scores"][0, 0].cpu().tolist()
    assert isinstance(got, tuple) and len(got) == 2                      # the tuple return is unchanged
