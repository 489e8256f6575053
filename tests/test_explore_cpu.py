"""CPU: the host side of exploration (amdrec.explore) - the numpy oracle's own properties (the uniforms, the Plackett-Luce
frequencies of the Gumbel draw, the greedy cases, the class order, the cap and the propensities), every refusal of ``explore`` /
``explore_seed`` / ``explore_from`` before the library is touched, on every entry point and on capture, the export in the
binding and the header, and the refusals of the C entry (before its first HIP call).  No GPU."""
import ctypes
import inspect
import math
import re

import numpy as np
import pytest
import torch

from amdrec import _lib, explore as ex
from tests import group_cap_oracle as go
from tests.test_abi import HEADER
from tests.test_value_cpu import _entries, _no_library

F32 = np.float32


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def test_mix64_is_the_stated_function_and_the_uniforms_are_exact_float32_inside_the_unit_interval():
    def ref(x):
        m = (1 << 64) - 1
        x ^= x >> 30
        x = x * 0xBF58476D1CE4E5B9 & m
        x ^= x >> 27
        x = x * 0x94D049BB133111EB & m
        return x ^ (x >> 31)
    rng = np.random.default_rng(0)
    vals = [0, 1, (1 << 64) - 1, 1 << 63] + [int(v) for v in rng.integers(0, 1 << 63, size=50)]
    assert [int(ex.mix64(v)) for v in vals] == [ref(v) for v in vals]
    assert ex.mix64(np.array(vals, dtype=np.uint64)).tolist() == [ref(v) for v in vals]
    ids = np.concatenate([rng.integers(-5, 1 << 40, size=20000), [-1, 0, np.iinfo(np.int64).max, np.iinfo(np.int64).min]])
    for seed in (0, 7, (1 << 64) - 1):
        u = ex.uniforms(seed, ids)
        assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all()
        h = [ref(ref(seed) ^ (int(i) & ((1 << 64) - 1))) >> 41 for i in ids.tolist()]
        exact = (np.array(h, dtype=np.float64) + 0.5) * 2.0 ** -23        # the rule in float64: float32 holds it exactly
        assert (u.astype(np.float64) == exact).all()
        g = ex.gumbels(seed, ids)
        assert np.isfinite(g).all() and g.dtype == np.float64
    assert F32((0 + 0.5) * 2.0 ** -23) > 0 and F32(((1 << 23) - 1 + 0.5) * 2.0 ** -23) < 1


def test_first_and_second_pick_frequencies_are_the_softmax():
    """200 000 consecutive seeds on 4 candidates: the first pick, and the second pick given the likeliest first one, within
    5 sigma of the Plackett-Luce probabilities (the keys formed as explore_user forms them, all seeds at once)."""
    z = np.array([0.0, 1.0, -0.5, 2.0], dtype=F32)
    T, n = F32(1.5), 200_000
    ids = np.array([11, 5, 900, 42], dtype=np.int64)
    x = z.astype(np.float64) / np.float64(T)
    keys = (x[None, :] + ex.gumbels(np.arange(n, dtype=np.uint64)[:, None], ids[None, :])).astype(F32)
    order = np.argsort(-keys, axis=1, kind="stable")                       # (k descending, slot ascending)
    pos = np.arange(4, dtype=np.int64)
    for seed in list(range(150)) + [n - 1]:                                # ... which is what the oracle does, seed by seed
        got = ex.explore_user(z, ids, pos, T, seed, 2)
        assert got["slots"].tolist() == order[seed, :2].tolist()
    w = np.exp(x - x.max())
    p1 = w / w.sum()
    cells = []
    for i in range(4):
        cells.append((int((order[:, 0] == i).sum()), n, p1[i]))
    first = int(np.argmax(p1))
    given = order[order[:, 0] == first]
    rest = [i for i in range(4) if i != first]
    for i in rest:
        cells.append((int((given[:, 1] == i).sum()), len(given), w[i] / w[rest].sum()))
    assert len(cells) == 7
    for count, trials, p in cells:
        sigma = math.sqrt(trials * p * (1 - p))
        assert abs(count - trials * p) <= 5 * sigma, (count, trials, p, (count - trials * p) / sigma)
    # the oracle's propensities are these probabilities
    got = ex.explore_user(z, ids, pos, T, 3, 4)
    s = got["slots"].tolist()
    left = list(range(4))
    for r in range(4):
        assert got["propensities"][r] == F32(w[s[r]] / w[left].sum())
        left.remove(s[r])
    assert got["propensities"][3] == 1.0


def random_user(rng, k_c, n_rows=40):
    z = rng.standard_normal(k_c).astype(F32)
    z[rng.random(k_c) < 0.08] = np.nan
    z[rng.random(k_c) < 0.05] = np.inf
    z[rng.random(k_c) < 0.05] = -np.inf
    pos = rng.integers(0, n_rows + 5, size=k_c).astype(np.int64)
    pos[rng.random(k_c) < 0.1] = -1
    ids = rng.permutation(10 * k_c)[:k_c].astype(np.int64)
    group_of = rng.choice(np.array([-1, 0, 7, 1 << 40], dtype=np.int64), size=n_rows)
    return z, ids, pos, group_of


def _capped_order(z, pos, group_of, cap):
    order = go.select_order(z, pos)
    keep = go.greedy_keep([go.group_at(group_of, pos[s]) for s in order], cap)
    return [s for s, k in zip(order, keep) if k]


@pytest.mark.parametrize("cap", [0, 1, 2])
def test_greedy_users_and_a_full_prefix_are_the_plain_selection_with_propensity_one(cap):
    rng = np.random.default_rng(20 + cap)
    for trial in range(60):
        k_c = int(rng.integers(1, 70))
        z, ids, pos, group_of = random_user(rng, k_c)
        want = go.select_order(z, pos) if not cap else _capped_order(z, pos, group_of, cap)
        for top_k in (1, 5, k_c + 3):
            slots = (want + [-1] * top_k)[:top_k]
            for T, g in ((0.0, 0), (-1.0, 2 if top_k > 2 else 0), (float("nan"), 0), (1.0, top_k), (float("inf"), top_k)):
                got = ex.explore_user(z, ids, pos, T, 9, top_k, g, group_of, len(group_of), cap)
                assert got["slots"].tolist() == slots
                assert got["propensities"].tolist() == [1.0 if s >= 0 else 0.0 for s in slots]


@pytest.mark.parametrize("cap", [0, 1, 2])
def test_the_sampled_walk_keeps_the_prefix_the_class_order_the_cap_and_exact_propensities(cap):
    rng = np.random.default_rng(40 + cap)
    for trial in range(60):
        k_c = int(rng.integers(2, 70))
        z, ids, pos, group_of = random_user(rng, k_c)
        T = float(rng.choice([0.25, 1.0, 4.0, np.inf]))
        plain = go.select_order(z, pos) if not cap else _capped_order(z, pos, group_of, cap)
        for g in (0, 1, 3):
            top_k = k_c + 2
            got = ex.explore_user(z, ids, pos, T, trial, top_k, g, group_of, len(group_of), cap)
            won = [s for s in got["slots"].tolist() if s >= 0]
            assert won[:g] == plain[:g] and len(set(won)) == len(won) and len(won) == len(plain)
            assert cap or sorted(won) == sorted(plain)                    # (under a cap the draw decides who stands for a group)
            assert (got["propensities"][:min(g, len(won))] == 1.0).all() and (got["propensities"][len(won):] == 0.0).all()
            tail = won[g:]
            cls = [0 if z[s] == np.inf else 1 if np.isfinite(z[s]) else 2 if z[s] == -np.inf else 3 for s in tail]
            if not cap:
                assert cls == sorted(cls)
                for c in (0, 2, 3):                                       # the forced classes keep slot order
                    assert [s for s, k in zip(tail, cls) if k == c] == sorted(s for s, k in zip(tail, cls) if k == c)
                k32 = got["keys"].astype(F32)
                fin = [s for s, k in zip(tail, cls) if k == 1]
                assert all(k32[a] > k32[b] or (k32[a] == k32[b] and a < b) for a, b in zip(fin, fin[1:]))
            counts = {}
            for s in won:
                gk = int(group_of[pos[s]]) if cap and pos[s] < len(group_of) else -1
                counts[gk] = counts.get(gk, 0) + 1
            assert all(v <= cap for k, v in counts.items() if k >= 0) or not cap
            for r, s in enumerate(won):
                p = got["propensities"][r]
                assert 0.0 <= p <= 1.0 and (p == 1.0 or (r >= g and np.isfinite(z[s])))
            if T == np.inf and not cap:                                   # a uniform draw: 1 / (finite candidates left)
                n_fin = int(np.isfinite(z[plain]).sum()) - int(np.isfinite(z[plain[:g]]).sum())
                seen = 0
                for r, s in enumerate(won[g:], start=g):
                    if np.isfinite(z[s]):
                        assert got["propensities"][r] == F32(1.0 / (n_fin - seen))
                        seen += 1


def test_the_noise_is_keyed_on_the_ad_id_not_the_slot():
    rng = np.random.default_rng(5)
    for trial in range(30):
        k_c = int(rng.integers(2, 60))
        z, ids, pos, _ = random_user(rng, k_c)
        z = np.where(np.isfinite(z), z, F32(0.5) + rng.standard_normal(k_c).astype(F32)).astype(F32)   # (forced classes go by slot)
        a = ex.explore_user(z, ids, pos, 1.0, 77, 6)
        perm = rng.permutation(k_c)
        b = ex.explore_user(z[perm], ids[perm], pos[perm], 1.0, 77, 6)
        ida = [int(ids[s]) for s in a["slots"] if s >= 0]
        idb = [int(ids[perm][s]) for s in b["slots"] if s >= 0]
        assert ida == idb and np.array_equal(a["propensities"], b["propensities"])
        c = ex.explore_user(z, ids, pos, 1.0, 78, 6)
        assert k_c < 4 or [int(ids[s]) for s in c["slots"] if s >= 0] != ida or trial % 7       # (another seed, another draw)


def test_the_batch_oracle_and_the_host_helpers():
    rng = np.random.default_rng(6)
    k_c, top_k = 30, 4
    rows = [random_user(rng, k_c) for _ in range(3)]
    z, ids, pos = (np.stack([r[i] for r in rows]) for i in range(3))
    temp = np.array([0.0, 1.0, 4.0], dtype=F32)
    seeds = np.array([5, (1 << 64) - 1, 1 << 63], dtype=np.uint64)
    got = ex.explore_oracle(z, ids, pos, temp, seeds, top_k, 1)
    same = ex.explore_oracle(z, ids, pos, temp, seeds.view(np.int64), top_k, 1)                  # (int64 bit patterns)
    for u in range(3):
        one = ex.explore_user(z[u], ids[u], pos[u], temp[u], int(seeds[u]), top_k, 1)
        assert got["slots"][u].tolist() == one["slots"].tolist() == same["slots"][u].tolist()
        assert np.array_equal(got["propensities"][u], one["propensities"])
        assert got["ids"][u].tolist() == [int(ids[u, s]) if s >= 0 else -1 for s in one["slots"]]
    e = ex.check_explore(0.5, (1 << 64) - 2, 0, 10)
    t, s = ex.host_arrays(e, 4)
    assert t.dtype == np.float32 and t.tolist() == [0.5] * 4
    assert s.dtype == np.uint64 and s.tolist() == [(1 << 64) - 2, (1 << 64) - 1, 0, 1]           # (seed + u) mod 2^64
    e = ex.check_explore([0, 0.25], [3, (1 << 64) - 1], 2, 10, 2, per_user=True)
    t, s = ex.host_arrays(e, 2)
    assert t.tolist() == [0.0, 0.25] and s.tolist() == [3, (1 << 64) - 1] and e.greedy == 2
    assert ex.seed_tensor((1 << 64) - 1, 3, "cpu").tolist() == [-1, 0, 1]
    assert ex.temperature_tensor(0.5, 2, "cpu").tolist() == [0.5, 0.5]


# ---- refusals -----------------------------------------------------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """A host tensor that says it lives on the device: the shape refusals come behind the device check."""
    is_cuda = True


def _dev(t):
    return t.as_subclass(_OnDevice)


def test_check_explore():
    chk = ex.check_explore
    assert chk(None, None, 0, 10) is None
    assert chk(0, 0, 0, 10) == (0.0, 0, 0) and chk(1.5, (1 << 64) - 1, 10, 10) == (1.5, (1 << 64) - 1, 10)
    assert chk(np.float32(0.1), np.int64(4), np.int32(2), 128) == (float(np.float32(0.1)), 4, 2)
    nan, inf = float("nan"), float("inf")
    with pytest.raises(ValueError, match="explore without explore_seed"):
        chk(1.0, None, 0, 10)
    with pytest.raises(ValueError, match="explore_seed without explore"):
        chk(None, 1, 0, 10)
    with pytest.raises(ValueError, match="explore_from without explore"):
        chk(None, None, 1, 10)
    for g in (-1, 11):
        with pytest.raises(ValueError, match="explore_from"):
            chk(1.0, 1, g, 10)
    with pytest.raises(ValueError, match="top_k <= 128"):
        chk(1.0, 1, 0, 129)
    for bad in (-1.0, -1e-30, nan, inf, -inf, 1e39):
        with pytest.raises(ValueError, match="explore"):
            chk(bad, 1, 0, 10)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match="explore_seed"):
            chk(1.0, bad, 0, 10)
    for bad in (True, "1", [1.0], (1.0,), np.bool_(True), torch.ones(2, dtype=torch.float64), torch.ones(2, dtype=torch.int64),
                torch.ones(2), _dev(torch.ones(2, dtype=torch.float64))):                      # (the one before last: not on the device)
        with pytest.raises(TypeError, match="explore"):
            chk(bad, 1, 0, 10, 2)
    for bad in (True, "1", 1.5, [1], torch.ones(2, dtype=torch.int32), torch.ones(2, dtype=torch.int64),
                _dev(torch.ones(2, dtype=torch.float32))):
        with pytest.raises(TypeError, match="explore_seed"):
            chk(1.0, bad, 0, 10, 2)
    for bad in (True, 1.0, "1", None):
        with pytest.raises(TypeError, match="explore_from"):
            chk(1.0, 1, bad, 10)
    with pytest.raises(TypeError, match="explore_from"):                  # ... whether or not anything explores
        chk(None, None, True, 10)
    for bad in (_dev(torch.ones(3)), _dev(torch.ones((2, 1))), _dev(torch.ones(()))):
        with pytest.raises(ValueError, match="explore must be a float32 tensor"):
            chk(bad, 1, 0, 10, 2)
    for bad in (_dev(torch.ones(3, dtype=torch.int64)), _dev(torch.ones((2, 1), dtype=torch.int64))):
        with pytest.raises(ValueError, match="explore_seed must be an int64 tensor"):
            chk(1.0, bad, 0, 10, 2)
    t, s = _dev(torch.ones(2)), _dev(torch.ones(2, dtype=torch.int64))
    got = chk(t, s, 1, 10, 2)
    assert got.temperature is t and got.seed is s and chk(t, s, 0, 10).greedy == 0
    for kw in (dict(auction=True), dict(head_weights=True), dict(diversity=True)):
        with pytest.raises(ValueError, match="explore together"):
            chk(1.0, 1, 0, 10, **kw)
        assert chk(None, None, 0, 10, **kw) is None
    # one per user: the host calls only
    assert chk([0, 1.5], 7, 0, 10, 2, per_user=True).temperature.tolist() == [0.0, 1.5]
    assert chk(np.array([0.5, 1.5]), np.array([1, 2]), 0, 10, 2, per_user=True).seed.dtype == np.uint64
    for bad, err in (([0.5], ValueError), ([0.5, -1.0], ValueError), ([0.5, nan], ValueError), ([0.5, True], TypeError),
                     ([0.5, "1"], TypeError)):
        with pytest.raises(err, match="explore"):
            chk(bad, 1, 0, 10, 2, per_user=True)
    for bad, err in (([1], ValueError), ([1, -1], ValueError), ([1, 1 << 64], ValueError), ([1, 1.0], TypeError),
                     ([1, True], TypeError)):
        with pytest.raises(err, match="explore_seed"):
            chk(1.0, bad, 0, 10, 2, per_user=True)


def test_explore_refusals_come_before_the_library_on_every_entry_point(monkeypatch):
    _no_library(monkeypatch)
    calls, captures, rec = _entries()
    nan = float("nan")
    for call in calls:
        with pytest.raises(ValueError, match="explore without explore_seed"):
            call(explore=1.0)
        with pytest.raises(ValueError, match="explore_seed without explore"):
            call(explore_seed=3)
        with pytest.raises(ValueError, match="explore_from without explore"):
            call(explore_from=2)
        for g in (-1, 11):
            with pytest.raises(ValueError, match="explore_from"):
                call(explore=1.0, explore_seed=3, explore_from=g)
        for bad in (-0.5, nan, float("inf")):
            with pytest.raises(ValueError, match="temperature"):
                call(explore=bad, explore_seed=3)
        for bad in (-1, 1 << 64):
            with pytest.raises(ValueError, match="explore_seed"):
                call(explore=1.0, explore_seed=bad)
        for bad in (True, "0.5", torch.ones(1, dtype=torch.float64), torch.ones(1)):
            with pytest.raises(TypeError, match="explore"):
                call(explore=bad, explore_seed=3)
        for bad in (True, 2.0, "3", torch.ones(1, dtype=torch.int32), torch.ones(1, dtype=torch.int64)):
            with pytest.raises(TypeError, match="explore_seed"):
                call(explore=1.0, explore_seed=bad)
        for bad in (True, 1.0):
            with pytest.raises(TypeError, match="explore_from"):
                call(explore=1.0, explore_seed=3, explore_from=bad)
        for kw in (dict(rank_by="ecpm"), dict(rank_by="ecpm", reserve=0.5), dict(head_weights=[1, 1, 1]), dict(diversity=0.5)):
            with pytest.raises(ValueError, match="explore together"):
                call(explore=1.0, explore_seed=3, **kw)
        with pytest.raises(ValueError, match=">= 1"):                    # the cap refusal still comes first
            call(explore=-1.0, explore_seed=3, max_per_group=0)
        with pytest.raises(ValueError, match='needs rank_by="ecpm"'):    # and the auction's
            call(explore=1.0, explore_seed=3, reserve=0.5)
    for call in calls[:4]:                                               # (retrieve_and_rank names its top_k stage2_k)
        with pytest.raises(ValueError, match="top_k <= 128"):
            call(explore=1.0, explore_seed=3, top_k=129)
        with pytest.raises(ValueError, match="explore_from"):
            call(explore=1.0, explore_seed=3, explore_from=6, top_k=5)
    with pytest.raises(ValueError, match="top_k <= 128"):
        calls[4](explore=1.0, explore_seed=3, stage2_k=129)
    # shapes: a device tensor for the wrong number of users
    uc = torch.zeros((2, 6), dtype=torch.int64)
    for kw in (dict(explore=_dev(torch.ones(3)), explore_seed=3), dict(explore=1.0, explore_seed=_dev(torch.ones(3, dtype=torch.int64)))):
        with pytest.raises(ValueError, match=r"tensor \[2\]"):
            rec.recommend_device(uc, None, **kw)
        with pytest.raises(ValueError, match=r"tensor \[2\]"):
            rec.recommend_tensors(uc, None, **kw)
    # one number per user: the host calls take it, the device call does not
    for call in (lambda **kw: rec.recommend_tensors(uc[:1], None, **kw), *calls[2:4]):
        with pytest.raises(ValueError, match="one temperature per user"):
            call(explore=[0.5, 0.5], explore_seed=3)
        with pytest.raises(ValueError, match="one seed per user"):
            call(explore=0.5, explore_seed=[3, 4])
        with pytest.raises(TypeError, match="explore"):
            call(explore=[True], explore_seed=3)
    with pytest.raises(TypeError, match="explore"):
        calls[0](explore=[0.5], explore_seed=3)
    for call in captures:
        for bad in (1.0, 1, "yes", None):
            with pytest.raises(TypeError, match="explore"):
                call(explore=bad)
        for kw in (dict(rank_by="ecpm"), dict(head_weights=True), dict(diversity=0.5)):
            with pytest.raises(ValueError, match="explore together"):
                call(explore=True, **kw)
        with pytest.raises(ValueError, match="explore_from without explore"):
            call(explore_from=1)
        with pytest.raises(ValueError, match="explore_from"):
            call(explore=True, explore_from=11)
        with pytest.raises(TypeError, match="explore_from"):
            call(explore=True, explore_from=True)
        with pytest.raises(ValueError, match=">= 1"):
            call(explore=True, max_per_group=0)
    with pytest.raises(ValueError, match="top_k <= 128"):
        rec.capture(2, top_k=129, explore=True)


def test_a_replayer_captured_without_explore_takes_no_temperatures_and_checks_the_ones_it_takes(monkeypatch):
    from amdrec.pipeline import GraphedRecommender
    _no_library(monkeypatch)
    g = object.__new__(GraphedRecommender)
    g._temp = g._seed = None
    g.top_k, g.batch_size = 10, 2
    for kw in (dict(explore=1.0), dict(explore_seed=3), dict(explore=1.0, explore_seed=3)):
        with pytest.raises(ValueError, match="captured without explore=True"):
            g._replay(None, None, **kw)
    g._temp, g._seed = torch.zeros(2), torch.zeros(2, dtype=torch.int64)
    for kw, err in ((dict(explore=-1.0), ValueError), (dict(explore=True), TypeError), (dict(explore_seed=1 << 64), ValueError),
                    (dict(explore_seed=1.0), TypeError), (dict(explore=_dev(torch.ones(3))), ValueError),
                    (dict(explore_seed=torch.ones(2, dtype=torch.int64)), TypeError)):
        with pytest.raises(err, match="explore"):
            g._replay(None, None, **kw)
    assert g._temp.tolist() == [0.0, 0.0] and g._seed.tolist() == [0, 0]                         # nothing was written


def test_sharded_serving_and_the_micro_batcher_do_not_take_the_arguments():
    from amdrec.serving import MicroBatcher
    from amdrec.sharded import ShardedRecommender
    for cls in (MicroBatcher, ShardedRecommender):
        for name, fn in inspect.getmembers(cls, inspect.isfunction):
            for arg in ("explore", "explore_seed", "explore_from"):
                assert arg not in inspect.signature(fn).parameters, (cls.__name__, name)


def test_every_serving_entry_takes_the_three_arguments_and_defaults_to_no_exploration():
    from amdrec.pipeline import AdRecommenderInference, TwoStageRetriever
    for fn in (AdRecommenderInference.recommend_device, AdRecommenderInference.recommend_tensors,
               AdRecommenderInference.recommend_ads, AdRecommenderInference.batch_recommend, TwoStageRetriever.retrieve_and_rank):
        p = inspect.signature(fn).parameters
        assert p["explore"].default is None and p["explore_seed"].default is None and p["explore_from"].default == 0
    p = inspect.signature(AdRecommenderInference.capture).parameters
    assert p["explore"].default is False and p["explore_from"].default == 0


# ---- the C entry --------------------------------------------------------------------------------------------------------------
def _header_arg_count(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_the_entry_is_bound_and_the_header_agrees_with_the_binding():
    lib = _lib.load()
    src = open(HEADER).read()
    assert lib.amdrec_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define AMDREC_ABI_VERSION (\d+)", src).group(1))
    name = "amdrec_select_topk_sampled"
    assert name in _lib.exported_symbols()
    assert len(getattr(lib, name).argtypes) == 20 == len(_lib._SIGNATURES[name]) == _header_arg_count(name)
    # the capped entry's arguments, then four inputs and one output
    assert _lib._SIGNATURES[name][:15] == _lib._SIGNATURES["amdrec_select_topk_capped"][:15]
    assert _header_arg_count("amdrec_select_topk_capped") + 4 == 20


def test_the_entry_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    raw = ctypes.create_string_buffer(4096 + 256)
    p = (ctypes.addressof(raw) + 255) // 256 * 256                         # non-null, aligned, never dereferenced

    def select(n_tasks=3, rank=0, ids=p, pos=p, users=1, k_c=500, top_k=10, out=p, sc=p, slots=None, groups=p, n_rows=100, cap=2,
               temp=p, seeds=p, greedy=0, prop=p, ld=500, logits=p):
        return lib.amdrec_select_topk_sampled(logits, ld, n_tasks, rank, ids, pos, users, k_c, top_k, out, sc, slots, groups,
                                              n_rows, cap, temp, seeds, greedy, prop, None)
    assert select(n_tasks=0) == -1 and select(rank=3) == -1 and select(rank=-1) == -1 and b"task" in lib.amdrec_last_error()
    assert select(k_c=0) == -1 and select(k_c=_lib.MAX_K + 1) == -1 and b"candidates" in lib.amdrec_last_error()
    assert select(top_k=0) == -1 and b"top_k=0" in lib.amdrec_last_error()
    assert select(top_k=129, greedy=0) == -1 and b"top_k=129" in lib.amdrec_last_error()
    assert select(greedy=-1) == -1 and b"greedy=-1" in lib.amdrec_last_error()
    assert select(greedy=11) == -1 and b"greedy=11" in lib.amdrec_last_error()
    assert select(cap=-1) == -1 and b"max_per_group=-1" in lib.amdrec_last_error()
    assert select(cap=_lib.MAX_K + 1) == -1 and b"max_per_group=2049" in lib.amdrec_last_error()
    assert select(n_rows=-1) == -1 and b"n_group_rows" in lib.amdrec_last_error()
    assert select(users=1 << 31) == -1 and b"n_users" in lib.amdrec_last_error()
    assert select(pos=None) == -1 and b"cand_pos" in lib.amdrec_last_error()
    assert select(groups=None) == -1 and b"group_of" in lib.amdrec_last_error()          # required iff capped
    for kw in (dict(temp=None), dict(seeds=None), dict(prop=None)):
        assert select(**kw) == -1 and b"temperature, seeds or out_propensity" in lib.amdrec_last_error()
    for kw in (dict(ids=None), dict(out=None), dict(sc=None), dict(logits=None)):
        assert select(**kw) == -1 and b"null pointer" in lib.amdrec_last_error()
    for kw in (dict(seeds=p + 4), dict(ids=p + 4), dict(pos=p + 2), dict(out=p + 1), dict(groups=p + 4)):
        assert select(**kw) == -1 and b"8-byte aligned" in lib.amdrec_last_error()
    for kw in (dict(logits=p + 2), dict(temp=p + 1), dict(sc=p + 2), dict(prop=p + 3), dict(slots=p + 2)):
        assert select(**kw) == -1 and b"4-byte aligned" in lib.amdrec_last_error()
    assert select(ld=499) == -1 and b"ld_logits" in lib.amdrec_last_error()
    assert select(users=0, ids=None, pos=None, groups=None, out=None, sc=None, temp=None, seeds=None, prop=None, logits=None) == 0
    assert select(users=-3, cap=0, groups=None) == 0                                      # no user: nothing to do
    del raw
