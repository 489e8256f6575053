"""CPU: the host side of value ranking (amdrec.value) - the numpy oracle's own properties (the two one-hot consequences against
the auction tests' numpy rule, zero-weight heads, the tie order, the price cases), every refusal of ``head_weights`` before the
library is touched, on every entry point and on capture, the two exports in the binding and the header, and the refusals of
the C entries (before their first HIP call).  No GPU."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

from amdrec import _lib, value as va
from tests import auction_oracle as ao
from tests import group_cap_oracle as go
from tests.test_abi import HEADER

F32 = np.float32
TASKS = ["ctr", "engagement", "revenue"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def random_user(rng, k_c, n_tasks=3, nan=0.1):
    """-> (logits [n_tasks, k_c], p = sigmoid(logits), pos, bid_of, group_of) for one user, heavy ties, NaNs, holes."""
    logits = rng.choice(ao.VALUES, size=(n_tasks, k_c))
    logits[rng.random(logits.shape) < nan] = np.nan
    n_rows = 40
    pos = rng.integers(0, n_rows + 5, size=k_c).astype(np.int64)          # (>= n_rows: no bid of its own, no group)
    pos[rng.random(k_c) < 0.15] = -1
    return (logits, ao.sigmoid(logits), pos, rng.choice(ao.BIDS, size=n_rows),
            rng.choice(np.array([-1, 0, 7, 1 << 40], dtype=np.int64), size=n_rows))


@pytest.mark.parametrize("cap", [0, 1, 2])
def test_one_hot_weights_under_the_auction_are_the_auction_rule_bit_for_bit(cap):
    rng = np.random.default_rng(70 + cap)
    for trial in range(60):
        k_c = int(rng.integers(1, 70))
        _, p, pos, bid_of, group_of = random_user(rng, k_c)
        for r_task in (0, 2):
            w = np.zeros(3, dtype=F32)
            w[r_task] = 1.0
            for reserve in (None, F32(0.0), F32(0.4), F32(9.0)):
                order, e, b = ao.accepted(p[r_task], pos, bid_of, len(bid_of), reserve, group_of, cap)
                for top_k in (1, 5, k_c + 3):
                    slots, ecpm, price, _ = ao.results(order, e, b, p[r_task], reserve, top_k)
                    got = va.select_user(p, pos, w, top_k, group_of, len(group_of), cap, r_task, bid_of, len(bid_of), reserve)
                    assert got["slots"].tolist() == slots.tolist() and got["order"] == order
                    assert np.array_equal(bits(got["ecpm"]), bits(ecpm)) and np.array_equal(bits(got["price"]), bits(price))
                    assert np.array_equal(bits(got["values"]), bits(ecpm))               # v = e


def test_one_hot_weights_order_by_the_probability_which_is_the_logit_order_only_without_ties():
    rng = np.random.default_rng(3)
    for trial in range(40):
        k_c = int(rng.integers(2, 60))
        logits = rng.standard_normal((3, k_c)).astype(F32) * 3                             # distinct logits, distinct sigmoids
        p = ao.sigmoid(logits)
        pos = np.where(rng.random(k_c) < 0.2, -1, np.arange(k_c)).astype(np.int64)
        for r_task in range(3):
            assert len(set(p[r_task].tolist())) == k_c
            w = np.zeros(3, dtype=F32)
            w[r_task] = 1.0
            got = va.select_user(p, pos, w, k_c)
            assert got["order"] == go.select_order(logits[r_task], pos)
            n = len(got["order"])
            assert np.array_equal(bits(got["values"][:n]), bits(p[r_task][got["order"]])) and (got["values"][n:] == 0).all()
    # saturated sigmoids tie and resolve by slot: not the logit order
    logits = np.array([[20.0, 30.0, 25.0, 1.0]] * 3, dtype=F32)
    p = ao.sigmoid(logits)
    assert p[0, 0] == p[0, 1] == p[0, 2] == 1.0
    pos = np.arange(4, dtype=np.int64)
    assert va.select_user(p, pos, [1, 0, 0], 4)["order"] == [0, 1, 2, 3] != go.select_order(logits[0], pos)


def test_a_zero_weight_head_has_no_influence_nan_included_and_all_zero_weights_give_plus_zero():
    rng = np.random.default_rng(4)
    for trial in range(40):
        k_c = int(rng.integers(1, 50))
        _, p, pos, bid_of, group_of = random_user(rng, k_c, nan=0.0)
        w = np.array([0.75, -0.0 if trial % 2 else 0.0, -1.5], dtype=F32)
        dirty = p.copy()
        dirty[1] = np.where(rng.random(k_c) < 0.5, np.nan, rng.random(k_c)).astype(F32)
        for kw in (dict(), dict(rank_task=0, bid_of=bid_of, n_bid_rows=len(bid_of), reserve=F32(-0.5))):
            a = va.select_user(p, pos, w, 7, group_of, len(group_of), 2, **kw)
            b = va.select_user(dirty, pos, w, 7, group_of, len(group_of), 2, **kw)
            for k in ("slots", "values", "ecpm", "price"):
                assert np.array_equal(bits(a[k]), bits(b[k])), k
            assert not np.isnan(a["values"]).any()
        z = va.select_user(dirty, pos, np.array([0.0, -0.0, 0.0], dtype=F32), 5)
        assert z["order"] == [i for i in range(k_c) if pos[i] >= 0] and (bits(z["values"]) == 0).all()
    assert bits(va.chain(np.array([0, -1], dtype=F32), np.array([np.nan, 0.0], dtype=F32)))[0] == bits(F32(-0.0))[0]


def test_the_order_is_value_descending_then_slot_nan_last_and_signed_zeros_tie():
    p = np.array([[0.5, 0.0, 0.5, np.nan, 0.25, 0.0, np.nan, 0.5]] * 2, dtype=F32)
    p[1] = 0.0
    pos = np.array([3, 1, 0, 2, 9, 4, 5, -1], dtype=np.int64)
    got = va.select_user(p, pos, np.array([2.0, 0.0], dtype=F32), 8)
    assert got["order"] == [0, 2, 4, 1, 5, 3, 6] and got["slots"].tolist() == [0, 2, 4, 1, 5, 3, 6, -1]
    assert bits(got["values"]).tolist() == bits(np.array([1, 1, 0.5, 0, 0, np.nan, np.nan, 0], dtype=F32)).tolist()
    neg = va.select_user(p, pos, np.array([-2.0, 0.0], dtype=F32), 4)     # -0.0 (slots 1, 5) sorts with +0.0, above -0.5
    assert neg["order"][:4] == [1, 5, 4, 0] and np.signbit(neg["values"][:2]).all() and (neg["values"][:2] == 0).all()
    rng = np.random.default_rng(5)
    for trial in range(40):
        k_c = int(rng.integers(1, 60))
        _, pr, ps, bid_of, group_of = random_user(rng, k_c)
        w = rng.choice(np.array([-1.0, 0.0, 0.5, 2.0], dtype=F32), size=3)
        got = va.select_user(pr, ps, w, k_c)
        v = np.array([va.chain(w, pr[:, i]) for i in range(k_c)])
        order = got["order"]
        fin = [s for s in order if not np.isnan(v[s])]
        assert sorted(order) == [i for i in range(k_c) if ps[i] >= 0]
        assert order == fin + sorted(s for s in order if np.isnan(v[s]))
        assert all(v[x] > v[y] or (v[x] == v[y] and x < y) for x, y in zip(fin, fin[1:]))


def _priced(p_ctr, p_rev, w, bids, top_k, reserve=None):
    p = np.array([p_ctr, p_rev], dtype=F32)
    k_c = p.shape[1]
    return va.select_user(p, np.arange(k_c, dtype=np.int64), np.array(w, dtype=F32), top_k, rank_task=0,
                          bid_of=np.array(bids, dtype=F32), n_bid_rows=k_c, reserve=None if reserve is None else F32(reserve))


def test_price_cases():
    # the plain second price under a blend: floor = next v, q = the quality term, d = w_ctr * p
    got = _priced([0.5, 0.25], [0.5, 0.5], [1.0, 0.5], [4.0, 4.0], 1)
    v0, v1 = F32(4.0 * 0.5 + 0.25), F32(4.0 * 0.25 + 0.25)
    assert got["values"][0] == v0 and got["ecpm"][0] == 2.0 and got["price"][0] == F32((v1 - F32(0.25)) / F32(0.5)) == 2.0
    # num <= 0: the quality alone holds the rank
    got = _priced([0.5, 0.5], [0.9, 0.1], [1.0, 2.0], [1.0, 1.0], 1)
    assert got["slots"][0] == 0 and got["price"][0] == 0.0 and got["values"][0] == F32(0.5) + F32(2.0) * F32(0.9)
    # negative quality weights: a negative next value, floor 0 without a reserve, num = 0 - q > 0
    got = _priced([0.5, 0.5], [0.25, 0.75], [1.0, -2.0], [1.0, 1.0], 2)
    assert got["slots"].tolist() == [0, 1] and got["values"].tolist() == [0.0, -1.0]
    assert got["price"][0] == 1.0 and got["price"][1] == 1.0              # min(b, (0 + 0.5) / 0.5), min(b, (0 + 1.5) / 0.5)
    # d <= 0: a CTR weight of zero or below, or p = 0 - the bid does not hold the rank
    for w_ctr, p0 in ((0.0, 0.5), (-1.0, 0.5), (1.0, 0.0)):
        got = _priced([p0, 0.25], [0.9, 0.1], [w_ctr, 1.0], [2.0, 2.0], 1, reserve=-5.0)
        assert got["slots"][0] == 0 and bits(got["price"])[0] == 0
    # no runner-up: the reserve, or zero
    got = _priced([0.5], [0.0], [1.0, 1.0], [3.0], 2, reserve=0.75)
    assert got["slots"].tolist() == [0, -1] and got["price"][0] == F32(0.75) / F32(0.5) and got["price"][1] == 0 == got["values"][1]
    assert _priced([0.5], [0.0], [1.0, 1.0], [3.0], 2)["price"][0] == 0.0
    # a NaN runner-up counts as 0; a NaN winner has a NaN price and the canonical NaN value
    got = _priced([0.5, 0.5], [0.0, np.nan], [1.0, 1.0], [3.0, 3.0], 2)
    assert got["slots"].tolist() == [0, 1] and got["price"][0] == 0.0
    assert bits(got["price"])[1] == bits(va.NAN)[0] == bits(got["values"])[1] and got["ecpm"][1] == 1.5
    # a runner-up dropped by the reserve: the reserve is the floor
    got = _priced([0.5, 0.125], [0.0, 0.0], [1.0, 1.0], [2.0, 2.0], 1, reserve=0.5)
    assert got["order"] == [0] and got["price"][0] == 1.0                 # 0.5 / 0.5, not 0.25 / 0.5
    # never above the winner's own bid
    got = _priced([0.5, 0.5], [0.0, 1.0], [1.0, -1.0], [1.0, 8.0], 1)
    assert got["slots"][0] == 1 and got["price"][0] == F32((0.5 + 1.0) / 0.5) and got["price"][0] <= 8.0


def test_the_reported_value_is_the_chain_over_the_reported_scores():
    rng = np.random.default_rng(9)
    for trial in range(30):
        k_c = int(rng.integers(1, 50))
        _, p, pos, bid_of, group_of = random_user(rng, k_c)
        w = rng.choice(np.array([-1.0, 0.0, 0.5, 2.0], dtype=F32), size=3)
        got = va.select_user(p, pos, w, 6, rank_task=0, bid_of=bid_of, n_bid_rows=len(bid_of))
        for r, s in enumerate(got["slots"]):
            if s >= 0:
                y = p[:, s].copy()
                y[0] = got["ecpm"][r]
                v = va.chain(w, y)
                assert bits(got["values"])[r] == bits(va.NAN if np.isnan(v) else v)[0]


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_check_head_weights():
    chk = va.check_head_weights
    assert chk(None, TASKS) is None
    assert chk({"ctr": 1, "revenue": 0.5}, TASKS) == (1.0, 0.0, 0.5) and chk([0, 0, -2], TASKS) == (0.0, 0.0, -2.0)
    assert chk(np.array([1, 2, 3], dtype=np.float64), TASKS) == (1.0, 2.0, 3.0) and chk((1.0,), ["ctr"]) == (1.0,)
    assert chk([0.1, 0, 0], TASKS)[0] == float(np.float32(0.1))
    nan, inf = float("nan"), float("inf")
    for bad in ([True, 1, 1], {"ctr": False}, ["1", 1, 1], [None, 1, 1], 1.0, "abc", True, torch.ones((2, 3), dtype=torch.float64),
                torch.ones((2, 3), dtype=torch.int64), torch.ones((2, 3))):                # (the last: float32, but not on the device)
        with pytest.raises(TypeError, match="head_weights"):
            chk(bad, TASKS, 2)
    for bad in ([1, nan, 1], [inf, 1, 1], [1e39, 0, 0], {"clicks": 1.0}, {"ctr": 1.0, "x": 0}, [1, 1], [1, 1, 1, 1], [], {},
                [0, 0, 0], [0.0, -0.0, 0], {"ctr": 0.0}):
        with pytest.raises(ValueError, match="head_weights"):
            chk(bad, TASKS, 2)
    for bad in ([0, 1, 1], [-1, 1, 1], {"revenue": 1.0}):
        assert chk(bad, TASKS) is not None
        with pytest.raises(ValueError, match="CTR weight > 0"):
            chk(bad, TASKS, 2, auction=True)
    with pytest.raises(ValueError, match="diversity"):
        chk([1, 1, 1], TASKS, diversity=True)
    with pytest.raises(ValueError, match="ctr_first"):
        chk([1, 1, 1], TASKS, heads="ctr_first")
    assert chk([1, 1, 1], TASKS, heads="all") == (1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="at most 4"):
        chk([1] * 5, list("abcde"))


def _no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))


def _entries():
    from amdrec.pipeline import AdRecommenderInference, GraphedRecommender, TwoStageRetriever
    from tests.test_auction_cpu import _bare_index
    idx = _bare_index(bids=torch.ones(3), groups=torch.zeros(3, dtype=torch.int64))
    ranker = types.SimpleNamespace(prediction_heads=dict.fromkeys(TASKS))
    rec = object.__new__(AdRecommenderInference)
    rec.faiss_index, rec.heads_mode, rec.transformer_ranker = idx, "ctr_first", ranker
    two = object.__new__(TwoStageRetriever)
    two.faiss_index, two.transformer_ranker = idx, ranker
    return [lambda **kw: rec.recommend_device(None, None, **kw), lambda **kw: rec.recommend_tensors(None, None, **kw),
            lambda **kw: rec.batch_recommend([{}], **kw), lambda **kw: rec.recommend_ads({}, **kw),
            lambda **kw: two.retrieve_and_rank(None, None, **kw)], \
        [lambda **kw: rec.capture(2, **kw), lambda **kw: GraphedRecommender(rec, 2, 10, 500, **kw)], rec


def test_head_weights_refusals_come_before_the_library_on_every_entry_point(monkeypatch):
    from amdrec.sharded import ShardedRecommender
    _no_library(monkeypatch)
    calls, captures, rec = _entries()
    nan = float("nan")
    for call in calls:
        for bad in ([True, 1, 1], ["1", 1, 1], 2.0, torch.ones((1, 3), dtype=torch.float64), torch.ones((1, 3))):
            with pytest.raises(TypeError, match="head_weights"):
                call(head_weights=bad)
        for bad in ([1, nan, 1], [1, float("inf"), 1], {"clicks": 1.0}, [1, 1], [0, 0, 0], {}):
            with pytest.raises(ValueError, match="head_weights"):
                call(head_weights=bad)
        for bad in ([0, 1, 1], {"ctr": -1.0, "revenue": 1.0}):
            with pytest.raises(ValueError, match="CTR weight > 0"):
                call(head_weights=bad, rank_by="ecpm")
        with pytest.raises(ValueError, match="head_weights together with diversity"):
            call(head_weights=[1, 1, 1], diversity=0.5)
        with pytest.raises(ValueError, match=">= 1"):                    # the cap refusal still comes first
            call(head_weights=[0, 0, 0], max_per_group=0)
        with pytest.raises(ValueError, match='needs rank_by="ecpm"'):    # and the auction's
            call(head_weights=[0, 0, 0], reserve=0.5)
    with pytest.raises(ValueError, match="ctr_first"):                   # an explicit per-call "ctr_first" (recommend_device only)
        calls[0](head_weights=[1, 1, 1], heads="ctr_first")
    for call in captures:
        with pytest.raises(ValueError, match="head_weights together with diversity"):
            call(head_weights=True, diversity=0.5)
        with pytest.raises(ValueError, match=">= 1"):
            call(head_weights=True, max_per_group=0)
    sh = object.__new__(ShardedRecommender)
    for kw in (dict(head_weights=[1, 1, 1]), dict(head_weights={"ctr": 1.0})):
        with pytest.raises(NotImplementedError, match="sharded"):
            sh.recommend_device(None, None, **kw)
        with pytest.raises(NotImplementedError, match="sharded"):
            sh.recommend_all(None, None, **kw)
    with pytest.raises(NotImplementedError, match="per-group caps"):     # in step with - behind - the cap and auction refusals
        sh.recommend_device(None, None, head_weights=[1, 1, 1], max_per_group=2)
    with pytest.raises(NotImplementedError, match="auction"):
        sh.recommend_device(None, None, head_weights=[1, 1, 1], rank_by="ecpm")


def test_the_micro_batcher_does_not_take_the_argument():
    import inspect
    from amdrec.serving import MicroBatcher
    for name, fn in inspect.getmembers(MicroBatcher, inspect.isfunction):
        assert "head_weights" not in inspect.signature(fn).parameters, name


# ---- the C entries ------------------------------------------------------------------------------------------------------------
def _header_arg_count(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_both_entries_are_bound_and_the_header_agrees_with_the_binding():
    lib = _lib.load()
    assert lib.amdrec_abi_version() == 14 == _lib.ABI_VERSION
    for name, n in (("amdrec_select_topk_value", 17), ("amdrec_select_topk_value_auction", 23)):
        assert name in _lib.exported_symbols()
        assert len(getattr(lib, name).argtypes) == n == len(_lib._SIGNATURES[name]) == _header_arg_count(name)
    assert _header_arg_count("amdrec_select_topk_auction") == len(_lib._SIGNATURES["amdrec_select_topk_auction"])
    src = open(HEADER).read()
    assert int(re.search(r"#define AMDREC_MAX_TASKS (\d+)", src).group(1)) == va.MAX_TASKS


def test_the_entries_refuse_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    raw = ctypes.create_string_buffer(4096 + 256)
    p = (ctypes.addressof(raw) + 255) // 256 * 256                         # non-null, aligned, never dereferenced

    def plain(n_tasks=3, ids=p, pos=p, users=1, k_c=500, top_k=10, w=p, groups=p, n_rows=100, cap=2, out=p, sc=p, values=p,
              ld=500, logits=p):
        return lib.amdrec_select_topk_value(logits, ld, n_tasks, ids, pos, users, k_c, top_k, w, groups, n_rows, cap, out, sc,
                                            None, values, None)

    def auction(n_tasks=3, rank=0, ids=p, pos=p, users=1, k_c=500, top_k=10, w=p, bids=p, n_bids=100, reserve=None, groups=p,
                n_rows=100, cap=2, out=p, sc=p, values=p, ecpm=p, price=p, ld=500, logits=p):
        return lib.amdrec_select_topk_value_auction(logits, ld, n_tasks, rank, ids, pos, users, k_c, top_k, w, bids, n_bids,
                                                    reserve, groups, n_rows, cap, out, sc, None, values, ecpm, price, None)
    for select in (plain, auction):
        assert select(n_tasks=0) == -1 and b"n_tasks=0" in lib.amdrec_last_error()
        assert select(n_tasks=5) == -1 and b"n_tasks=5" in lib.amdrec_last_error()
        assert select(k_c=0) == -1 and select(k_c=_lib.MAX_K + 1) == -1 and b"candidates" in lib.amdrec_last_error()
        assert select(top_k=0) == -1 and select(top_k=_lib.MAX_K + 1) == -1 and b"top_k" in lib.amdrec_last_error()
        assert select(cap=-1) == -1 and b"max_per_group=-1" in lib.amdrec_last_error()
        assert select(cap=_lib.MAX_K + 1) == -1 and b"max_per_group=2049" in lib.amdrec_last_error()
        assert select(n_rows=-1) == -1 and b"n_group_rows" in lib.amdrec_last_error()
        assert select(users=1 << 31) == -1 and b"n_users" in lib.amdrec_last_error()
        assert select(pos=None) == -1 and b"cand_pos" in lib.amdrec_last_error()
        assert select(w=None) == -1 and b"weights" in lib.amdrec_last_error()
        assert select(values=None) == -1 and b"out_values" in lib.amdrec_last_error()
        assert select(groups=None) == -1 and b"group_of" in lib.amdrec_last_error()      # required iff capped
        for kw in (dict(ids=None), dict(out=None), dict(sc=None), dict(logits=None)):
            assert select(**kw) == -1 and b"null pointer" in lib.amdrec_last_error()
        assert select(ld=499) == -1 and b"ld_logits" in lib.amdrec_last_error()
        assert select(users=0, ids=None, pos=None, w=None, groups=None, out=None, sc=None, values=None, logits=None) == 0
        assert select(users=-3, cap=0, groups=None) == 0                                  # no user: nothing to do
    assert auction(rank=3) == -1 and auction(rank=-1) == -1 and b"task" in lib.amdrec_last_error()
    assert auction(n_bids=-1) == -1 and b"n_bid_rows" in lib.amdrec_last_error()
    assert auction(bids=None) == -1 and b"bid_of" in lib.amdrec_last_error()
    assert auction(ecpm=None) == -1 and auction(price=None) == -1 and b"null pointer" in lib.amdrec_last_error()
    assert auction(users=0, bids=None, ecpm=None, price=None, pos=None, w=None, values=None) == 0
    del raw
