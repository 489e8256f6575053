"""CPU: the host side of auction ranking (amdrec.auction) - the oracle's self-checks, the guarantee that the GPU tests' seeds
exercise the rule, the host helpers, every refusal that must happen before the library is touched (and after the cap
refusals), bids in the index file and through growth, and the refusals of the C entry (before its first HIP call).  No GPU."""
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

from amdrec import _lib, auction as au
from tests import auction_oracle as ao
from tests import group_cap_oracle as go

K_CS = [1, 2, 63, 64, 65, 128, 129, 500, 512, 513, 2048]               # the GPU test's candidate counts
USERS, TOP_KS, CAPS = (1, 5, 9), (1, 10, 32, 33), (0, 1, 2)


def seed_for(n_users, k_c):
    return 1000 * n_users + k_c


def exercised(k_c, prob_of):
    """Over the GPU test's parametrisation for one k_c, with ``prob_of(logits, n_users)`` -> [n_users, k_c] probabilities:
    how often (eCPM order != CTR order, a reserve dropped a would-be winner, a cap changed the runner-up)."""
    reorder = dropped = runner_moved = 0
    for n_users in USERS:
        logits, ids, pos, group_of, bid_of = ao.inputs(n_users, k_c, seed_for(n_users, k_c))
        p = prob_of(logits, n_users)
        ones = np.ones_like(bid_of)
        for top_k in TOP_KS:
            base = ao.select_topk_auction(p, ids, pos, top_k, bid_of, len(bid_of), None, group_of, 0)
            ctr = ao.select_topk_auction(p, ids, pos, top_k, ones, len(ones), None, group_of, 0)
            reorder += int(not np.array_equal(base[1], ctr[1]))
            for kind in ao.RESERVE_KINDS[1:]:
                rv = ao.reserve_for(kind, n_users)
                for u in range(n_users):
                    won = base[1][u][base[1][u] >= 0]
                    dropped += int(any(not (base[2][u][r] >= rv[u]) for r in range(len(won))))
            for cap in CAPS[1:]:
                capped = ao.select_topk_auction(p, ids, pos, top_k, bid_of, len(bid_of), None, group_of, cap)
                runner_moved += int(not np.array_equal(capped[4], base[4]))
    return reorder, dropped, runner_moved


@pytest.mark.parametrize("k_c", [k for k in K_CS if k >= 8])
def test_the_gpu_tests_seeds_exercise_the_rule(k_c):
    got = exercised(k_c, lambda logits, n_users: ao.sigmoid(logits[0]).reshape(n_users, k_c))
    assert all(got), got


def _random_user(rng, k_c):
    p = ao.sigmoid(rng.choice(ao.VALUES, size=k_c))
    p[rng.random(k_c) < 0.1] = np.nan
    n_rows = 40
    pos = rng.integers(0, n_rows + 5, size=k_c).astype(np.int64)          # (>= n_rows: no bid of its own, no group)
    pos[rng.random(k_c) < 0.15] = -1
    return p, pos, rng.choice(ao.BIDS, size=n_rows), rng.choice(np.array([-1, 0, 7, 1 << 40], dtype=np.int64), size=n_rows)


@pytest.mark.parametrize("cap", [0, 1, 2, 50])
def test_oracle_self_checks(cap):
    rng = np.random.default_rng(50 + cap)
    for trial in range(60):
        k_c = int(rng.integers(1, 70))
        p, pos, bid_of, group_of = _random_user(rng, k_c)
        for reserve in (None, np.float32(0.0), np.float32(0.4), np.float32(9.0)):
            order, e, b = ao.accepted(p, pos, bid_of, len(bid_of), reserve, group_of, cap)
            assert all(pos[s] >= 0 for s in order) and len(set(order)) == len(order)
            # the order: e descending, slot ascending, NaN last; with a reserve nothing below it and no NaN
            fin = [s for s in order if not np.isnan(e[s])]
            assert order == fin + sorted(s for s in order if np.isnan(e[s]))
            assert all(e[x] > e[y] or (e[x] == e[y] and x < y) for x, y in zip(fin, fin[1:]))
            if reserve is not None:
                assert fin == order and all(e[s] >= reserve for s in order)
            # the greedy loop under a cap equals "in-group rank, then cut" over the uncapped order
            free, _, _ = ao.accepted(p, pos, bid_of, len(bid_of), reserve, group_of, 0)
            if cap:
                groups = [go.group_at(group_of, int(pos[s])) for s in free]
                assert order == [s for s, ok in zip(free, go.rank_form(groups, cap)) if ok]
            else:
                assert order == free
            for top_k in (1, 5, k_c + 3):
                slots, ecpm, price, runner = ao.results(order, e, b, p, reserve, top_k)
                n = min(top_k, len(order))
                assert slots.tolist() == order[:n] + [-1] * (top_k - n) and runner == (order[top_k] if len(order) > top_k else -1)
                assert (ecpm[n:] == 0).all() and (price[n:] == 0).all()
                for r in range(n):
                    s = slots[r]
                    if np.isnan(e[s]):
                        assert np.isnan(ecpm[r]) and np.isnan(price[r])
                        continue
                    assert ecpm[r].view(np.int32) == e[s].view(np.int32) and e[s] == b[s] * p[s]
                    assert 0 <= price[r] <= b[s]                                      # never above the winner's own bid
                    if reserve is not None:
                        assert ecpm[r] >= reserve
                    if b[s] == 0:
                        assert ecpm[r] == 0 and price[r] == 0
                if reserve is None and n and n == len(order) and not np.isnan(e[order[n - 1]]):
                    assert price[n - 1] == 0                                          # no runner-up, no reserve: free


def test_host_helpers():
    b = au.as_bids([0, -0.0, 0.5, 3], 4)
    assert b.dtype == np.float32 and b.tolist() == [0.0, 0.0, 0.5, 3.0] and not np.signbit(b).any()
    assert au.as_bids(np.array([1, 2], dtype=np.int32), 2).tolist() == [1.0, 2.0]
    assert au.as_bids(np.array([-0.0, 2.5], dtype=np.float64), 2).view(np.int32)[0] == 0
    assert au.as_bids(torch.tensor([4.0, 0.25], dtype=torch.float64), 2).tolist() == [4.0, 0.25]
    assert au.as_bids(torch.tensor([1, 7], dtype=torch.int16), 2).tolist() == [1.0, 7.0]
    assert au.as_bids([], 0).shape == (0,)
    nan, inf = float("nan"), float("inf")
    for bad, exc in (([True, False], TypeError), (torch.zeros(2, dtype=torch.bool), TypeError), (np.zeros(2, dtype=bool), TypeError),
                     (["1", "2"], TypeError), ([1.0, 2.0, 3.0], ValueError), (np.zeros(3, dtype=np.float32), ValueError),
                     (np.zeros((2, 1), dtype=np.float32), ValueError), ([1.0, nan], ValueError), ([inf, 1.0], ValueError),
                     ([1.0, -0.5], ValueError), (np.array([1e39, 1.0]), ValueError), (torch.tensor([nan, 1.0]), ValueError),
                     (torch.tensor([-1.0, 1.0]), ValueError)):
        with pytest.raises(exc, match="bids"):
            au.as_bids(bad, 2)
        with pytest.raises(exc, match="bids"):
            au.device_bids(bad, 2, "cpu")
    assert au.device_bids([1, 2], 2, "cpu").dtype == torch.float32
    assert au.check_rank_by(None) is False and au.check_rank_by("ctr") is False and au.check_rank_by("ecpm") is True
    for bad in ("revenue", "ECPM", 1, True):
        with pytest.raises(ValueError, match="rank_by"):
            au.check_rank_by(bad)
    assert au.check_reserve(None) is None and au.check_reserve(None, auction=False) is None
    assert au.check_reserve(0) == 0.0 and au.check_reserve(np.float32(0.5)) == 0.5 and au.check_reserve(2, 7) == 2.0
    t = torch.zeros(3)
    assert au.check_reserve(t, 3) is t and au.check_reserve(t) is t
    for bad in (-1, -0.001, nan, inf, 1e39, True, "1", [0.5]):
        with pytest.raises(ValueError, match="reserve"):
            au.check_reserve(bad)
    for bad in (torch.zeros(4), torch.zeros(3, dtype=torch.float64), torch.zeros((3, 1))):
        with pytest.raises(ValueError, match="reserve"):
            au.check_reserve(bad, 3)
    with pytest.raises(ValueError, match='needs rank_by="ecpm"'):
        au.check_reserve(0.5, auction=False)


def _bare_index(bids=None, groups=None):
    """An index object that was never constructed: no device, no library - only what the refusals look at."""
    from amdrec.index import FAISSIndex
    idx = object.__new__(FAISSIndex)
    idx.index_type, idx._groups, idx._tags = "Flat", groups, None
    if bids is not None:
        idx._bids = bids
    idx.dimension, idx.device, idx._n = 8, torch.device("cpu"), 3
    idx._default_ids_ok, idx._trained, idx.verbose = True, True, False
    return idx


def _no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))


def _entries(idx):
    from amdrec.pipeline import AdRecommenderInference, GraphedRecommender, TwoStageRetriever
    rec = object.__new__(AdRecommenderInference)
    rec.faiss_index, rec.heads_mode = idx, "all"
    two = object.__new__(TwoStageRetriever)
    two.faiss_index = idx
    return [lambda **kw: rec.recommend_device(None, None, **kw), lambda **kw: rec.recommend_tensors(None, None, **kw),
            lambda **kw: rec.batch_recommend([{}], **kw), lambda **kw: rec.recommend_ads({}, **kw),
            lambda **kw: two.retrieve_and_rank(None, None, **kw)], \
        [lambda **kw: rec.capture(2, **kw), lambda **kw: GraphedRecommender(rec, 2, 10, 500, **kw)]


def test_auction_refusals_come_before_the_library_and_after_the_cap_refusals(monkeypatch):
    from amdrec.sharded import ShardedRecommender
    _no_library(monkeypatch)
    calls, captures = _entries(_bare_index())                             # no bids (the attribute itself is missing), no groups
    for call in calls + captures:
        with pytest.raises(ValueError, match="without bids"):
            call(rank_by="ecpm")
        with pytest.raises(ValueError, match="rank_by"):
            call(rank_by="revenue")
        with pytest.raises(ValueError, match="without group keys"):      # the cap refusal still comes first
            call(rank_by="ecpm", max_per_group=2)
    for call in calls:
        for kw in (dict(reserve=0.5), dict(reserve=0.5, rank_by="ctr")):
            with pytest.raises(ValueError, match='needs rank_by="ecpm"'):
                call(**kw)
    for call in captures:
        with pytest.raises(ValueError, match='needs rank_by="ecpm"'):
            call(reserve=True)
    calls, _ = _entries(_bare_index(bids=torch.ones(3), groups=torch.zeros(3, dtype=torch.int64)))
    for call in calls:
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="reserve must be finite"):
                call(rank_by="ecpm", reserve=bad)
        with pytest.raises(ValueError, match=">= 1"):                    # the cap refusal first, here too
            call(rank_by="ecpm", reserve=-1.0, max_per_group=0)
    sh = object.__new__(ShardedRecommender)                               # the sharded path takes no auction at all
    for kw in (dict(rank_by="ecpm"), dict(reserve=0.5), dict(rank_by="ecpm", reserve=0.0)):
        with pytest.raises(NotImplementedError, match="sharded"):
            sh.recommend_device(None, None, **kw)
        with pytest.raises(NotImplementedError, match="sharded"):
            sh.recommend_all(None, None, **kw)


def test_bad_bids_are_refused_and_leave_the_index_as_it_was(monkeypatch):
    _no_library(monkeypatch)
    x = np.zeros((3, 8), dtype=np.float32)
    for bids in (None, torch.tensor([1.0, 2.0, 3.0])):
        idx = _bare_index(bids=bids)
        before = dict(idx.__dict__)
        for bad, exc in (([1, 2], ValueError), (np.zeros(4, dtype=np.float32), ValueError), ([1.0, float("nan"), 3.0], ValueError),
                         ([1.0, -2.0, 3.0], ValueError), ([1.0, float("inf"), 3.0], ValueError), ([True, False, True], TypeError)):
            with pytest.raises(exc, match="bids"):
                idx.add(x, bids=bad)
            with pytest.raises(exc, match="bids"):
                idx.set_bids(bad)
        assert idx.__dict__.keys() == before.keys() and all(idx.__dict__[k] is before[k] for k in before)
        if bids is not None:
            assert idx._bids.tolist() == [1.0, 2.0, 3.0]


def test_bids_in_the_index_file_through_growth_and_a_plain_file_loads_as_ever(tmp_path):
    """A Flat fp32 index on "cpu" allocates and saves without a kernel: rows are put in place by hand, the bids through
    set_bids."""
    from amdrec.index import FAISSIndex

    def index(n):
        idx = FAISSIndex(8, index_type="Flat", device="cpu", prefilter="fp32")
        idx._reserve(n)
        idx._xb[:n] = torch.eye(8)[:n]
        idx._ids[:n] = torch.arange(n)
        idx._n = n
        return idx

    def header(path):
        with open(path, "rb") as f:
            f.read(9)
            (hl,) = struct.unpack("<Q", f.read(8))
            return json.loads(f.read(hl).decode())
    bids = [0.0, 0.5, 3.0, 1.0, 2.25]
    idx = index(5)
    assert idx._bids is None and idx.get_bids().tolist() == [1.0] * 5 and len(idx.resident_tensors()) == 4
    idx.set_bids(bids)
    assert idx.get_bids().tolist() == bids and idx._bids.dtype == torch.float32
    assert any(t is idx._bids for t in idx.resident_tensors()) and len(idx.resident_tensors()) == 5
    old, snapshot = idx._bids, idx._bids.clone()
    idx.set_bids([-0.0] * 5)                                                # out of place; -0.0 is stored as +0.0
    assert idx._bids is not old and torch.equal(old, snapshot) and not torch.signbit(idx._bids[:5]).any()
    idx.set_bids(bids)
    path = str(tmp_path / "with_bids.bin")
    idx.save(path)
    assert [a["name"] for a in header(path)["arrays"]] == ["xb", "ids", "bids"]
    back = FAISSIndex(8, index_type="Flat", device="cpu", prefilter="fp32")
    back.load(path)
    assert back.get_bids().tolist() == bids and back._bids.dtype == torch.float32 and back.index.ntotal == 5
    idx.set_groups([3, -1, 3, 7, 9])
    idx.save(path)
    assert [a["name"] for a in header(path)["arrays"]] == ["xb", "ids", "groups", "bids"]
    back.load(path)
    assert back.get_bids().tolist() == bids and back.get_groups().tolist() == [3, -1, 3, 7, 9]
    idx._reserve(5000)                                                      # growth keeps the bids
    assert idx.get_bids().tolist() == bids and idx._bids.shape[0] >= 5000
    plain = str(tmp_path / "plain.bin")
    index(5).save(plain)
    assert [a["name"] for a in header(plain)["arrays"]] == ["xb", "ids"]   # the file every earlier build wrote
    back.load(plain)
    assert back._bids is None and back.get_bids().tolist() == [1.0] * 5


def test_the_auction_entry_is_bound_and_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    assert lib.amdrec_abi_version() == 14 == _lib.ABI_VERSION
    assert "amdrec_select_topk_auction" in _lib.exported_symbols()
    assert len(lib.amdrec_select_topk_auction.argtypes) == 21
    raw = ctypes.create_string_buffer(4096 + 256)
    p = (ctypes.addressof(raw) + 255) // 256 * 256                         # non-null, aligned, never dereferenced

    def select(n_tasks=3, rank=0, ids=p, pos=p, users=1, k_c=500, top_k=10, bids=p, n_bids=100, reserve=None, groups=p,
               n_rows=100, cap=2, out=p, ecpm=p, price=p, ld=500):
        return lib.amdrec_select_topk_auction(p, ld, n_tasks, rank, ids, pos, users, k_c, top_k, bids, n_bids, reserve, groups,
                                              n_rows, cap, out, p, None, ecpm, price, None)
    assert select(rank=5) == -1 and b"task" in lib.amdrec_last_error()
    assert select(n_tasks=0) == -1 and b"task" in lib.amdrec_last_error()
    assert select(k_c=0) == -1 and select(k_c=_lib.MAX_K + 1) == -1 and b"candidates" in lib.amdrec_last_error()
    assert select(top_k=0) == -1 and select(top_k=_lib.MAX_K + 1) == -1 and b"top_k" in lib.amdrec_last_error()
    assert select(cap=-1) == -1 and b"max_per_group=-1" in lib.amdrec_last_error()
    assert select(cap=_lib.MAX_K + 1) == -1 and b"max_per_group=2049" in lib.amdrec_last_error()
    assert select(n_bids=-1) == -1 and b"n_bid_rows" in lib.amdrec_last_error()
    assert select(n_rows=-1) == -1 and b"n_group_rows" in lib.amdrec_last_error()
    assert select(pos=None) == -1 and b"cand_pos" in lib.amdrec_last_error()
    assert select(bids=None) == -1 and b"bid_of" in lib.amdrec_last_error()
    assert select(groups=None) == -1 and b"group_of" in lib.amdrec_last_error()      # required iff capped
    assert select(ids=None) == -1 and select(out=None) == -1 and b"null pointer" in lib.amdrec_last_error()
    assert select(ecpm=None) == -1 and select(price=None) == -1 and b"null pointer" in lib.amdrec_last_error()
    assert select(ld=499) == -1 and b"ld_logits" in lib.amdrec_last_error()
    assert select(users=0, ids=None, pos=None, bids=None, groups=None, out=None, ecpm=None, price=None) == 0
    assert select(users=-3, cap=0, groups=None) == 0                                  # no user: nothing to do
    del raw
