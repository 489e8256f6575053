"""CPU: the host side of the per-group caps (amdrec.group_cap) - the oracle's greedy loop against the parallel "in-group rank
below the cap, then cut" form that the kernels implement, the host helpers, every refusal that must happen before the library
is touched, and the refusals of the two C entries (each returns before its first HIP call).  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from amdrec import _lib, group_cap as gc
from tests import group_cap_oracle as go


def _random_row(rng, k_c):
    """One user's candidates with everything the rule has to survive: logits from 5 values (heavy ties, both zeros), NaN
    logits, unfilled slots, and groups from 3 keys plus ungrouped (-1, -9) plus positions outside the group array."""
    logits = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 3.0], dtype=np.float32), size=k_c)
    logits[rng.random(k_c) < 0.1] = np.nan
    n_rows = 40
    group_of = rng.choice(np.array([-9, -1, 0, 7, 1 << 40], dtype=np.int64), size=n_rows)
    pos = rng.integers(0, n_rows + 5, size=k_c)                          # (>= n_rows: outside the array, ungrouped)
    pos[rng.random(k_c) < 0.15] = -1
    return logits, pos.astype(np.int64), group_of


@pytest.mark.parametrize("cap", [1, 2, 3, 50])
def test_greedy_loop_equals_in_group_rank_then_cut(cap):
    rng = np.random.default_rng(100 + cap)
    for trial in range(60):
        k_c = int(rng.integers(1, 70))
        logits, pos, group_of = _random_row(rng, k_c)
        order = go.select_order(logits, pos)
        assert all(pos[s] >= 0 for s in order) and len(order) == int((pos >= 0).sum())
        # the order itself: NaN last, ties by slot, the two zeros equal
        fin = [s for s in order if not np.isnan(logits[s])]
        assert order == fin + sorted(s for s in order if np.isnan(logits[s]))
        assert all(logits[a] > logits[b] or (logits[a] == logits[b] and a < b) for a, b in zip(fin, fin[1:]))
        groups = [go.group_at(group_of, int(pos[s])) for s in order]
        keep = go.greedy_keep(groups, cap)
        assert np.array_equal(keep, go.rank_form(groups, cap))
        for g in set(groups):
            n = sum(1 for x, ok in zip(groups, keep) if ok and x == g)
            assert n == (groups.count(g) if g < 0 else min(cap, groups.count(g)))
        # ... then cut: the selection's result is the first top_k of the kept ones, ids and slots, tail -1
        for top_k in (1, 5, k_c + 3):
            ids, slots = go.select_topk_capped(logits[None], (pos * 10 + 1)[None], pos[None], top_k, group_of, cap)
            won = [s for s, ok in zip(order, go.rank_form(groups, cap)) if ok][:top_k]
            assert slots[0].tolist() == won + [-1] * (top_k - len(won))
            assert ids[0].tolist() == [int(pos[s]) * 10 + 1 for s in won] + [-1] * (top_k - len(won))


def test_compact_oracle_keeps_unfilled_entries_and_never_counts_them():
    group_of = np.array([5, 5, 5, -1, 9, 9], dtype=np.int64)
    pos = np.array([[0, 1, 3, 2, 4, 77, 5, -1, -1]], dtype=np.int64)      # 77: outside the array, ungrouped
    sc = np.arange(9, dtype=np.float32)[None] * -1
    p, s = go.compact(pos, sc, group_of, 1, 9, np.float32(-np.inf))
    assert p[0].tolist() == [0, 3, 4, 77, -1, -1, -1, -1, -1]
    assert s[0].tolist()[:6] == [-0.0, -2.0, -4.0, -5.0, -7.0, -8.0] and np.isneginf(s[0, 6:]).all()
    p, s = go.compact(pos, sc, group_of, 2, 3, np.float32(np.inf))
    assert p[0].tolist() == [0, 1, 3]
    p, _ = go.compact(pos, sc, group_of, 9, 9, np.float32(np.inf))
    assert np.array_equal(p, pos)
    rng = np.random.default_rng(3)
    for _ in range(40):                                                  # the loop against the rank form, unfilled tails
        kc = int(rng.integers(1, 60))
        row = rng.integers(0, 8, size=kc).astype(np.int64)
        row[kc - int(rng.integers(0, kc + 1)):] = -1
        cap, k = int(rng.integers(1, 4)), int(rng.integers(1, kc + 1))
        p, _ = go.compact(row[None], np.zeros((1, kc), dtype=np.float32), group_of, cap, k, np.float32(0))
        groups = [go.group_at(group_of, int(x)) for x in row]
        kept = row[go.rank_form(groups, cap)][:k]
        assert p[0].tolist() == kept.tolist() + [-1] * (k - len(kept))


def test_host_helpers():
    assert gc.check_cap(1) == 1 and gc.check_cap(np.int64(7)) == 7 and gc.check_cap(10 ** 9) == _lib.MAX_K
    for bad in (0, -1, -(1 << 40)):
        with pytest.raises(ValueError, match=">= 1"):
            gc.check_cap(bad)
    for bad in (1.0, True, "2", None):
        with pytest.raises(TypeError):
            gc.check_cap(bad)
    assert gc.overfetch_k(500, 2) == 1000 and gc.overfetch_k(1500, 2) == 2048 and gc.overfetch_k(2048, 1) == 2048
    assert gc.overfetch_k(500, 2, 1548) == 500 and gc.overfetch_k(10, 3, 7) == 30
    with pytest.raises(ValueError, match="AMDREC_MAX_K = 2048"):
        gc.overfetch_k(500, 2, 1549)
    with pytest.raises(ValueError, match="AMDREC_MAX_K = 2048"):
        gc.overfetch_k(2049, 2)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="group_overfetch"):
            gc.overfetch_k(10, bad)
    k = gc.as_keys([3, -1, 1 << 62], 3)
    assert k.dtype == np.int64 and k.tolist() == [3, -1, 1 << 62]
    assert gc.as_keys(np.array([1, 2], dtype=np.int32), 2).dtype == np.int64
    assert gc.as_keys(torch.tensor([4, -5], dtype=torch.int16), 2).tolist() == [4, -5]
    assert gc.as_keys([], 0).shape == (0,)
    for bad, exc in (([1.0, 2.0], TypeError), (np.zeros(2, dtype=np.float32), TypeError), (torch.zeros(2), TypeError),
                     ([True, False], TypeError), (torch.zeros(2, dtype=torch.bool), TypeError), ([1, 2, 3], ValueError),
                     (np.zeros(3, dtype=np.int64), ValueError), (np.zeros((2, 1), dtype=np.int64), ValueError),
                     ([1 << 63, 0], ValueError), (np.array([1 << 63, 0], dtype=np.uint64), ValueError)):
        with pytest.raises(exc):
            gc.as_keys(bad, 2)


def _bare_index(groups=None, index_type="Flat"):
    """An index object that was never constructed: no device, no library - only what the refusals look at."""
    from amdrec.index import FAISSIndex
    idx = object.__new__(FAISSIndex)
    idx.index_type, idx._groups, idx._tags = index_type, groups, None
    idx.dimension, idx.device, idx._n = 8, torch.device("cpu"), 3
    idx._default_ids_ok, idx._trained, idx.verbose = True, True, False
    return idx


def _no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))


def test_a_cap_without_groups_and_a_cap_below_one_are_refused_before_the_library_is_touched(monkeypatch):
    from amdrec.pipeline import AdRecommenderInference, GraphedRecommender, TwoStageRetriever
    from amdrec.sharded import ShardedRecommender
    _no_library(monkeypatch)
    q = np.zeros((2, 8), dtype=np.float32)

    def entries(idx):
        rec = object.__new__(AdRecommenderInference)
        rec.faiss_index, rec.heads_mode = idx, "all"
        two = object.__new__(TwoStageRetriever)
        two.faiss_index = idx
        calls = []
        for name in ("max_per_group", "stage1_max_per_group"):
            calls += [lambda c, n=name: rec.recommend_device(None, None, **{n: c}),
                      lambda c, n=name: rec.recommend_tensors(None, None, **{n: c}),
                      lambda c, n=name: rec.batch_recommend([{}], **{n: c}),
                      lambda c, n=name: rec.recommend_ads({}, **{n: c}),
                      lambda c, n=name: rec.capture(2, **{n: c}),
                      lambda c, n=name: GraphedRecommender(rec, 2, 10, 500, **{n: c}),
                      lambda c, n=name: two.retrieve_and_rank(None, None, **{n: c})]
        return calls + [lambda c: idx.search_device(q, 3, max_per_group=c), lambda c: idx.search(q, 3, max_per_group=c),
                        lambda c: idx.batch_search(q, 3, max_per_group=c)]

    for call in entries(_bare_index(groups=None)):
        with pytest.raises(ValueError, match="without group keys"):
            call(2)
    for call in entries(_bare_index(groups=torch.zeros(3, dtype=torch.int64))):
        for bad in (0, -1):
            with pytest.raises(ValueError, match=">= 1"):
                call(bad)
        with pytest.raises(TypeError):
            call(2.0)
    # the sharded path takes no cap at all
    sh = object.__new__(ShardedRecommender)
    for kw in (dict(max_per_group=2), dict(stage1_max_per_group=1)):
        with pytest.raises(NotImplementedError, match="sharded"):
            sh.recommend_device(None, None, **kw)
        with pytest.raises(NotImplementedError, match="sharded"):
            sh.recommend_all(None, None, **kw)


def test_overfetch_below_k_is_refused_before_the_library_is_touched(monkeypatch):
    _no_library(monkeypatch)
    idx = _bare_index(groups=torch.zeros(3, dtype=torch.int64))
    q = torch.zeros((2, 8))
    with pytest.raises(ValueError, match=r"AMDREC_MAX_K - E = 548"):        # K1 = min(1200, 2048 - 1500) = 548 < 600
        idx.search_device(q, 600, exclude=torch.zeros((2, 1500), dtype=torch.int64), max_per_group=2)
    with pytest.raises(ValueError, match="AMDREC_MAX_K = 2048"):
        idx.search_device(q, 2049, max_per_group=2)
    with pytest.raises(ValueError, match="group_overfetch"):
        idx.search_device(q, 10, max_per_group=2, group_overfetch=0)


def test_bad_groups_are_refused_and_leave_the_index_as_it_was(monkeypatch):
    _no_library(monkeypatch)
    x = np.zeros((3, 8), dtype=np.float32)
    for groups in (None, torch.arange(3)):
        idx = _bare_index(groups=groups)
        before = dict(idx.__dict__)
        for bad, exc in (([1, 2], ValueError), (np.zeros(4, dtype=np.int64), ValueError), ([1.0, 2.0, 3.0], TypeError),
                         (np.zeros(3, dtype=np.float64), TypeError), (torch.zeros(3), TypeError)):
            with pytest.raises(exc, match="group keys"):
                idx.add(x, groups=bad)
            with pytest.raises(exc, match="group keys"):
                idx.set_groups(bad)
        assert idx.__dict__.keys() == before.keys() and all(idx.__dict__[k] is before[k] for k in before)
        if groups is not None:
            assert idx._groups.tolist() == [0, 1, 2]


def test_groups_survive_save_and_load_and_a_file_without_them_loads_as_ever(tmp_path):
    """A Flat fp32 index on "cpu" allocates and saves without a kernel (only add and search launch): rows are put in place
    by hand, the keys through set_groups."""
    import json
    import struct
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
    keys = [3, -1, 3, 7, 1 << 40]
    idx = index(5)
    assert idx._groups is None and idx.get_groups().tolist() == [-1] * 5 and len(idx.resident_tensors()) == 4
    idx.set_groups(keys)
    assert idx.get_groups().tolist() == keys and any(t is idx._groups for t in idx.resident_tensors())
    path = str(tmp_path / "with_groups.bin")
    idx.save(path)
    assert [a["name"] for a in header(path)["arrays"]] == ["xb", "ids", "groups"]
    back = FAISSIndex(8, index_type="Flat", device="cpu", prefilter="fp32")
    back.load(path)
    assert back.get_groups().tolist() == keys and back._groups.dtype == torch.int64 and back.index.ntotal == 5
    idx._reserve(5000)                                                      # growth keeps the keys
    assert idx.get_groups().tolist() == keys and idx._groups.shape[0] >= 5000
    plain = str(tmp_path / "plain.bin")
    index(5).save(plain)
    assert [a["name"] for a in header(plain)["arrays"]] == ["xb", "ids"]  # the file every earlier build wrote
    back.load(plain)
    assert back._groups is None and back.get_groups().tolist() == [-1] * 5


def _fake_pointer():
    raw = ctypes.create_string_buffer(4096 + 256)
    return raw, (ctypes.addressof(raw) + 255) // 256 * 256            # non-null, aligned, never dereferenced


def test_capped_entries_refuse_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    raw, p = _fake_pointer()

    def select(n_tasks=3, rank=0, ids=p, pos=p, users=1, k_c=500, top_k=10, out=p, groups=p, n_rows=100, cap=2, ld=500):
        return lib.amdrec_select_topk_capped(p, ld, n_tasks, rank, ids, pos, users, k_c, top_k, out, p, None, groups, n_rows,
                                             cap, None)
    assert select(rank=5) == -1 and b"task" in lib.amdrec_last_error()
    assert select(k_c=0) == -1 and select(k_c=_lib.MAX_K + 1) == -1 and b"candidates" in lib.amdrec_last_error()
    assert select(top_k=0) == -1 and select(top_k=_lib.MAX_K + 1) == -1 and b"top_k" in lib.amdrec_last_error()
    assert select(cap=0) == -1 and b"max_per_group=0" in lib.amdrec_last_error()
    assert select(cap=_lib.MAX_K + 1) == -1 and b"max_per_group=2049" in lib.amdrec_last_error()
    assert select(n_rows=-1) == -1 and b"n_group_rows" in lib.amdrec_last_error()
    assert select(pos=None) == -1 and b"cand_pos" in lib.amdrec_last_error()      # required here, optional in the uncapped one
    assert select(groups=None) == -1 and b"group_of" in lib.amdrec_last_error()
    assert select(ids=None) == -1 and select(out=None) == -1 and b"null pointer" in lib.amdrec_last_error()
    assert select(ld=499) == -1 and b"ld_logits" in lib.amdrec_last_error()
    assert select(users=0, ids=None, pos=None, groups=None) == 0                 # no user: nothing to do

    def compact(nq=1, kc=100, k=50, cap=2, pos=p, groups=p, n_rows=100, out=p):
        return lib.amdrec_group_cap_compact(pos, p, nq, kc, groups, n_rows, cap, k, float("-inf"), out, p, None)
    assert compact(kc=0) == -1 and compact(kc=_lib.MAX_K + 1) == -1 and b"kc=" in lib.amdrec_last_error()
    assert compact(k=0) == -1 and compact(k=101) == -1 and b"k=101" in lib.amdrec_last_error()
    assert compact(cap=0) == -1 and compact(cap=_lib.MAX_K + 1) == -1 and b"max_per_group" in lib.amdrec_last_error()
    assert compact(n_rows=-5) == -1 and b"n_group_rows" in lib.amdrec_last_error()
    assert compact(pos=None) == -1 and compact(out=None) == -1 and b"null pointer" in lib.amdrec_last_error()
    assert compact(groups=None) == -1 and b"group_of" in lib.amdrec_last_error()
    assert compact(nq=0, pos=None, groups=None, out=None) == 0                   # no query: nothing to do
    del raw
