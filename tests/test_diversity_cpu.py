"""CPU: the host side of the diversified selection (amdrec.diversity) - the rule module on hand-made cases and against the
float64 oracle of tests/diversity_oracle.py, the binding, every refusal of the C entry (each returns before a HIP call), the
Python refusals that happen before the library is touched, and the oracle's forced share on the GPU tests' inputs.  No GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from amdrec import _lib, diversity as dv
from tests import diversity_oracle as do

ROOT = Path(__file__).resolve().parent.parent


def _unit(*rows):
    x = np.asarray(rows, dtype=np.float64)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _run(logits, pos, rows, lam, pool, top_k, group_of=None, cap=0):
    logits, pos = np.asarray(logits, dtype=np.float32)[None], np.asarray(pos, dtype=np.int64)[None]
    slots, values = dv.select_diverse(logits, pos, rows, lam, pool, top_k, group_of, cap)
    o_slots, o_values, _, _ = do.select(logits, dv.sigmoid_f32(logits), pos, rows, lam, pool, top_k, group_of, cap)
    assert slots.tolist() == o_slots.tolist() and np.allclose(values, o_values, rtol=0, atol=1e-12, equal_nan=True)
    return slots[0].tolist(), values[0]


def test_the_rule_on_hand_made_cases():
    rows = _unit([1, 0, 0], [1, 0, 0], [0, 1, 0], [0.6, 0.8, 0], [0, 0, 1])
    # an exact duplicate of the winner at lam = 1 drops behind a less relevant but dissimilar ad
    slots, values = _run([2.0, 1.9, 0.5, -1.0], [0, 1, 2, 4], rows, 1.0, 4, 4)
    assert slots == [0, 2, 3, 1] and values[3] == 0.0
    p = dv.sigmoid_f32(np.float32([2.0, 0.5, -1.0]))
    assert values[:3].tolist() == [float(x) for x in p]                    # orthogonal rows: no discount
    # lam = 0 is the plain order, ties by slot, the two zeros equal
    assert _run([0.0, 2.0, -0.0, 2.0], [0, 1, 2, 3], rows, 0.0, 4, 4)[0] == [1, 3, 0, 2]
    # a partial discount: 0.6 similarity at lam = 0.5 scales by 0.7
    slots, values = _run([1.0, 0.9], [0, 3], rows, 0.5, 2, 2)
    assert slots == [0, 1] and abs(values[1] - float(dv.sigmoid_f32(0.9)) * (1 - 0.5 * 0.6)) < 1e-7
    # a negative similarity does not discount
    neg = _unit([1, 0], [-1, 0])
    assert _run([1.0, 0.5], [0, 1], neg, 1.0, 2, 2)[1].tolist() == [float(x) for x in dv.sigmoid_f32(np.float32([1.0, 0.5]))]
    # cap, then pool: groups [7, 7, 7, -1, 9] under cap 1 accept slots 0, 3, 4; a pool of 2 holds slots 0 and 3 only
    groups = np.array([7, 7, 7, -1, 9], dtype=np.int64)
    assert _run([5, 4, 3, 2, 1], [0, 1, 2, 3, 4], rows, 0.5, 2, 2, groups, 1)[0] == [0, 3]
    # (slot 3's row is 0.6 similar to the winner's: sigmoid(2) * 0.7 < sigmoid(1), so slot 4 overtakes it)
    assert _run([5, 4, 3, 2, 1], [0, 1, 2, 3, 4], rows, 0.5, 5, 5, groups, 1)[0] == [0, 4, 3, -1, -1]
    # a NaN logit is last in the relevance order and its NaN value ranks after every other, unfilled slots are no candidates
    slots, values = _run([np.nan, 1.0, 3.0, 0.5], [0, 2, -1, 4], rows, 1.0, 4, 4)
    assert slots == [1, 3, 0, -1] and np.isnan(values[2]) and values[3] == 0.0
    # a NaN row gives no discount, to itself or to others; a position beyond the rows is never read: similarity 0
    nan_rows = rows.copy()
    nan_rows[1, 0] = np.nan
    assert _run([2.0, 1.9, 1.8], [0, 1, 0], nan_rows, 1.0, 3, 3)[0] == [0, 1, 2]
    assert _run([2.0, 1.9, 1.8], [0, 99, 0], rows, 1.0, 3, 3)[0] == [0, 1, 2]
    # a pool smaller than the candidate count never admits a non-pool ad, however dissimilar
    slots, _ = _run([3.0, 2.9, 2.8, 2.7], [0, 1, 1, 4], rows, 1.0, 3, 3)
    assert sorted(slots) == [0, 1, 2] and slots[0] == 0
    # short tail
    slots, values = _run([1.0, 2.0], [0, -1], rows, 0.3, 8, 5)
    assert slots == [0, -1, -1, -1, -1] and values[1:].tolist() == [0.0] * 4


def test_the_module_reference_equals_the_oracle_and_rank_zero_is_the_most_relevant():
    for k_c in (7, 65, 500):
        for top_k, pool, dim, n_users, _, lam, cap, seed in do.direct_cases(k_c):
            logits, _, pos, group_of = do.direct_inputs(n_users, k_c, seed)
            rank = logits[0].reshape(n_users, k_c)
            rows = do.corpus(dim)
            slots, values = dv.select_diverse(rank, pos, rows, lam, pool, top_k, group_of, cap)
            o_slots, o_values, _, _ = do.select(rank, dv.sigmoid_f32(rank), pos, rows, lam, pool, top_k, group_of, cap)
            assert np.array_equal(slots, o_slots) and np.allclose(values, o_values, rtol=0, atol=1e-12, equal_nan=True)
            for u in range(n_users):
                members = do.pool_slots(rank[u], pos[u], pool, group_of, cap)
                assert slots[u, 0] == (members[0] if members else -1)
                # lam = 0: the pool's own order
                plain, _ = dv.select_diverse(rank[u:u + 1], pos[u:u + 1], rows, 0.0, pool, top_k, group_of, cap)
                assert plain[0].tolist() == (members + [-1] * top_k)[:top_k]


@pytest.mark.parametrize("k_c", do.K_CS)
def test_the_gpu_tests_inputs_force_at_least_95_percent_of_the_rounds(k_c):
    rounds = forced = 0
    for top_k, pool, dim, n_users, _, lam, cap, seed in do.direct_cases(k_c):
        logits, _, pos, group_of = do.direct_inputs(n_users, k_c, seed)
        rank = logits[0].reshape(n_users, k_c)
        _, _, n, f = do.select(rank, dv.sigmoid_f32(rank), pos, do.corpus(dim), lam, pool, top_k, group_of, cap)
        rounds, forced = rounds + n, forced + f
    assert rounds and forced >= do.MIN_FORCED * rounds, (forced, rounds)


def test_the_walk_along_checker_accepts_the_rule_and_rejects_its_neighbours():
    """The checker's own power: the pure oracle's result passes; the same result under another lam, with two winners swapped,
    with a non-pool ad, with a repeated ad, or with values of the wrong round does not."""
    k_c, top_k, pool, dim, n_users, lam = 500, 10, 64, 256, 4, 0.7
    logits, _, pos, _ = do.direct_inputs(n_users, k_c, 123)
    rank, rows = logits[0].reshape(n_users, k_c), do.corpus(dim)
    rel = dv.sigmoid_f32(rank)
    slots, values, rounds, forced = do.select(rank, rel, pos, rows, lam, pool, top_k)
    assert do.check(slots, values, rank, rel, pos, rows, lam, pool, top_k) == (rounds, forced) and forced == rounds
    plain, plain_values, _, _ = do.select(rank, rel, pos, rows, 0.0, pool, top_k)
    assert not np.array_equal(plain, slots)                                  # the discount does re-order these users
    outside = do.pool_slots(rank[0], pos[0], pool + 1)[-1]

    def edited(fn):
        s, v = slots.copy(), values.copy()
        fn(s, v)
        return s, v
    wrong = {
        "the plain order": (plain, plain_values),
        "swapped winners": edited(lambda s, v: s.__setitem__((0, [2, 3]), s[0, [3, 2]])),
        "a non-pool ad": edited(lambda s, v: s.__setitem__((0, top_k - 1), outside)),
        "a repeated ad": edited(lambda s, v: s.__setitem__((0, 5), s[0, 1])),
        "a value off by a part in 10^5": edited(lambda s, v: v.__setitem__((1, 4), v[1, 4] * (1 + 1e-5))),
        "a short tail": edited(lambda s, v: (s.__setitem__((2, top_k - 1), -1), v.__setitem__((2, top_k - 1), 0.0))),
    }
    for what, (s, v) in wrong.items():
        with pytest.raises(AssertionError):
            do.check(s, v, rank, rel, pos, rows, lam, pool, top_k, what=what)
    with pytest.raises(AssertionError):
        do.check(slots, values, rank, rel, pos, rows, 0.69, pool, top_k, what="another lam")


def test_binding_is_declared_and_exported():
    assert "amdrec_select_topk_diverse" in _lib.exported_symbols()
    header = (ROOT / "include" / "amdrec.h").read_text()
    m = re.search(r"int amdrec_select_topk_diverse\((.*?)\);", header, re.S)
    assert m is not None
    args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
    assert len(args) == len(_lib._SIGNATURES["amdrec_select_topk_diverse"]) == 23
    assert hasattr(_lib.load(), "amdrec_select_topk_diverse")


def test_the_entry_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    raw = ctypes.create_string_buffer(4096 + 256)
    p = (ctypes.addressof(raw) + 255) // 256 * 256                        # non-null, aligned, never dereferenced

    def call(n_tasks=3, rank=0, ids=p, pos=p, users=1, k_c=500, top_k=10, rows=p, n_rows=100, ld_rows=256, dim=256, lam=0.5,
             pool=64, groups=None, n_group_rows=0, cap=0, out=p, values=p, ld=500, logits=p):
        return lib.amdrec_select_topk_diverse(logits, ld, n_tasks, rank, ids, pos, users, k_c, top_k, rows, n_rows, ld_rows, dim,
                                              lam, pool, groups, n_group_rows, cap, out, p, None, values, None)

    def refused(needle, **kw):
        assert call(**kw) == -1, kw
        assert needle in lib.amdrec_last_error(), (kw, lib.amdrec_last_error())
    refused(b"task", rank=3)
    refused(b"task", n_tasks=0)
    refused(b"candidates", k_c=0)
    refused(b"candidates", k_c=_lib.MAX_K + 1)
    refused(b"pool=0", pool=0, top_k=1)
    refused(b"pool=129", pool=129)
    refused(b"top_k=0", top_k=0)
    refused(b"top_k=65", top_k=65)                                          # above the pool
    refused(b"dim=0", dim=0)
    refused(b"ld_rows=255", ld_rows=255)
    refused(b"pool * dim = 32896", pool=128, dim=257, ld_rows=257)
    for bad in (-0.01, 1.01, float("nan"), float("inf"), float("-inf")):
        refused(b"lam=", lam=bad)
    refused(b"n_rows", n_rows=-1)
    refused(b"max_per_group=-1", cap=-1)
    refused(b"max_per_group=2049", cap=_lib.MAX_K + 1)
    refused(b"n_group_rows", n_group_rows=-1)
    refused(b"cand_pos", pos=None)
    refused(b"rows", rows=None)
    refused(b"group_of", cap=2, groups=None, n_group_rows=5)
    for name in ("ids", "out", "values", "logits"):
        refused(b"null pointer", **{name: None})
    refused(b"ld_logits", ld=499)
    refused(b"n_users", users=1 << 31)
    # no user: nothing to do, whatever the pointers; the limits themselves are fine
    assert call(users=0, ids=None, pos=None, rows=None, out=None, values=None, logits=None) == 0
    assert call(users=-3, logits=None) == 0
    assert call(users=0, k_c=0) == -1                                      # (the scalars are still checked)
    del raw


def _bare_index(index_type="Flat", dim=256, bids=None, groups=None):
    """An index object that was never constructed: no device, no library - only what the refusals look at."""
    from amdrec.index import FAISSIndex
    idx = object.__new__(FAISSIndex)
    idx.index_type, idx._groups, idx._tags, idx._bids = index_type, groups, None, bids
    idx.dimension, idx.device, idx._n = dim, torch.device("cpu"), 3
    idx._default_ids_ok, idx._trained, idx.verbose = True, True, False
    return idx


def _entries(idx):
    from amdrec.pipeline import AdRecommenderInference, GraphedRecommender, TwoStageRetriever
    rec = object.__new__(AdRecommenderInference)
    rec.faiss_index, rec.heads_mode = idx, "all"
    two = object.__new__(TwoStageRetriever)
    two.faiss_index = idx
    return [lambda **kw: rec.recommend_device(None, None, **kw),
            lambda **kw: rec.recommend_tensors(None, None, **kw),
            lambda **kw: rec.batch_recommend([{}], **kw),
            lambda **kw: rec.recommend_ads({}, **kw),
            lambda **kw: rec.capture(2, **kw),
            lambda **kw: GraphedRecommender(rec, 2, 10, 500, **kw),
            lambda **kw: two.retrieve_and_rank(None, None, **kw)]


def test_bad_diversity_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    for call in _entries(_bare_index()):
        for bad in ("0.5", [0.5], True, torch.tensor(0.5)):
            with pytest.raises(TypeError, match="diversity"):
                call(diversity=bad)
        for bad in (-0.1, 1.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=r"in \[0, 1\]"):
                call(diversity=bad)
        with pytest.raises(ValueError, match="smaller than top_k"):
            call(diversity=0.5, diversity_pool=9)                            # top_k (stage2_k) is 10 everywhere
        with pytest.raises(ValueError, match="exceeds 128"):
            call(diversity=0.5, diversity_pool=129)
        with pytest.raises(ValueError, match="without diversity"):
            call(diversity_pool=32)
        with pytest.raises(TypeError, match="diversity_pool"):
            call(diversity=0.5, diversity_pool=64.0)
    for call in _entries(_bare_index(dim=512)):
        with pytest.raises(ValueError, match="exceeds 32768"):
            call(diversity=0.5, diversity_pool=128)                          # 128 * 512
    for call in _entries(_bare_index(bids=torch.ones(3))):
        with pytest.raises(ValueError, match="ecpm"):
            call(diversity=0.5, rank_by="ecpm")
    for call in _entries(_bare_index(index_type="IVFPQ")):
        with pytest.raises(NotImplementedError, match="IVFPQ"):
            call(diversity=0.5)


def test_check_diversity_returns_what_the_entry_takes():
    assert dv.check_diversity(None, 64, 10, 256) is None
    assert dv.check_diversity(0, 64, 10, 256) == (0.0, 64)
    assert dv.check_diversity(np.float32(0.5), np.int64(10), 10, 256) == (0.5, 10)
    assert dv.check_diversity(1, 128, 128, 256, "IVF") == (1.0, 128)
    # the sharded recommender and the micro-batcher do not take the arguments
    import inspect
    from amdrec.serving import MicroBatcher
    from amdrec.sharded import ShardedRecommender
    for fn in (ShardedRecommender.recommend_device, ShardedRecommender.recommend_all, MicroBatcher.__init__):
        assert "diversity" not in inspect.signature(fn).parameters
