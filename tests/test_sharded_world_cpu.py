"""The sharded-serving scenario table (tests/sharded_world.py) on the CPU engine, the launcher's containment, and the
float64 premises of the short-list scenarios.

World 3 runs every scenario that needs no device through gloo with the numpy ``OracleEngine`` and compares with the numpy
pipeline on the whole corpus, bit for bit: that the table's slices, exchange kinds, statistics and empty ranks are right is
settled here, so tests/test_sharded_world_gpu.py only has to add the device."""
import numpy as np
import pytest

from amdrec.sharded import short_list_k
from tests import sharded_world as sw

B, K1, TOPK = sw.B_MAIN, sw.K1, sw.TOPK


@pytest.fixture(scope="module")
def world3():
    res = sw.run_world(3, "oracle", sw.scenarios_for("oracle"), timeout_s=600)
    assert res.failure is None, res.failure
    return res


@pytest.fixture(scope="module")
def world4_d():
    res = sw.run_world(4, "oracle", ["d"], timeout_s=300)
    assert res.failure is None, res.failure
    return res


@pytest.fixture(scope="module")
def ref():
    cache = {}

    def get(variant="plain", B=B, nan_user=None):
        key = (variant, B, nan_user)
        if key not in cache:
            cache[key] = sw.oracle_unsharded(variant, B, nan_user)
        return cache[key]
    return get


def test_every_process_computes_the_same_corpus(world3):
    for rank in range(3):
        hello = world3[(rank, "(hello)")]
        assert hello == {"digest": sw.digest(), "backend": "gloo", "world": 3}
    assert world3.exitcodes == [0, 0, 0]


def test_a_b_full_lists_all_to_all_and_all_gather(world3, ref):
    sw.assert_equals_unsharded(world3, "a", 3, B, ref())
    sw.assert_equals_unsharded(world3, "b", 3, B, ref())
    for rank in range(3):
        assert world3[(rank, "a")]["last_exchange"] == {"kind": "all_to_all", "bytes_per_rank": B * K1 * 8, "list_k": K1}
        assert world3[(rank, "b")]["last_exchange"] == {"kind": "all_gather", "bytes_per_rank": B * K1 * 8, "list_k": K1}
        assert world3[(rank, "a")]["q0"] == 4 * rank
        for key in sw.KEYS:
            assert np.array_equal(world3[(rank, "a")][key], world3[(rank, "b")][key])


def test_c_ragged_batch_with_a_nan_user(world3, ref):
    r = ref(B=7, nan_user=3)
    assert (r["candidate_ids"][3] == -1).all() and np.isneginf(r["candidate_scores"][3]).all()
    assert (r["ad_ids"][3] == -1).all() and (r["scores"][:, 3] == 0.0).all()
    assert (r["candidate_ids"][[0, 1, 2, 4, 5, 6]] >= 0).all()
    sw.assert_equals_unsharded(world3, "c", 3, 7, r)
    assert [world3[(rank, "c")]["nq"] for rank in range(3)] == [3, 3, 1]
    assert all(world3[(rank, "c")]["last_exchange"]["kind"] == "all_gather" for rank in range(3))


@pytest.mark.parametrize("world", [3, 4])
def test_d_ranks_without_users(world, world3, world4_d, ref):
    res = world3 if world == 3 else world4_d
    sw.assert_equals_unsharded(res, "d", world, 2, ref(B=2))
    for rank in range(world):
        r = res[(rank, "d")]
        if rank >= 2:
            assert r["nq"] == 0 and r["ad_ids"].shape == (0, TOPK) and r["scores"].shape == (3, 0, TOPK)
            assert r["candidate_ids"].shape == (0, K1) and r["candidate_scores"].shape == (0, K1)
        assert "divisible" in r["all_error"] and "all_ad_ids" not in r          # on every rank, after the same collectives


def test_e_auto_short_lists_are_proven(world3, ref):
    sw.assert_equals_unsharded(world3, "e", 3, B, ref())
    for rank in range(3):
        r = world3[(rank, "e")]
        assert r["used_k"] == 256 == short_list_k(K1, 3) and r["shard_k_after"] == "auto"
        st = r["stats"]
        assert (st["batches"], st["unproven_queries"], st["repeated_batches"], st["hit_rate"]) == (1, 0, 0, 1.0)
        assert not st["switched_off"]
        assert r["last_exchange"] == {"kind": "all_to_all", "bytes_per_rank": B * 256 * 8, "list_k": 256}


def test_f_short_lists_on_a_sorted_corpus_are_repeated_with_full_lists(world3, ref):
    sw.assert_equals_unsharded(world3, "f", 3, B, ref("sorted"))
    counts = set()
    for rank in range(3):
        r = world3[(rank, "f")]
        st = r["stats"]
        assert r["used_k"] == sw.f_shard_k(3) == 174 and r["shard_k_after"] is None
        assert st["batches"] == 1 and st["repeated_batches"] == 1 and st["switched_off"]
        assert st["unproven_queries"] > 0.05 * B
        assert r["last_exchange"]["list_k"] == K1                               # the repeat ran with full lists
        f2 = world3[(rank, "f2")]
        assert f2["inexact_first"] == st["unproven_queries"] and f2["inexact_second"] == 0
        assert f2["last_exchange"]["list_k"] == 174 and f2["stats"]["batches"] == 0
        counts.add(f2["inexact_first"])
    assert len(counts) == 1 and counts.pop() > 0


def test_g_recommend_all(world3, ref):
    r = ref()
    for rank in range(3):
        g = world3[(rank, "g")]
        assert np.array_equal(g["ad_ids"], r["ad_ids"]) and np.array_equal(g["scores"], r["scores"])
        assert g["stats"]["batches"] == 1 and g["stats"]["repeated_batches"] == 0


def test_h_duplicated_ads_tie_by_global_position(world3, ref):
    r = ref("dup")
    h = sw.N_ADS // 2
    assert np.array_equal(r["candidate_ids"][:, 0::2] + h, r["candidate_ids"][:, 1::2])      # pairs: an ad, then its copy
    assert np.array_equal(r["candidate_scores"][:, 0::2], r["candidate_scores"][:, 1::2])
    sw.assert_equals_unsharded(world3, "h", 3, B, r)
    sw.assert_equals_unsharded(world3, "h_auto", 3, B, r)
    assert all(world3[(rank, "h_auto")]["used_k"] == 256 for rank in range(3))


def test_i_shards_and_corpus_smaller_than_stage1_k(world3, ref):
    r700, r300 = ref("n700"), ref("n300", B=7)
    assert (r700["candidate_ids"] >= 0).all()
    assert (r300["candidate_ids"][:, :300] >= 0).all() and (r300["candidate_ids"][:, 300:] == -1).all()
    assert np.isneginf(r300["candidate_scores"][:, 300:]).all()
    sw.assert_equals_unsharded(world3, "i700", 3, B, r700)
    sw.assert_equals_unsharded(world3, "i300", 3, 7, r300)


def test_m_refusals_come_before_any_collective(world3):
    for rank in range(3):
        m = world3[(rank, "m")]
        for tag in ("max_per_group", "ecpm", "reserve"):
            for fn in ("recommend_device", "recommend_all"):
                assert m[f"{tag}/{fn}"] == "NotImplementedError"
        assert m["collectives_during_refusals"] == [] and m["exchange_after_refusals"] is None
        assert m["ivfpq"] == "NotImplementedError"
    order = sw.scenarios_for("oracle")                                          # the scenarios behind m have all run
    assert order.index("m") < len(order) - 1 and all((rank, s) in world3.results for rank in range(3) for s in order)


def test_float64_truth_of_a_and_c_on_the_cpu_engine(world3):
    from tests import cases
    for sc, Bn, nan_user in (("a", B, None), ("c", 7, 3)):
        sw.assert_float64_truth(world3, sc, 3, Bn, "plain", nan_user, cases.SCORE_ATOL, cases.TOPK_TAU, 2 * cases.SCORE_ATOL)


@pytest.mark.parametrize("world,most,list_k", [(2, 267, 352), (3, 193, 256), (4, 144, 192)])
def test_float64_premises_of_e_and_f(world, most, list_k):
    """(e) may not repeat: under the contiguous split no user has more than ``most`` of its float64 top 500 on one shard,
    against lists of ``list_k``.  (f) must repeat: on the reordered corpus every user has a shard that holds MORE than
    ``shard_k`` of its top 500, so that shard's list is cut ahead of the merged 500th entry."""
    assert short_list_k(K1, world) == list_k
    plain = sw.top_rows_per_shard("plain", world)
    assert plain.sum(axis=1).tolist() == [K1] * B and plain.max() == most < list_k
    srt = sw.top_rows_per_shard("sorted", world)
    assert srt[0, 0] == K1                                                       # user 0: all of them on shard 0
    assert (srt.max(axis=1) > sw.f_shard_k(world)).all()
    assert sw.f_shard_k(world) * world >= K1 and sw.f_shard_k(world) < K1        # short lists are in force (list_k rule)


# ---- the launcher's containment (CPU engine only; a private flag keeps the real one clean) -------------------------------
def test_a_scenario_that_raises_on_one_rank_is_reported_and_every_child_is_gone():
    flag = sw.LaunchFlag()
    res = sw.run_world(2, "oracle", ["_raise_rank1", "a"], timeout_s=120, flag=flag)
    assert res.failure is not None and "rank 1, scenario '_raise_rank1'" in res.failure
    assert "rank 1 fails on request" in res.failure and "Traceback" in res.failure
    assert res.wall_s < 120 and all(c is not None for c in res.exitcodes) and res.exitcodes[1] == 1
    assert (0, "_raise_rank1") in res.results and (1, "a") not in res.results
    assert flag.reason is None and sw.NO_MORE_LAUNCHES.reason is None           # a Python error is no fault and no hang


def test_a_child_past_the_deadline_is_killed_and_nothing_is_launched_afterwards():
    """(The one test here that waits for a limit: the deadline IS what it is about; 8 s cover the children's start.)"""
    flag = sw.LaunchFlag()
    res = sw.run_world(2, "oracle", ["_sleep"], timeout_s=8, flag=flag)
    assert res.failure is not None and "deadline" in res.failure
    assert all(c is not None and c < 0 for c in res.exitcodes)                  # terminated: every child is gone
    assert flag.reason is not None and sw.NO_MORE_LAUNCHES.reason is None
    again = sw.run_world(2, "oracle", ["a"], timeout_s=120, flag=flag)
    assert again.failure.startswith("not started") and again.exitcodes == [] and again.wall_s == 0.0


def test_the_device_engine_refuses_the_containment_scenarios():
    with pytest.raises(ValueError):
        sw.run_world(2, "hip", ["_sleep"], timeout_s=5, flag=sw.LaunchFlag())
    with pytest.raises(ValueError):
        sw.run_world(5, "oracle", ["a"], timeout_s=5, flag=sw.LaunchFlag())
