"""GPU: the shipped sharded composition - ShardedRecommender + HipEngine at world 2, 3 and 4 - against the unsharded pipeline.

Several ranks share ``cuda:0`` and meet over gloo (tests/sharded_world.py; the mechanism of bench.py's rehearsal), so what
runs is ``HipEngine.local_search`` with ``pos_offset``, the int64 -> int32 wire format on device uint8 views, the
host-staged exchange, the merge kernels on real search output at ``q0 > 0``, ``_stage2(ids_are_positions=True)`` on the
replicated ad table, the device proof counter and its staged all-reduce, the repeat with full lists, ``recommend_all``, the
StageTimer on HIP events and ``share_ivf_centroids`` with device tensors.  One launch per world; every test reads its cached
result.  The reference is the parent's own UNSHARDED ``recommend_device`` on the whole corpus and batch, compared bit for
bit; (a) and (c) are also held against float64 truth, since two code paths agreeing is not yet the truth.  What the table's
statistics, slices and exchange kinds must be is proven on the CPU engine in tests/test_sharded_world_cpu.py.

Not covered (needs more than one GPU): RCCL collectives at world > 1, the asynchronous proof read across real ranks, xGMI."""
import numpy as np
import pytest
import torch

from amdrec.sharded import STAGES, short_list_k, user_slice
from tests import cases
from tests import sharded_world as sw

pytestmark = pytest.mark.gpu

B, K1, TOPK, N = sw.B_MAIN, sw.K1, sw.TOPK, sw.N_ADS
WORLDS = (2, 3, 4)
_RUNS = {}                         # world -> WorldResult: one launch per world, whatever became of it


@pytest.fixture(scope="module", params=WORLDS)
def run(request):
    world = request.param
    if world not in _RUNS:
        _RUNS[world] = sw.run_world(world, "hip", sw.scenarios_for("hip"), timeout_s=420)
        print(f"sharded world {world}: run_world took {_RUNS[world].wall_s:.1f} s; rank 0 spent "
              f"{_RUNS[world].results.get((0, '(spent)'))}")
    res = _RUNS[world]
    assert res.failure is None, res.failure
    return world, res


@pytest.fixture(scope="module")
def models():
    return sw.hip_models()


@pytest.fixture(scope="module")
def ref(models):
    """The unsharded device pipeline, once per (corpus, batch)."""
    cache = {}

    def get(variant="plain", B=B, nan_user=None):
        key = (variant, B, nan_user)
        if key not in cache:
            cache[key] = sw.hip_unsharded(models, variant, B, nan_user)
        return cache[key]
    return get


def test_every_rank_is_a_gloo_rank_on_the_same_inputs(run):
    world, res = run
    for rank in range(world):
        assert res[(rank, "(hello)")] == {"digest": sw.digest(), "backend": "gloo", "world": world}
    assert res.exitcodes == [0] * world


def test_a_b_full_lists_all_to_all_and_all_gather(run, ref):
    world, res = run
    sw.assert_equals_unsharded(res, "a", world, B, ref())
    sw.assert_equals_unsharded(res, "b", world, B, ref())
    for rank in range(world):
        a, b = res[(rank, "a")], res[(rank, "b")]
        assert a["q0"] == rank * (B // world) and a["used_k"] == K1
        assert a["last_exchange"] == {"kind": "all_to_all", "bytes_per_rank": B * K1 * 8, "list_k": K1}
        assert b["last_exchange"] == {"kind": "all_gather", "bytes_per_rank": B * K1 * 8, "list_k": K1}
        for key in sw.KEYS:
            assert np.array_equal(a[key], b[key]), (rank, key)


def test_c_ragged_batch_with_a_nan_user(run, ref):
    world, res = run
    r = ref(B=7, nan_user=3)
    assert (r["candidate_ids"][3] == -1).all() and np.isneginf(r["candidate_scores"][3]).all()
    assert (r["ad_ids"][3] == -1).all() and (r["scores"][:, 3] == 0.0).all()
    others = [0, 1, 2, 4, 5, 6]
    assert (r["candidate_ids"][others] >= 0).all() and (r["ad_ids"][others] >= 0).all()
    sw.assert_equals_unsharded(res, "c", world, 7, r)
    assert [res[(rank, "c")]["nq"] for rank in range(world)] == {2: [4, 3], 3: [3, 3, 1], 4: [2, 2, 2, 1]}[world]
    for rank in range(world):
        assert res[(rank, "c")]["last_exchange"] == {"kind": "all_gather", "bytes_per_rank": 7 * K1 * 8, "list_k": K1}


def test_d_ranks_without_users(run, ref):
    world, res = run
    r = ref(B=2)
    sw.assert_equals_unsharded(res, "d", world, 2, r)
    for rank in range(world):
        d = res[(rank, "d")]
        assert (d["q0"], d["nq"]) == user_slice(2, rank, world)
        if rank >= 2:
            assert d["ad_ids"].shape == (0, TOPK) and d["scores"].shape == (3, 0, TOPK)
            assert d["candidate_ids"].shape == (0, K1) and d["candidate_scores"].shape == (0, K1)
        if world == 2:
            assert np.array_equal(d["all_ad_ids"], r["ad_ids"]) and np.array_equal(d["all_scores"], r["scores"])
        else:                      # raised on every rank, after the same collectives (or the next scenario would have hung)
            assert "divisible" in d["all_error"] and "all_ad_ids" not in d


def test_e_auto_short_lists_are_proven(run, ref):
    world, res = run
    k = {2: 352, 3: 256, 4: 192}[world]
    assert short_list_k(K1, world) == k
    sw.assert_equals_unsharded(res, "e", world, B, ref())
    for rank in range(world):
        e = res[(rank, "e")]
        st = e["stats"]
        assert e["used_k"] == k and e["shard_k_after"] == "auto"
        assert (st["batches"], st["unproven_queries"], st["repeated_batches"], st["hit_rate"]) == (1, 0, 0, 1.0)
        assert not st["switched_off"]
        assert e["last_exchange"] == {"kind": "all_to_all", "bytes_per_rank": B * k * 8, "list_k": k}


def test_f_unproven_short_lists_are_counted_summed_and_repeated_with_full_lists(run, ref):
    world, res = run
    k = sw.f_shard_k(world)
    sw.assert_equals_unsharded(res, "f", world, B, ref("sorted"))
    counts = set()
    for rank in range(world):
        f, f2 = res[(rank, "f")], res[(rank, "f2")]
        st = f["stats"]
        assert f["used_k"] == k and f["shard_k_after"] is None
        assert st["batches"] == 1 and st["repeated_batches"] == 1 and st["switched_off"]
        assert st["unproven_queries"] > 0.05 * B
        assert f["last_exchange"] == {"kind": "all_to_all", "bytes_per_rank": B * K1 * 8, "list_k": K1}
        # f2, verify=False: the short-list result stands, the caller reads the count - the sum over the ranks, on every rank
        assert f2["inexact_first"] == st["unproven_queries"] and f2["inexact_second"] == 0
        assert f2["last_exchange"]["list_k"] == k and f2["stats"]["batches"] == 0 and f2["shard_k_after"] == k
        counts.add(f2["inexact_first"])
    assert len(counts) == 1 and counts.pop() > 0


def test_g_recommend_all(run, ref):
    world, res = run
    r = ref()
    for rank in range(world):
        g = res[(rank, "g")]
        assert g["ad_ids"].dtype == np.int64 and g["scores"].dtype == np.float32
        assert np.array_equal(g["ad_ids"], r["ad_ids"]) and np.array_equal(g["scores"], r["scores"])
        assert g["stats"]["batches"] == 1 and g["stats"]["repeated_batches"] == 0


def test_h_duplicated_ads_tie_by_global_position(run, ref):
    world, res = run
    r = ref("dup")
    h = N // 2
    # premise: every candidate comes with its copy at the same score, the k-th place included
    srt = np.sort(r["candidate_ids"] % h, axis=1)
    assert np.array_equal(srt[:, 0::2], srt[:, 1::2])
    assert np.array_equal(r["candidate_scores"][:, K1 - 1], r["candidate_scores"][:, K1 - 2])
    sw.assert_equals_unsharded(res, "h", world, B, r)
    sw.assert_equals_unsharded(res, "h_auto", world, B, r)
    assert all(res[(rank, "h_auto")]["used_k"] == short_list_k(K1, world) for rank in range(world))


def test_i_shards_and_corpus_smaller_than_stage1_k(run, ref):
    world, res = run
    r700, r300 = ref("n700"), ref("n300", B=7)
    assert (r700["candidate_ids"] >= 0).all()
    assert (r300["candidate_ids"][:, :300] >= 0).all() and (r300["candidate_ids"][:, 300:] == -1).all()
    assert np.isneginf(r300["candidate_scores"][:, 300:]).all() and np.isfinite(r300["candidate_scores"][:, :300]).all()
    assert (r300["ad_ids"] >= 0).all()                                           # top_k < N: no tail here
    sw.assert_equals_unsharded(res, "i700", world, B, r700)
    sw.assert_equals_unsharded(res, "i300", world, 7, r300)
    assert res[(0, "i700")]["last_exchange"]["kind"] == "all_to_all"             # -1 slots inside the shard lists on both wires
    assert res[(0, "i300")]["last_exchange"]["kind"] == "all_gather"


def test_j_ctr_first_heads(run, ref):
    world, res = run
    sw.assert_equals_unsharded(res, "j", world, B, ref())                        # (the reference ran heads="all")
    assert all(res[(rank, "j")]["heads_effective"] == "ctr_first" for rank in range(world))


def test_k_ivf_with_shared_centroids(run, models):
    from amdrec.index import FAISSIndex
    world, res = run
    corpus, _ = sw.corpus_variant("plain")
    cent = res[(0, "k")]["centroids"]
    assert cent.shape == (sw.IVF_NLIST, 256) and cent.dtype == np.float32
    for rank in range(world):
        k = res[(rank, "k")]
        assert k["centroids"].tobytes() == cent.tobytes() and k["centroids_installed"].tobytes() == cent.tobytes()
    lo, hi = sw.shard_rows(N, 0, world)
    own = FAISSIndex(256, index_type="IVF", nlist=sw.IVF_NLIST, nprobe=sw.IVF_NPROBE)
    own.train(corpus[lo:hi])                                                     # training is bit-reproducible
    assert own.centroids.cpu().numpy().tobytes() == cent.tobytes()
    whole = FAISSIndex(256, index_type="IVF", nlist=sw.IVF_NLIST, nprobe=sw.IVF_NPROBE)
    whole.set_trained_centroids(torch.from_numpy(cent))
    r = sw.hip_unsharded(models, "plain", B, index=whole)
    assert (r["candidate_ids"] >= 0).any(axis=1).all()
    sw.assert_equals_unsharded(res, "k", world, B, r)


def test_l_stage_timer_on_hip_events(run, ref):
    world, res = run
    sw.assert_equals_unsharded(res, "l", world, B, ref())
    for rank in range(world):
        t = res[(rank, "l")]
        assert set(t["report"]) == set(STAGES) == set(t["stages"]) and len(t["report"]) == len(STAGES) and t["steps"] == 2
        assert all(t["report"][s] > 0 for s in ("tower", "search", "exchange", "merge", "ranker", "select")), t["report"]
        assert all(v >= 0 for v in t["report"].values()) and t["plain_equal"]


def test_m_refusals_come_before_any_collective(run):
    world, res = run
    for rank in range(world):
        m = res[(rank, "m")]
        for tag in ("max_per_group", "ecpm", "reserve"):
            for fn in ("recommend_device", "recommend_all"):
                assert m[f"{tag}/{fn}"] == "NotImplementedError"
        assert m["collectives_during_refusals"] == [] and m["exchange_after_refusals"] is None
        assert m["ivfpq"] == "NotImplementedError"


@pytest.mark.parametrize("scenario,Bn,nan_user", [("a", B, None), ("c", 7, 3)])
def test_candidates_against_float64_truth(run, scenario, Bn, nan_user):
    world, res = run
    sw.assert_float64_truth(res, scenario, world, Bn, "plain", nan_user, score_atol=cases.SCORE_ATOL,
                            tau=cases.TOPK_TAU, check_tol=2 * cases.SCORE_ATOL)              # as tests/test_pipeline_gpu.py
