"""tests/pipeline_oracle.py on its own (no GPU): on fully filled lists it is oracle.pipeline.select_top / sigmoid, and the
short-list contract on hand-written cases."""
import numpy as np

import oracle
from amdrec import synth
from tests import cases
from tests import pipeline_oracle as po


def test_fully_filled_lists_are_select_top():
    rng = np.random.default_rng(1)
    for k1, top_k in ((500, 10), (37, 10), (7, 7), (64, 1)):
        B, T = 4, 3
        logits = rng.standard_normal((T, B, k1)).astype(np.float32)
        logits[0, 1, :] = 0.25                                           # all tied: the lowest slots, in order
        logits[0, 2, ::3] = logits[0, 2, 1]                              # scattered ties
        pos = np.stack([rng.permutation(9000)[:k1] for _ in range(B)])
        ids = pos * 3 + 11
        ad_ids, scores, slots = po.expected(pos, ids, logits, top_k)
        for b in range(B):
            top = oracle.pipeline.select_top(logits[0, b], top_k)
            assert slots[b].tolist() == top.tolist()
            assert ad_ids[b].tolist() == ids[b][top].tolist()
            for t in range(T):
                assert np.array_equal(scores[t, b], oracle.pipeline.sigmoid(logits[t, b][top]))


def test_hand_written_short_lists():
    inf = np.inf
    # all slots unfilled: nothing is reported, whatever the logits say
    pos = np.full((1, 5), -1)
    lg = np.array([[[9.0, 8.0, 7.0, 6.0, 5.0]], [[1.0] * 5]])
    ad_ids, scores, slots = po.expected(pos, np.full((1, 5), 4), lg, 3)
    assert ad_ids.tolist() == [[-1, -1, -1]] and slots.tolist() == [[-1, -1, -1]] and not scores.any()
    # unfilled slots in the middle, with the largest logits of the row: real candidates only, by logit then slot
    pos = np.array([[10, -1, 12, -1, 14, 15]])
    ids = np.array([[110, 999, 112, 999, 114, 115]])
    lg = np.array([[[0.5, 50.0, 2.0, 60.0, 2.0, -1.0]]])
    ad_ids, scores, slots = po.expected(pos, ids, lg, 3)
    assert slots.tolist() == [[2, 4, 0]] and ad_ids.tolist() == [[112, 114, 110]]
    assert np.array_equal(scores[0, 0], oracle.pipeline.sigmoid(np.array([2.0, 2.0, 0.5])))
    # fewer real candidates than top_k: the tail reads -1 / 0.0 for every task
    ad_ids, scores, slots = po.expected(pos, ids, np.concatenate([lg, -lg]), 6)
    assert ad_ids.tolist() == [[112, 114, 110, 115, -1, -1]] and slots[0, 4:].tolist() == [-1, -1]
    assert (scores[:, 0, 4:] == 0).all() and (scores[:, 0, :4] > 0).all()
    # a NaN logit in a real slot next to an unfilled slot with a large logit: NaN is last among the real, the unfilled
    # slot is behind it, i.e. nowhere; -inf is an ordinary (smallest) logit
    pos = np.array([[3, -1, 5, 6]])
    ids = np.array([[3, 6, 5, 6]])
    lg = np.array([[[np.nan, 1e9, -inf, 0.0]]])
    ad_ids, scores, slots = po.expected(pos, ids, lg, 4)
    assert slots.tolist() == [[3, 2, 0, -1]] and ad_ids.tolist() == [[6, 5, 3, -1]]
    assert scores[0, 0, 1] == 0.0 and np.isnan(scores[0, 0, 2]) and scores[0, 0, 3] == 0.0
    assert po.select(pos[0], lg[0, 0], 1).tolist() == [3]


def test_candidate_ids_keep_the_search_convention():
    pos = np.array([[2, -1, 0], [-1, -1, 1]])
    id_map = np.array([11, 14, 17])
    assert po.candidate_ids(pos, id_map).tolist() == [[17, 17, 11], [17, 17, 14]]
    assert po.candidate_ids(pos, np.arange(3)).tolist() == [[2, 2, 0], [2, 2, 1]]
    assert po.candidate_ids(pos, None, ids_are_positions=True).tolist() == pos.tolist()


def test_logits64_is_the_float64_ranker_on_the_filled_slots():
    user, ad, nnum = cases.small_dims()
    sd = synth.ranker_state(user, ad, nnum, seed=5, cross_scale=1.0 / 16)
    table = synth.ad_features(ad, 9, seed=6)
    uc, un = synth.user_batch(user, nnum, 2, seed=7)
    pos = np.array([[4, -1, 0], [-1, -1, -1]])
    lg = po.logits64(sd, uc, un, pos, table)
    ref = oracle.ranker.forward(sd, uc[[0, 0]], table[[4, 0]], un[[0, 0]], dtype=np.float64)
    for t in oracle.ranker.TASKS:
        assert lg[t].dtype == np.float64 and lg[t].shape == (2, 3)
        assert np.array_equal(lg[t][0, [0, 2]], ref[t]) and np.isnan(lg[t][0, 1]) and np.isnan(lg[t][1]).all()
