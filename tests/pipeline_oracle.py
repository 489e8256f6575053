"""Numpy oracle for the serving pipeline behind stage 1 when a candidate list is short (test infrastructure).

Stage 1 hands stage 2 corpus POSITIONS ``cand_pos [B, k1]``; a negative position is a slot the search could not fill (the
corpus is smaller than ``k1``, narrow IVF probes, a stored NaN row, a NaN query, exclusions, removed ads).  The contract:

* such a slot is not a candidate.  The selection orders a user's slots by (real before unfilled, ranking logit descending
  with NaN last, slot ascending) and reports the first ``top_k`` REAL ones;
* where fewer than ``top_k`` real candidates exist, the tail reads ad id -1 and probability 0.0 for every task (what a list
  shorter than ``top_k`` reads);
* ``candidate_ids`` keeps the search's convention ``id_map[-1]`` for an unfilled slot; validity is decided by position.

``logits64`` is the float64 truth of the filled slots (oracle.ranker.forward), NaN elsewhere.
"""
import numpy as np

import oracle


def candidate_ids(cand_pos, id_map, ids_are_positions=False):
    """What ``candidate_ids`` holds: ``id_map[pos]``, an unfilled slot reads ``id_map[-1]`` (faiss_retrieval.py:159-160);
    with ``ids_are_positions`` the positions themselves."""
    cand_pos = np.asarray(cand_pos, dtype=np.int64)
    if ids_are_positions:
        return cand_pos.copy()
    id_map = np.asarray(id_map, dtype=np.int64)
    return id_map[np.where(cand_pos >= 0, cand_pos, len(id_map) - 1)]


def logits64(rk_sd, user_cat, user_num, cand_pos, ad_table):
    """-> {task: float64 [B, k1]}: the ranker in double precision on (user b, ad_table[cand_pos[b, j]]) for every filled
    slot, NaN in the unfilled ones."""
    cand_pos = np.asarray(cand_pos, dtype=np.int64)
    B, k1 = cand_pos.shape
    ub, sl = np.nonzero(cand_pos >= 0)
    out = {t: np.full((B, k1), np.nan) for t in oracle.ranker.TASKS}
    if len(ub):
        lg = oracle.ranker.forward(rk_sd, np.asarray(user_cat)[ub], np.asarray(ad_table)[cand_pos[ub, sl]],
                                   np.asarray(user_num, dtype=np.float32)[ub], dtype=np.float64)
        for t in oracle.ranker.TASKS:
            out[t][ub, sl] = lg[t]
    return out


def select(cand_pos_row, rank_logits_row, top_k):
    """One user: the reported slots, int64 [top_k], -1 where fewer than ``top_k`` real candidates exist."""
    pos = np.asarray(cand_pos_row, dtype=np.int64)
    v = np.asarray(rank_logits_row, dtype=np.float64)
    unfilled = pos < 0
    nan = np.isnan(v) & ~unfilled
    key = np.where(nan | unfilled, 0.0, v)
    with np.errstate(invalid="ignore"):
        order = np.lexsort((np.arange(len(pos)), -key, nan, unfilled))          # last key first: unfilled, NaN, logit, slot
    n_real = int((~unfilled).sum())
    out = np.full(top_k, -1, dtype=np.int64)
    n = min(top_k, n_real)
    out[:n] = order[:n]
    return out


def expected(cand_pos, cand_ids, logits, top_k, rank_task=0):
    """``logits`` [T, B, k1] (any float type; the GPU's own, or float64 truth) -> (ad_ids int64 [B, top_k], scores float32
    [T, B, top_k], slots int64 [B, top_k]) under the contract."""
    cand_pos = np.asarray(cand_pos, dtype=np.int64)
    cand_ids = np.asarray(cand_ids, dtype=np.int64)
    logits = np.asarray(logits)
    T, B, k1 = logits.shape
    ad_ids = np.full((B, top_k), -1, dtype=np.int64)
    scores = np.zeros((T, B, top_k), dtype=np.float32)
    slots = np.full((B, top_k), -1, dtype=np.int64)
    for b in range(B):
        s = select(cand_pos[b], logits[rank_task, b], top_k)
        real = s >= 0
        slots[b] = s
        ad_ids[b, real] = cand_ids[b, s[real]]
        for t in range(T):
            x = logits[t, b, s[real]].astype(np.float64)
            with np.errstate(over="ignore"):
                scores[t, b, real] = (1.0 / (1.0 + np.exp(-x))).astype(np.float32)
    return ad_ids, scores, slots
