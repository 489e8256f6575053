"""Diversified selection: the stage-2 selection re-ordered by relevance discounted by similarity to what is already chosen,
decided inside one selection kernel (``amdrec_select_topk_diverse``).

The per-group cap needs a group key the caller knows; ten creatives that embed almost identically under different keys, or
under none, still fill ten slots.  This rule looks at the embeddings instead: the index's own L2-normalised rows
(``FAISSIndex._xb``, Flat and IVF), read at call time through the candidates' corpus positions.  It is a multiplicative form
of MMR - scale-free: pCTRs are small, similarities are O(1), and no per-user normalisation of relevance is needed.  Per user,
with ``lam`` in [0, 1] and ``pool = M``:

1. Candidates and relevance order are ``amdrec_select_topk``'s: a slot is a candidate iff ``cand_pos >= 0``; CTR logit
   descending, slot ascending, NaN logits last.
2. Cap first (``max_per_group = c > 0``): a candidate is accepted iff fewer than ``c`` better-ranked candidates share its
   non-negative group - ``amdrec_select_topk_capped``'s acceptance.  Without a cap every candidate is accepted.
3. The pool is the first ``M`` accepted candidates in that order (fewer if there are fewer).  It holds at most ``c`` members of
   any group, so the greedy loop keeps no cap bookkeeping and its result satisfies the cap by construction.
4. Greedy: member ``i`` has ``rel_i``, the fp32 probability the selection reports for its ranking logit, and ``m_i = 0``.  For
   rank ``r = 0 .. top_k - 1`` the untaken member with the largest ``v_i = rel_i * fmaf(-lam, m_i, 1.0f)`` (fp32, two
   roundings) wins.  Equal values go to the member earlier in the relevance order; a NaN value ranks after every non-NaN one,
   among NaNs the earlier member first.  After winner ``w``, for every remaining ``i``: ``m_i = fminf(1, fmaxf(m_i, s_iw))``
   with ``s_iw`` the fp32 inner product of rows ``cand_pos[i]`` and ``cand_pos[w]`` (accumulation order free).  A NaN
   similarity leaves ``m_i`` as it was, a negative one does not discount, and a position beyond the row array is never read:
   similarity 0.
5. The winners go out in pick order, ids / every task's probability / slots as ``amdrec_select_topk`` writes them, and
   ``values[u][r]`` is the winning ``v``.  A pool shorter than ``top_k`` leaves the tail: id -1, slot -1, probabilities 0.0,
   value 0.0.

With ``lam == 0`` the result is ``amdrec_select_topk``'s (``amdrec_select_topk_capped``'s under a cap) bit for bit - sigmoid is
monotone, and ties in probability fall back to the logit order -, and the rank-0 winner is always the most relevant accepted
candidate.  Out of scope: the auction (a generalised second price has no meaning under a re-ordered slate), IVFPQ (it keeps
codes, not rows), the sharded recommender and the micro-batcher.

This module holds the host helpers and a float64 numpy statement of the rule (no GPU needed).
"""
from __future__ import annotations

import math

import numpy as np

MAX_POOL = 128           # the kernel's pool_key / m arrays
MAX_POOL_FLOATS = 32768  # pool * dim: the pool's rows are staged in one workgroup's LDS (128 KB)
DEFAULT_POOL = 64


def check_diversity(diversity, diversity_pool, top_k: int, dim: int, index_type: str = "Flat", auction: bool = False):
    """The ``diversity`` / ``diversity_pool`` arguments -> None (today's selection) or ``(lam, pool)`` as the entry takes
    them.  Refused, before the library is touched: a ``lam`` that is no number (TypeError), outside [0, 1] or not finite, a
    pool that is no integer (TypeError), below ``top_k``, above 128 or with ``pool * dim > 32768``, a pool without ``diversity``,
    ``diversity`` under the auction (ValueError), and ``diversity`` on an IVFPQ index (NotImplementedError)."""
    if isinstance(diversity_pool, (bool, np.bool_)) or not isinstance(diversity_pool, (int, np.integer)):
        raise TypeError(f"diversity_pool must be an integer, got {diversity_pool!r} ({type(diversity_pool).__name__})")
    pool = int(diversity_pool)
    if diversity is None:
        if pool != DEFAULT_POOL:
            raise ValueError(f"diversity_pool={pool} without diversity: the pool belongs to the diversified selection")
        return None
    if isinstance(diversity, (bool, np.bool_)) or not isinstance(diversity, (int, float, np.integer, np.floating)):
        raise TypeError(f"diversity must be a number in [0, 1], got {diversity!r} ({type(diversity).__name__})")
    lam = float(diversity)
    if not math.isfinite(lam) or not 0.0 <= lam <= 1.0:
        raise ValueError(f"diversity must be finite and in [0, 1], got {diversity!r}")
    if auction:
        raise ValueError('diversity with rank_by="ecpm": a generalised second price has no meaning under a re-ordered slate')
    if index_type == "IVFPQ":
        raise NotImplementedError("diversity on an IVFPQ index: it keeps codes, not rows")
    top_k, dim = int(top_k), int(dim)
    if pool < top_k:
        raise ValueError(f"diversity_pool={pool} is smaller than top_k={top_k}")
    if pool > MAX_POOL:
        raise ValueError(f"diversity_pool={pool} exceeds {MAX_POOL}")
    if pool * dim > MAX_POOL_FLOATS:
        raise ValueError(f"diversity_pool * dim = {pool} * {dim} exceeds {MAX_POOL_FLOATS}: the pool's rows must fit one "
                         f"workgroup's LDS")
    return lam, pool


def check_index_diversity(idx, diversity, diversity_pool, top_k: int, auction: bool = False):
    """check_diversity against a FAISSIndex (its dimension and type are looked at only where ``diversity`` is given)."""
    if diversity is None:
        return check_diversity(None, diversity_pool, top_k, 0)
    return check_diversity(diversity, diversity_pool, top_k, idx.dimension, idx.index_type, auction)


def sigmoid_f32(x) -> np.ndarray:
    """1 / (1 + exp(-x)) evaluated in float32, the shape of the device's expression (the device's ``expf`` may differ in the
    last bit: compare against the probabilities the device wrote where bits matter)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-x))).astype(np.float32)


def relevance_order(logits_row, cand_pos_row) -> list:
    """The selection's visiting order of one user's slots: candidates only; logit descending (-0.0 == +0.0), slot ascending,
    NaN logits last."""
    slots = [i for i in range(len(logits_row)) if cand_pos_row[i] >= 0]
    return sorted(slots, key=lambda i: (1, 0.0, i) if np.isnan(logits_row[i]) else (0, -float(logits_row[i]), i))


def build_pool(logits_row, cand_pos_row, pool: int, group_of=None, max_per_group: int = 0) -> list:
    """Steps 1-3: the slots of one user's pool, in relevance order."""
    out, taken = [], {}
    for s in relevance_order(logits_row, cand_pos_row):
        if len(out) == pool:
            break
        p = int(cand_pos_row[s])
        g = int(group_of[p]) if (max_per_group > 0 and group_of is not None and p < len(group_of)) else -1
        if g >= 0:
            if taken.get(g, 0) >= max_per_group:
                continue
            taken[g] = taken.get(g, 0) + 1
        out.append(s)
    return out


def similarity(rows, pos_a: int, pos_b: int) -> float:
    """float64 inner product of two corpus rows; 0 where either position lies beyond the array (never read)."""
    if pos_a >= len(rows) or pos_b >= len(rows):
        return 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.dot(np.asarray(rows[pos_a], dtype=np.float64), np.asarray(rows[pos_b], dtype=np.float64)))


def better(v_a: float, v_b: float) -> bool:
    """Does value ``v_a`` of an EARLIER member lose to ``v_b`` of a later one?  Only when v_b is strictly larger, or v_a is NaN
    and v_b is not."""
    if math.isnan(v_b):
        return False
    return math.isnan(v_a) or v_b > v_a


def select_diverse(rank_logits, cand_pos, rows, lam: float, pool: int, top_k: int, group_of=None, max_per_group: int = 0,
                   rel=None):
    """The rule in float64.  ``rank_logits`` / ``cand_pos`` [n_users, k_c], ``rows`` [n_rows, dim]; ``rel`` [n_users, k_c]: the
    candidates' relevance (default: sigmoid_f32 of the logits) -> (slots int32 [n_users, top_k], values float64 [n_users,
    top_k]); tail -1 / 0.0."""
    rank_logits, cand_pos = np.asarray(rank_logits), np.asarray(cand_pos)
    n_users = cand_pos.shape[0]
    rel = sigmoid_f32(rank_logits) if rel is None else np.asarray(rel)
    lam = float(np.float32(lam))
    slots = np.full((n_users, top_k), -1, dtype=np.int32)
    values = np.zeros((n_users, top_k), dtype=np.float64)
    for u in range(n_users):
        members = build_pool(rank_logits[u], cand_pos[u], pool, group_of, max_per_group)
        m = [0.0] * len(members)
        free = list(range(len(members)))
        for r in range(min(top_k, len(members))):
            best, best_v = None, 0.0
            for i in free:
                v = float(rel[u, members[i]]) * (1.0 - lam * m[i])
                if best is None or better(best_v, v):
                    best, best_v = i, v
            free.remove(best)
            slots[u, r], values[u, r] = members[best], best_v
            for i in free:
                s = similarity(rows, int(cand_pos[u, members[i]]), int(cand_pos[u, members[best]]))
                if not math.isnan(s):
                    m[i] = min(1.0, max(m[i], s))
    return slots, values
