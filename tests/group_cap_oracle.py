"""The per-group cap (amdrec.group_cap) restated in numpy as the plain greedy loop: walk the entries in rank order, accept one
while fewer than ``cap`` ACCEPTED entries share its group, never cap a negative group.  The kernels are compared with this,
not with each other; ``rank_form`` is the parallel statement the kernels implement ("fewer than cap better-ranked entries of
my group"), compared with the loop in tests/test_group_cap_cpu.py."""
import numpy as np


def group_at(group_of, pos):
    """Group key of corpus position ``pos``: a position outside the array is ungrouped (-1) and never read."""
    return int(group_of[pos]) if 0 <= pos < len(group_of) else -1


def greedy_keep(groups, cap):
    """``groups``: the entries' group keys in rank order -> bool per entry, by the greedy loop."""
    taken, keep = {}, []
    for g in groups:
        g = int(g)
        ok = g < 0 or taken.get(g, 0) < cap
        if ok and g >= 0:
            taken[g] = taken.get(g, 0) + 1
        keep.append(ok)
    return np.array(keep, dtype=bool)


def rank_form(groups, cap):
    """The same decision from each entry's own group prefix: keep iff fewer than cap EARLIER entries have its group."""
    groups = np.asarray(groups, dtype=np.int64)
    return np.array([g < 0 or int((groups[:i] == g).sum()) < cap for i, g in enumerate(groups)], dtype=bool)


def select_order(logits_row, cand_pos_row):
    """The stage-2 selection's visiting order of one user's candidate slots: unfilled slots (position < 0) are no candidates;
    logit descending (-0.0 == +0.0), slot ascending, NaN logits after every other logit."""
    slots = [i for i in range(len(logits_row)) if cand_pos_row[i] >= 0]
    return sorted(slots, key=lambda i: (1, 0.0, i) if np.isnan(logits_row[i]) else (0, -float(logits_row[i]), i))


def select_topk_capped(rank_logits, cand_ids, cand_pos, top_k, group_of, cap):
    """amdrec_select_topk_capped's ids and slots: ``rank_logits`` [n_users, k_c] (the ranking task's logits), ``cand_ids`` /
    ``cand_pos`` [n_users, k_c] -> (out_ids int64 [n_users, top_k], out_slots int32 [n_users, top_k]); tail -1 / -1."""
    n_users, k_c = cand_pos.shape
    out_ids = np.full((n_users, top_k), -1, dtype=np.int64)
    out_slots = np.full((n_users, top_k), -1, dtype=np.int32)
    for u in range(n_users):
        order = select_order(rank_logits[u], cand_pos[u])
        keep = greedy_keep([group_at(group_of, int(cand_pos[u, s])) for s in order], cap)
        won = [s for s, ok in zip(order, keep) if ok][:top_k]
        out_slots[u, :len(won)] = won
        out_ids[u, :len(won)] = cand_ids[u, won]
    return out_ids, out_slots


def scores_at(prob_by_slot, out_slots):
    """out_scores for ``out_slots``: ``prob_by_slot`` [n_tasks, n_users, k_c] (each candidate's probabilities as the device
    writes them) gathered at the winners, 0.0 in the tail."""
    n_tasks, n_users, _ = prob_by_slot.shape
    out = np.zeros((n_tasks, n_users, out_slots.shape[1]), dtype=np.float32)
    for u in range(n_users):
        for r, s in enumerate(out_slots[u]):
            if s >= 0:
                out[:, u, r] = prob_by_slot[:, u, s]
    return out


def compact(pos, scores, group_of, cap, k, fill_score):
    """amdrec_group_cap_compact: pos / scores [nq, kc] in the index's order -> ([nq, k], [nq, k]).  An unfilled entry (pos <
    0) is never counted and never dropped; the slots past the last kept entry read -1 / fill_score."""
    nq, kc = pos.shape
    out_pos = np.full((nq, k), -1, dtype=np.int64)
    out_sc = np.full((nq, k), fill_score, dtype=np.float32)
    for q in range(nq):
        keep = greedy_keep([group_at(group_of, int(p)) for p in pos[q]], cap)
        cols = np.nonzero(keep)[0][:k]
        out_pos[q, :len(cols)] = pos[q, cols]
        out_sc[q, :len(cols)] = scores[q, cols]
    return out_pos, out_sc


def fill_score(index_type):
    return np.float32(np.inf) if index_type == "IVFPQ" else np.float32(-np.inf)
