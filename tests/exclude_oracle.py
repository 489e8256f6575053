"""numpy restatement of the exclusion contract (amdrec.exclude): take the block an unfiltered search for kc = k + E
returned, remove per query every entry whose id is in the query's exclusion list, keep the order, cut to k, pad.

``ids`` / ``pos`` / ``scores`` are [nq, kc]; ``ids`` are what the list is matched against (= ``pos`` for an index whose ids are
its positions), ``pos`` < 0 marks an unfilled entry (never matched, keeps its place).  Negative list entries are padding.
-> (pos [nq, k], scores [nq, k]); slots past the last survivor are -1 / ``fill_score``."""
import numpy as np


def compact(ids, pos, scores, excl, k, fill_score):
    ids, pos, scores, excl = np.asarray(ids), np.asarray(pos), np.asarray(scores), np.asarray(excl)
    nq, kc = pos.shape
    assert ids.shape == pos.shape == scores.shape and excl.shape[0] == nq and 1 <= k <= kc
    drop = np.zeros((nq, kc), dtype=bool)
    for i in range(nq):
        drop[i] = np.isin(ids[i], excl[i][excl[i] >= 0]) & (pos[i] >= 0) & (ids[i] >= 0)
    order = np.argsort(drop, axis=1, kind="stable")[:, :k]           # survivors first, in their order
    gone = np.take_along_axis(drop, order, axis=1)
    out_pos = np.where(gone, -1, np.take_along_axis(pos, order, axis=1)).astype(np.int64)
    out_sc = np.where(gone, np.float32(fill_score), np.take_along_axis(scores, order, axis=1)).astype(np.float32)
    return out_pos, out_sc


def fill_score(index_type):
    """The score of an unfilled slot: IVFPQ returns distances (ascending, +inf), Flat / IVF inner products (-inf)."""
    return np.float32(np.inf) if index_type == "IVFPQ" else np.float32(-np.inf)


def ids_of(pos, id_map):
    """The id path of FAISSIndex on positions: id_map[pos], an unfilled slot (-1) reading id_map[-1] like the reference."""
    return np.asarray(id_map)[np.asarray(pos)]
