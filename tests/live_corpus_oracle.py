"""numpy oracle of the live-corpus entries (amdrec_remove_plan / amdrec_rows_gather): a removal is ``keep = ~isin(ids,
remove)``, ``kept = nonzero(keep)``; a gather is fancy indexing with zero rows for positions out of range."""
import numpy as np


def kept_positions(ids, n, remove):
    """ids: int64 [n] or None (a row's key is its position) -> the old positions of the rows that stay, ascending."""
    keys = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)[:n]
    return np.nonzero(~np.isin(keys, np.asarray(remove, dtype=np.int64)))[0].astype(np.int64)


def gather_bytes(src, pos):
    """src: uint8 [n_src, row_bytes]; pos: int64 [m] -> uint8 [m, row_bytes]; out-of-range positions give zero rows."""
    pos = np.asarray(pos, dtype=np.int64)
    ok = (pos >= 0) & (pos < src.shape[0])
    out = np.zeros((len(pos), src.shape[1]), dtype=src.dtype)
    out[ok] = src[pos[ok]]
    return out


def removal_patterns(ids, n, rng):
    """The removal lists of the plan test, as {name: ascending unique int64 array of KEYS}: nothing, everything, the first
    row only, the last row only, every other row, one run across a 1024 boundary, and a mix with keys no row has."""
    keys = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    pats = {"nothing": np.empty(0, dtype=np.int64)}
    if n == 0:
        pats["absent"] = np.array([3, 9], dtype=np.int64)
        return pats
    absent = int(keys.max()) + 1 + np.arange(5, dtype=np.int64) * 3
    pats["everything"] = np.unique(keys)
    pats["first"] = keys[:1].copy()
    pats["last"] = keys[-1:].copy()
    pats["every_other"] = np.unique(keys[::2])
    lo, hi = max(0, min(n, 1024) - 37), min(n, 1024 + 41)
    pats["straddle"] = np.unique(keys[lo:hi])
    pats["mixed_absent"] = np.unique(np.concatenate([keys[rng.random(n) < 0.3], absent]))
    return pats
