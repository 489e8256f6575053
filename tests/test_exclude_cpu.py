"""Exclusion lists without a GPU: the host helpers (amdrec.exclude), the numpy oracle against a brute-force restatement, and
amdrec_exclude_compact's argument validation (nothing is launched)."""
import numpy as np
import pytest

from amdrec import _lib, exclude
from tests import exclude_oracle


def test_check_exclude_limit():
    assert exclude.check_exclude(500, 1548) == 2048                     # k + E = AMDREC_MAX_K is accepted
    assert exclude.check_exclude(2048, 0) == 2048
    with pytest.raises(ValueError, match="AMDREC_MAX_K = 2048"):
        exclude.check_exclude(500, 1549)                                # 2049
    with pytest.raises(ValueError, match="AMDREC_MAX_K = 2048"):
        exclude.check_exclude(2048, 1)
    with pytest.raises(ValueError):
        exclude.check_exclude(10, -1)


def test_pad_exclusions():
    blk = exclude.pad_exclusions([[5, 3, 5], [], (7,), np.array([1, 2], dtype=np.int32)])
    assert blk.dtype == np.int64 and blk.shape == (4, 3)
    assert blk.tolist() == [[5, 3, 5], [-1, -1, -1], [7, -1, -1], [1, 2, -1]]
    assert exclude.pad_exclusions([[1], [2, 3]], width=4).tolist() == [[1, -1, -1, -1], [2, 3, -1, -1]]
    assert exclude.pad_exclusions([[], []]).shape == (2, 0)
    assert exclude.pad_exclusions([]).shape == (0, 0)
    assert exclude.pad_exclusions([None, [4]]).tolist() == [[-1], [4]]
    with pytest.raises(ValueError, match="width"):
        exclude.pad_exclusions([[1, 2, 3]], width=2)
    with pytest.raises(ValueError, match=">= 0"):
        exclude.pad_exclusions([[1, -1]])
    for bad in (1.0, np.float32(2), "3", True, None):
        with pytest.raises(TypeError):
            exclude.pad_exclusions([[1, bad]])


def test_as_block():
    assert exclude.as_block(None, 3) is None
    assert exclude.as_block([[], [], []], 3) is None                     # E = 0: no list
    assert exclude.as_block([[1], [], [2, 3]], 3).tolist() == [[1, -1], [-1, -1], [2, 3]]
    arr = np.array([[4, -1], [5, 6]], dtype=np.int32)
    assert exclude.as_block(arr, 2).dtype == np.int64 and exclude.as_block(arr, 2).tolist() == arr.tolist()
    with pytest.raises(ValueError, match="2 exclusion lists for 3 queries"):
        exclude.as_block(arr, 3)
    with pytest.raises(TypeError):
        exclude.as_block(np.zeros((2, 2), dtype=np.float32), 2)


def _brute(ids, pos, scores, excl, k, fill):
    out_p = np.full((len(pos), k), -1, dtype=np.int64)
    out_s = np.full((len(pos), k), fill, dtype=np.float32)
    for i in range(len(pos)):
        banned = {int(e) for e in excl[i] if e >= 0}
        kept = [j for j in range(pos.shape[1]) if pos[i, j] < 0 or int(ids[i, j]) not in banned][:k]
        out_p[i, :len(kept)] = pos[i, kept]
        out_s[i, :len(kept)] = scores[i, kept]
    return out_p, out_s


@pytest.mark.parametrize("seed", range(6))
def test_oracle_equals_the_set_difference_restatement(seed):
    rng = np.random.default_rng(seed)
    nq, k, E = 9, int(rng.integers(1, 40)), int(rng.integers(1, 30))
    kc = k + E
    fill = np.float32(np.inf if seed % 2 else -np.inf)
    pos = np.stack([rng.permutation(200)[:kc] for _ in range(nq)]).astype(np.int64)
    scores = np.sort(rng.standard_normal((nq, kc)).astype(np.float32), axis=1)[:, ::-1].copy()
    id_map = rng.integers(0, 60, size=200)                              # duplicate ids: one id names several rows
    excl = rng.integers(-1, 60, size=(nq, E)).astype(np.int64)          # -1 = padding, duplicates, ids not among the rows
    excl[1] = -1                                                        # nothing excluded
    for i in (2, 3):                                                    # unfilled tails
        fillfrom = int(rng.integers(0, kc))
        pos[i, fillfrom:], scores[i, fillfrom:] = -1, fill
    ids = np.where(pos >= 0, id_map[pos], id_map[-1])                   # the remap's -1 -> id_map[-1]
    excl[3, 0] = id_map[-1]                                             # ... which must not make an unfilled entry match
    wide = np.unique(ids[4])[:E]
    if len(wide) == len(np.unique(ids[4])):                             # a list that names the row's whole top-kc
        excl[4, :len(wide)] = wide
    got = exclude_oracle.compact(ids, pos, scores, excl, k, fill)
    want = _brute(ids, pos, scores, excl, k, fill)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # identity ids (the list is matched against the positions themselves) and an all-excluded row
    excl2 = excl.copy()
    excl2[5, :] = -1
    p5 = pos[5][:E]
    excl2[5, :len(p5)] = p5
    got = exclude_oracle.compact(pos, pos, scores, excl2, k, fill)
    want = _brute(pos, pos, scores, excl2, k, fill)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_oracle_all_excluded_row_is_all_unfilled():
    pos = np.arange(6, dtype=np.int64)[None]
    sc = np.linspace(1, 0, 6, dtype=np.float32)[None]
    p, s = exclude_oracle.compact(pos, pos, sc, np.array([[0, 1, 2, 3, 4, 5]]), 2, -np.inf)   # (E > kc - k: only here)
    assert p.tolist() == [[-1, -1]] and np.isneginf(s).all()
    p, s = exclude_oracle.compact(pos, pos, sc, np.array([[1, 1, -1, 77]]), 2, -np.inf)
    assert p.tolist() == [[0, 2]] and s.tolist() == [[sc[0, 0], sc[0, 2]]]


def test_compact_entry_validates_arguments_without_a_gpu():
    """amdrec_exclude_compact refuses bad arguments before anything is launched; nq = 0 returns 0."""
    lib = _lib.load()

    def call(kc=564, E=64, ld=64, k=500, nq=1, keys=None, scores=None, carry=None, excl=None, ok=None, os_=None, oc=None):
        return lib.amdrec_exclude_compact(keys, scores, carry, nq, kc, excl, E, ld, k, -1, float("-inf"), -1, ok, os_, oc, None)

    assert call(k=0) == -1 and b"k=0" in lib.amdrec_last_error()
    assert call(k=565) == -1 and b"k=565" in lib.amdrec_last_error()              # k > kc
    assert call(kc=2049, k=500) == -1 and b"kc=2049" in lib.amdrec_last_error()
    assert call(kc=0) == -1
    assert call(E=0, ld=0) == -1 and b"n_exclude=0" in lib.amdrec_last_error()
    assert call(kc=2048, E=2048, ld=2048) == -1 and b"n_exclude=2048" in lib.amdrec_last_error()
    assert call(ld=63) == -1 and b"ld_exclude=63" in lib.amdrec_last_error()      # leading dimension smaller than E
    assert call(nq=0) == 0                                                        # nothing to do, nulls and all
    assert call(kc=2048, E=2047, ld=2047, k=1, nq=0) == 0                         # the largest shapes are in range
    assert call() == -1 and b"null pointer" in lib.amdrec_last_error()            # nulls
    import ctypes as C
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert call(kc=2, E=1, ld=1, k=1, keys=p, scores=p, excl=p, os_=p) == -1      # no out_keys and no carry
    assert b"out_keys" in lib.amdrec_last_error()
    assert call(kc=2, E=1, ld=1, k=1, keys=p, scores=p, excl=p, ok=p, os_=p, carry=p) == -1   # carry without out_carry
    assert b"carry" in lib.amdrec_last_error()
    assert call(kc=2, E=1, ld=1, k=1, keys=p, scores=p, ok=p, os_=p) == -1 and b"exclude" in lib.amdrec_last_error()


def test_abi_version_is_unchanged_and_the_export_is_bound():
    assert _lib.load().amdrec_abi_version() == 14 == _lib.ABI_VERSION
    assert "amdrec_exclude_compact" in _lib.exported_symbols()


def test_index_rejects_an_oversized_list_before_touching_the_device():
    """k + E > AMDREC_MAX_K is a ValueError from FAISSIndex.search_device whatever the tensors are (checked first)."""
    import torch
    from amdrec.index import FAISSIndex
    idx = FAISSIndex.__new__(FAISSIndex)                                  # no device, no library
    with pytest.raises(ValueError, match="AMDREC_MAX_K = 2048"):
        FAISSIndex.search_device(idx, torch.zeros(1, 8), 500, exclude=torch.zeros((1, 1549), dtype=torch.int64))
