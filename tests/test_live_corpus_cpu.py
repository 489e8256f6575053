"""Live corpus without a GPU: the removal-list helper, the numpy oracle against a brute-force restatement, and the argument
validation of amdrec_remove_plan / amdrec_rows_gather (nothing is launched: every refusal comes before the first HIP call)."""
import ctypes as C

import numpy as np
import pytest
import torch

from amdrec import _lib, rows_edit
from tests import live_corpus_oracle as lo


def test_removal_list_normalises_and_refuses():
    assert rows_edit.removal_list([5, 3, 5, 0]).tolist() == [0, 3, 5]                       # unsorted, duplicates
    assert rows_edit.removal_list([]).tolist() == [] and rows_edit.removal_list(None).tolist() == []
    assert rows_edit.removal_list(np.array([[9, 2], [2, 7]], dtype=np.int32)).tolist() == [2, 7, 9]
    assert rows_edit.removal_list(np.array([4, 1], dtype=np.uint8)).dtype == np.int64
    assert rows_edit.removal_list(torch.tensor([8, 8, 1])).tolist() == [1, 8]
    assert rows_edit.removal_list((np.int64(6), 2)).tolist() == [2, 6]
    out = rows_edit.removal_list(range(10, 0, -1))
    assert out.dtype == np.int64 and out.tolist() == list(range(1, 11))
    for bad in ([1, True], [np.bool_(False)], [1.0], ["3"], [None], np.array([1.5]), np.array([True]), torch.tensor([0.5])):
        with pytest.raises(TypeError):
            rows_edit.removal_list(bad)
    for bad in ([3, -1], np.array([-5]), torch.tensor([2, -2])):
        with pytest.raises(ValueError, match=">= 0"):
            rows_edit.removal_list(bad)


@pytest.mark.parametrize("seed", range(4))
def test_oracle_equals_a_loop(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 60))
    ids = rng.integers(0, 25, size=n).astype(np.int64)                                      # ids repeat
    remove = np.unique(rng.integers(0, 40, size=int(rng.integers(0, 12))))
    for keys in (ids, None):
        want = [i for i in range(n) if (i if keys is None else int(keys[i])) not in set(remove.tolist())]
        assert lo.kept_positions(keys, n, remove).tolist() == want
    src = rng.integers(0, 256, size=(max(n, 1), 7)).astype(np.uint8)
    pos = rng.integers(-3, src.shape[0] + 3, size=20)
    got = lo.gather_bytes(src, pos)
    for j, p in enumerate(pos):
        assert np.array_equal(got[j], src[p] if 0 <= p < src.shape[0] else np.zeros(7, dtype=np.uint8))


def test_exports_are_bound_and_the_abi_number_stays():
    lib = _lib.load()
    assert lib.amdrec_abi_version() == 14 == _lib.ABI_VERSION
    for name in ("amdrec_remove_plan_workspace", "amdrec_remove_plan", "amdrec_rows_gather"):
        assert name in _lib.exported_symbols() and hasattr(lib, name)


def test_plan_workspace_query():
    lib = _lib.load()
    nb = C.c_size_t(0)
    prev = 0
    for n in (0, 1, 1023, 1024, 1025, 70_001, 1_100_000, (1 << 31) - 1):
        assert lib.amdrec_remove_plan_workspace(n, C.byref(nb)) == 0
        assert nb.value >= prev and nb.value >= n + (n + 1023) // 1024 * 4                 # monotone; flags + block counts
        prev = nb.value
    assert lib.amdrec_remove_plan_workspace(1 << 31, C.byref(nb)) == -1 and b"2^31 - 1" in lib.amdrec_last_error()
    assert lib.amdrec_remove_plan_workspace(-1, C.byref(nb)) == -1 and b"n=-1" in lib.amdrec_last_error()
    assert lib.amdrec_remove_plan_workspace(10, None) == -1 and b"null pointer" in lib.amdrec_last_error()


def test_plan_entry_validates_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(ids=None, n=10, remove=p, n_remove=2, kept=p, n_kept=p, ws=p, ws_bytes=1 << 20):
        return lib.amdrec_remove_plan(ids, n, remove, n_remove, kept, n_kept, ws, ws_bytes, None)

    assert call(n=0, remove=None, n_remove=0, kept=None, n_kept=None, ws=None, ws_bytes=0) == 0   # empty, nulls and all
    assert call(n=-1) == -1 and b"n=-1" in lib.amdrec_last_error()
    assert call(n=1 << 31) == -1 and b"2^31 - 1" in lib.amdrec_last_error()
    assert call(n_remove=-1) == -1 and b"n_remove=-1" in lib.amdrec_last_error()
    assert call(remove=None) == -1 and b"null pointer: remove" in lib.amdrec_last_error()
    assert call(kept=None) == -1 and b"kept" in lib.amdrec_last_error()
    assert call(n_kept=None) == -1 and b"n_kept" in lib.amdrec_last_error()
    assert call(ws=None) == -3 and b"workspace too small" in lib.amdrec_last_error()
    assert call(n=70_001, ws_bytes=70_001) == -3 and b"workspace too small" in lib.amdrec_last_error()
    nb = C.c_size_t(0)
    assert lib.amdrec_remove_plan_workspace(70_001, C.byref(nb)) == 0
    misaligned = C.c_void_p(p.value + 8)
    assert call(n=10, ws=misaligned) == -1 and b"aligned" in lib.amdrec_last_error()


def test_gather_entry_validates_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    base = C.cast(buf, C.c_void_p).value
    src, dst, pos = C.c_void_p(base), C.c_void_p(base + 2048), C.c_void_p(base + 1024)

    def call(src=src, ld_src=16, n_src=8, pos=pos, n_out=4, row_bytes=16, dst=dst, ld_dst=16):
        return lib.amdrec_rows_gather(src, ld_src, n_src, pos, n_out, row_bytes, dst, ld_dst, None)

    assert call(n_out=0, src=None, pos=None, dst=None) == 0                                   # empty, nulls and all
    assert call(row_bytes=0, ld_src=0, ld_dst=0) == -1 and b"row_bytes=0" in lib.amdrec_last_error()
    assert call(row_bytes=-4) == -1 and b"row_bytes=-4" in lib.amdrec_last_error()
    assert call(n_src=-1) == -1 and b"n_src=-1" in lib.amdrec_last_error()
    assert call(n_out=-2) == -1 and b"n_out=-2" in lib.amdrec_last_error()
    assert call(ld_src=15) == -1 and b"ld_src_bytes=15" in lib.amdrec_last_error()
    assert call(ld_dst=8) == -1 and b"ld_dst_bytes=8" in lib.amdrec_last_error()
    assert call(pos=None) == -1 and b"null pointer: pos / dst" in lib.amdrec_last_error()
    assert call(dst=None) == -1 and b"null pointer: pos / dst" in lib.amdrec_last_error()
    assert call(src=None) == -1 and b"null pointer: src" in lib.amdrec_last_error()
    # overlap: the same array, a dst that starts inside src, a src that starts inside dst, a src that spans over dst
    assert call(dst=src) == -1 and b"overlaps" in lib.amdrec_last_error()
    assert call(dst=C.c_void_p(base + 8 * 16 - 1)) == -1 and b"overlaps" in lib.amdrec_last_error()
    assert call(src=C.c_void_p(base + 2048 + 3 * 16), dst=dst) == -1 and b"overlaps" in lib.amdrec_last_error()
    assert call(src=src, n_src=200, dst=dst, n_out=1) == -1 and b"overlaps" in lib.amdrec_last_error()   # src spans over dst
