"""IVFPQ without a GPU: the float64 oracle's table-lookup distance is the direct residual distance, and the new C-ABI
entries refuse bad arguments (null pointers, m, dim, k out of range) with -1 and a message before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from tests import ivfpq_oracle


@pytest.mark.parametrize("d,m", [(64, 4), (256, 8), (256, 32), (128, 16)])
def test_oracle_table_lookup_equals_direct_residual_distance(d, m):
    rng = np.random.default_rng(d + m)
    dsub = d // m
    cb = rng.standard_normal((m, 256, dsub))
    cent = rng.standard_normal((5, d))
    xb = rng.standard_normal((300, d))
    assign = rng.integers(0, 5, 300)
    codes = ivfpq_oracle.encode(xb, assign, cent, cb)
    q = rng.standard_normal(d)
    for l in range(5):
        lut = ivfpq_oracle.tables(q, cent[l], cb)
        rows = np.nonzero(assign == l)[0]
        recon = cb[np.arange(m)[None, :], codes[rows].astype(np.int64)].reshape(len(rows), d)     # r-hat
        direct = (((q - cent[l])[None, :] - recon) ** 2).sum(1)
        via = lut[np.arange(m)[None, :], codes[rows].astype(np.int64)].sum(1)
        np.testing.assert_allclose(via, direct, rtol=1e-12, atol=1e-12)
    # the encoder's codes are the arg-min codewords
    r = xb - cent[assign]
    for s in range(m):
        d2 = ((r[:, None, s * dsub:(s + 1) * dsub] - cb[s][None]) ** 2).sum(-1)
        assert np.array_equal(codes[:, s], d2.argmin(1))


def test_oracle_adc_search_orders_ascending_and_underfills():
    rng = np.random.default_rng(3)
    d, m = 32, 8
    cb = rng.standard_normal((m, 256, d // m))
    cent = rng.standard_normal((4, d))
    assign = rng.integers(0, 4, 50)
    codes = rng.integers(0, 256, (50, m)).astype(np.uint8)
    xq = rng.standard_normal((3, d))
    D, I = ivfpq_oracle.adc_search(codes, assign, cent, cb, xq, 60, 4)
    assert np.isinf(D[:, 50:]).all() and (I[:, 50:] == -1).all()
    assert (np.diff(D[:, :50], axis=1) >= 0).all()
    assert all(sorted(I[q, :50].tolist()) == list(range(50)) for q in range(3))


def _lib():
    from amdrec import _lib as L
    return L.load()


def test_ivfpq_entries_validate_arguments_without_a_gpu():
    lib = _lib()
    n = C.c_size_t(0)
    # workspace query: m, dim, rows
    assert lib.amdrec_ivfpq_train_workspace(65536, 256, 8, C.byref(n)) == 0
    assert n.value >= 65536 * 8 + 256 * 256 * 8 + 8 * 256 * 4
    assert lib.amdrec_ivfpq_train_workspace(100, 256, 7, C.byref(n)) == -1
    assert b"m=7" in lib.amdrec_last_error()
    assert lib.amdrec_ivfpq_train_workspace(100, 256, 64, C.byref(n)) == -1
    assert lib.amdrec_ivfpq_train_workspace(100, 96, 16, C.byref(n)) == -1        # dsub = 6: not a multiple of 4
    assert b"dim=96" in lib.amdrec_last_error()
    assert lib.amdrec_ivfpq_train_workspace(100, 4096, 8, C.byref(n)) == -1       # dim > 2048
    assert lib.amdrec_ivfpq_train_workspace(100, 256, 8, None) == -1
    assert b"null" in lib.amdrec_last_error()
    assert lib.amdrec_ivfpq_train_workspace((1 << 20) + 1, 256, 8, C.byref(n)) == -1
    # encode
    assert lib.amdrec_ivfpq_encode(None, 0, 256, 256, None, None, 256, 100, None, 8, None, None) == 0      # rows = 0
    assert lib.amdrec_ivfpq_encode(None, 10, 256, 256, None, None, 256, 100, None, 8, None, None) == -1
    assert b"null" in lib.amdrec_last_error()
    assert lib.amdrec_ivfpq_encode(None, 10, 256, 256, None, None, 256, 100, None, 12, None, None) == -1
    assert b"m=12" in lib.amdrec_last_error()
    assert lib.amdrec_ivfpq_encode(None, 10, 250, 250, None, None, 256, 100, None, 8, None, None) == -1
    assert b"dim=250" in lib.amdrec_last_error()
    # training step
    assert lib.amdrec_ivfpq_train_step(None, 10, 256, 256, None, None, 256, 100, None, 8, None, 0, None) == -1
    assert lib.amdrec_ivfpq_train_step(None, 10, 256, 256, None, None, 256, 100, None, 3, None, 0, None) == -1
    # tables
    assert lib.amdrec_ivfpq_tables(None, 0, 256, 256, None, 10, 10, None, 256, 100, None, 8, None, None) == 0   # nq = 0
    assert lib.amdrec_ivfpq_tables(None, 4, 256, 256, None, 10, 10, None, 256, 100, None, 8, None, None) == -1
    assert b"null" in lib.amdrec_last_error()
    assert lib.amdrec_ivfpq_tables(None, 4, 256, 256, None, 10, 10, None, 256, 100, None, 5, None, None) == -1
    assert lib.amdrec_ivfpq_tables(None, 4, 256, 260, None, 10, 10, None, 256, 100, None, 8, None, None) == -1
    assert b"dim=260" in lib.amdrec_last_error()
    # scan
    assert lib.amdrec_ivfpq_scan(None, 8, None, None, 100, 1000, None, 10, None, None, 130, 32, None, None, None, 40, None,
                                 1000, 0, None) == -1
    assert b"null" in lib.amdrec_last_error()
    assert lib.amdrec_ivfpq_scan(None, 6, None, None, 100, 1000, None, 10, None, None, 130, 32, None, None, None, 40, None,
                                 1000, 0, None) == -1
    assert b"m=6" in lib.amdrec_last_error()
    assert lib.amdrec_ivfpq_scan(None, 8, None, None, 100, 1000, None, 10, None, None, 130, 16, None, None, None, 40, None,
                                 1000, 0, None) == -1
    assert lib.amdrec_ivfpq_scan(None, 8, None, None, 100, 1000, None, 10, None, None, 70000, 32, None, None, None, 40, None,
                                 1000, 0, None) == -1
    # distances: k
    assert lib.amdrec_ivfpq_distances(None, 4, 0, None, None) == -1
    assert b"k=0" in lib.amdrec_last_error()
    assert lib.amdrec_ivfpq_distances(None, 4, 2049, None, None) == -1
    assert lib.amdrec_ivfpq_distances(None, 4, 10, None, None) == -1
    assert b"null" in lib.amdrec_last_error()
    assert lib.amdrec_ivfpq_distances(None, 0, 10, None, None) == 0


def test_ivfpq_constructor_arguments_are_checked_before_the_device():
    """pq_m and HNSW are refused at construction (no GPU needed to reach the checks)."""
    from amdrec import ivfpq
    with pytest.raises(ValueError):
        ivfpq.check_pq_m(256, 12)
    with pytest.raises(ValueError):
        ivfpq.check_pq_m(96, 16)
    with pytest.raises(ValueError):
        ivfpq.check_pq_m(256, 64)
    for m in (4, 8, 16, 32):
        ivfpq.check_pq_m(256, m)
    with pytest.raises(ValueError):
        ivfpq.check_nlist(65535)
    ivfpq.check_nlist(65534)
