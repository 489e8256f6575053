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
    # the scan with per-list finite-row counts (ABI v13): the same checks, and the counts are required
    assert lib.amdrec_ivfpq_scan_finite(None, 8, None, None, None, 100, 1000, None, 10, None, None, 130, 32, None, None, None,
                                        40, None, 1000, 0, None) == -1
    assert b"null" in lib.amdrec_last_error()
    buf = C.create_string_buffer(64)
    p = C.cast(C.addressof(buf) + (-C.addressof(buf)) % 16, C.c_void_p)   # any 16-byte aligned address: nothing launches
    assert lib.amdrec_ivfpq_scan_finite(p, 6, p, p, p, 100, 1000, p, 10, p, p, 130, 32, p, p, p, 40, p, 1000, 0, None) == -1
    assert b"m=6" in lib.amdrec_last_error()
    assert lib.amdrec_ivfpq_scan_finite(p, 8, p, p, p, 100, 1000, p, 10, p, p, 130, 16, p, p, p, 40, p, 1000, 0, None) == -1
    assert lib.amdrec_ivfpq_scan_finite(p, 8, p, p, p, 100, 1000, p, 10, p, p, 70000, 32, p, p, p, 40, p, 1000, 0, None) == -1
    assert lib.amdrec_ivfpq_scan_finite(p, 8, p, p, None, 100, 1000, p, 10, p, p, 130, 32, p, p, p, 40, p, 1000, 0, None) == -1
    assert b"list_finite" in lib.amdrec_last_error()
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


def test_oracle_encode_does_not_depend_on_its_chunk():
    """The broadcast chunk is sized by dsub (chunk x 256 x dsub float64); the codes are the same for any chunk."""
    rng = np.random.default_rng(21)
    for d, m in ((2048, 4), (96, 8)):
        dsub = d // m
        cb = rng.standard_normal((m, 256, dsub))
        cent = rng.standard_normal((3, d))
        x = rng.standard_normal((150, d))
        assign = rng.integers(0, 3, 150)
        ref = ivfpq_oracle.encode(x, assign, cent, cb)
        for chunk in (1, 7, 64, 4096):
            assert np.array_equal(ivfpq_oracle.encode(x, assign, cent, cb, chunk=chunk), ref), (d, m, chunk)
    assert ivfpq_oracle.ENCODE_CHUNK_ELEMS // (256 * 512) * 256 * 512 * 8 <= 64 << 20     # <= 64 MiB at dsub 512


@pytest.mark.parametrize("dsub", [4, 12, 48, 512])
def test_oracle_tolerances_bound_an_fp32_table_and_sum(dsub):
    """table_tol / dist_tol hold for an fp32 evaluation of the kernels' order of operations (q - c, then - C, squares summed
    in dimension order; here with a rounded product and a rounded add, looser than one fma), including entries near zero
    (a codeword at the residual) where only the cancellation term bounds the error."""
    rng = np.random.default_rng(dsub)
    m = 4
    d = m * dsub
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)     # noqa: E731
    q, c = unit(rng.standard_normal(d)).astype(np.float32), unit(rng.standard_normal(d)).astype(np.float32)
    cb = (0.3 * rng.standard_normal((m, 256, dsub))).astype(np.float32)
    r32 = (q - c).astype(np.float32)
    cb[:, 0] = r32.reshape(m, dsub)                                      # exact zero
    cb[:, 1] = (r32.reshape(m, dsub) + np.float32(1e-4) * rng.standard_normal((m, dsub))).astype(np.float32)
    lut64 = ivfpq_oracle.tables(q, c, cb)
    acc = np.zeros((m, 256), np.float32)
    for i in range(dsub):
        df = (r32.reshape(m, 1, dsub)[:, :, i] - cb[:, :, i]).astype(np.float32)
        acc = (acc + (df * df).astype(np.float32)).astype(np.float32)
    err = np.abs(acc.astype(np.float64) - lut64)
    assert (err <= ivfpq_oracle.table_tol(lut64, dsub)).all(), float((err / ivfpq_oracle.table_tol(lut64, dsub)).max())
    codes = rng.integers(0, 256, (500, m))
    codes[0], codes[1] = 0, 1                                            # sums of (near-)zero entries
    D64 = lut64[np.arange(m)[None, :], codes].sum(1)
    D32 = np.zeros(500, np.float32)
    for s in range(m):
        D32 = (D32 + acc[s][codes[:, s]]).astype(np.float32)
    derr = np.abs(D32.astype(np.float64) - D64)
    assert (derr <= ivfpq_oracle.dist_tol(D64, d, m)).all()
    # and it is a bound, not a blanket: a table error of 1e-3 at an O(1) entry is outside it
    assert not (1e-3 <= ivfpq_oracle.table_tol(np.float64(1.0), dsub))


def test_oracle_adc_search_ranks_non_finite_rows_last_at_inf():
    rng = np.random.default_rng(5)
    d, m = 32, 8
    cb = rng.standard_normal((m, 256, d // m))
    cent = rng.standard_normal((2, d))
    assign = rng.integers(0, 2, 40)
    codes = rng.integers(0, 256, (40, m)).astype(np.uint8)
    fin = np.ones(40, bool)
    fin[[3, 17]] = False
    xq = rng.standard_normal((2, d))
    D, I = ivfpq_oracle.adc_search(codes, assign, cent, cb, xq, 45, 2, finite=fin)
    assert np.isfinite(D[:, :38]).all() and np.isinf(D[:, 38:]).all()
    assert all(sorted(I[q, 38:40].tolist()) == [3, 17] for q in range(2)) and (I[:, 40:] == -1).all()
    D0, I0 = ivfpq_oracle.adc_search(codes, assign, cent, cb, xq, 45, 2)
    keep = ~np.isin(I0, [3, 17])
    assert np.array_equal(I0[keep].reshape(2, -1)[:, :38], I[:, :38])


def test_search_nprobe_is_clamped_to_nlist_and_refused_beyond_max_k():
    """IVF and IVFPQ searches take min(nprobe, nlist) probes (faiss's IndexIVF::search); more than AMDREC_MAX_K probes
    after the clamp raise a ValueError that names the limit, before anything reaches the device."""
    from amdrec import _lib as L
    from amdrec.ivf import search_nprobe
    assert search_nprobe(66, 16) == 16 and search_nprobe(10, 100) == 10 and search_nprobe(0, 16) == 1
    assert search_nprobe(5000, L.MAX_K) == L.MAX_K
    with pytest.raises(ValueError, match="AMDREC_MAX_K = 2048"):
        search_nprobe(2100, 3000)
