"""CPU: the host side of the per-request eligibility masks (amdrec.eligible) - word conversion, the numpy statement of the
contract, the tests' oracle, the near-tie cap of the GPU surface's inputs, and the refusals of the two C entries and of the
index types that do not take masks.  No GPU: every C call returns before its first HIP call."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from amdrec import _lib, eligible as el
from tests import cases, eligible_oracle as eo, flat_oracle

GPU_DIMS, GPU_KS, GPU_ROWS, GPU_NQ, TAG_SEED = (256, 32, 72, 100), (10, 100), 20_000, 513, 901


def test_as_words_round_trips_all_64_bits():
    vals = [0, 1, 1 << 32, 1 << 63, (1 << 64) - 1, -1, -(1 << 63)]
    w = el.as_words(vals, len(vals))
    assert w.dtype == np.int64 and w.shape == (len(vals),)
    assert [int(x) & ((1 << 64) - 1) for x in w] == [v & ((1 << 64) - 1) for v in vals]
    assert int(el.as_words([1 << 63], 1)[0]) == -(1 << 63) and int(el.as_words([(1 << 64) - 1], 1)[0]) == -1
    u = np.array([1 << 63, (1 << 64) - 1, 5], dtype=np.uint64)
    assert np.array_equal(el.as_words(u, 3).view(np.uint64), u)
    i = np.array([-(1 << 63), -1, 5], dtype=np.int64)
    assert np.array_equal(el.as_words(i, 3), i) and np.array_equal(el.as_words(torch.from_numpy(i), 3), i)
    assert np.array_equal(el.as_words(1 << 63, 3).view(np.uint64), np.full(3, 1 << 63, dtype=np.uint64))
    assert el.as_words([], 0).shape == (0,)


@pytest.mark.parametrize("bad, exc", [([1.0, 2.0], TypeError), (np.zeros(2, dtype=np.float32), TypeError),
                                      (np.zeros(2, dtype=np.int32), TypeError), (torch.zeros(2), TypeError),
                                      ([True, False], TypeError), (1.5, TypeError), ([1, 2, 3], ValueError),
                                      (np.zeros(3, dtype=np.uint64), ValueError), ([1 << 64, 0], ValueError),
                                      ([-(1 << 63) - 1, 0], ValueError)])
def test_as_words_refuses_floats_and_wrong_lengths(bad, exc):
    with pytest.raises(exc):
        el.as_words(bad, 2)


def test_eligible_matches_a_bit_by_bit_loop():
    rng = np.random.default_rng(5)
    bits = (0, 5, 31, 32, 63)

    def word(p):
        return sum(1 << b for b in bits if rng.random() < p)
    tags = [word(0.5) for _ in range(200)] + [0, (1 << 64) - 1]
    alls = [word(0.3) for _ in range(40)] + [0, 0, 1 << 63]
    anys = [word(0.3) for _ in range(40)] + [0, 1 << 63, 0]
    got = el.eligible(tags, alls, anys)
    assert got.shape == (len(alls), len(tags)) and got.dtype == bool
    for (q, (a, y)), (r, t) in itertools.product(enumerate(zip(alls, anys)), enumerate(tags)):
        has_all = all((t >> b) & 1 for b in range(64) if (a >> b) & 1)
        has_any = y == 0 or any((t >> b) & 1 for b in range(64) if (y >> b) & 1)
        assert got[q, r] == (has_all and has_any), (q, r)
    assert got[40].all()                                              # all = any = 0 admits every row


def test_seeded_tags_and_classes():
    tags = eo.tags_for(GPU_ROWS, TAG_SEED)
    assert tags.dtype == np.uint64 and not (tags & ~np.uint64(eo.B0 | eo.B32 | eo.B63)).any()
    assert tuple(len(eo.class_rows(tags, c)) for c in range(7)) == eo.CLASS_ROWS_20000
    a, y = eo.masks_for(15)
    assert [(int(u), int(v)) for u, v in zip(a, y)] == [eo.CLASSES[q % 7] for q in range(15)]


def test_expected_matches_brute_force():
    n, nq, k, dim = 300, 21, 12, 32
    xb, xq = flat_oracle.case_inputs(dict(n=n, dim=dim, nq=nq, kind="lifted", seed=3))
    tags = eo.tags_for(n, 7)
    a, y = eo.masks_for(nq)
    D, I = eo.expected(xb, xq, k, tags, a, y)
    s = (xq.astype(np.float64) @ xb.astype(np.float64).T).astype(np.float32)
    ok = el.eligible(tags, a, y)
    for q in range(nq):
        rows = [r for r in range(n) if ok[q, r]]
        rows.sort(key=lambda r: (-float(s[q, r]), r))
        rows = rows[:k]
        assert I[q].tolist() == rows + [-1] * (k - len(rows))
        assert D[q, :len(rows)].tolist() == [s[q, r] for r in rows] and np.all(np.isneginf(D[q, len(rows):]))
    assert (I[5::7] == -1).all()                                       # class 5: nothing is eligible


@pytest.mark.parametrize("dim", GPU_DIMS)
def test_near_tie_cap_of_the_gpu_surface(dim):
    """At most 2 % of the 513 queries may have their (k + 1)-th ELIGIBLE score inside cases.TOPK_TAU of the k-th without
    equalling it - what oracle.search.check_topk lets slip (the flat surface's rule, flat_oracle.loose_queries)."""
    xb, xq = flat_oracle.case_inputs(dict(n=GPU_ROWS, dim=dim, nq=GPU_NQ, kind="lifted", seed=1))
    tags = eo.tags_for(GPU_ROWS, TAG_SEED)
    a, y = eo.masks_for(GPU_NQ)
    for k in GPU_KS:
        D, _ = eo.expected(xb, xq, k + 1, tags, a, y)
        with np.errstate(invalid="ignore"):                                # (-inf) - (-inf): fewer than k eligible rows
            gap = D[:, k - 1].astype(np.float64) - D[:, k].astype(np.float64)
        loose = int((np.isfinite(D[:, k]) & (gap <= cases.TOPK_TAU) & (gap > 0)).sum())
        print(f"dim {dim} k {k}: {loose} of {GPU_NQ} queries inside the near-tie band")
        assert loose <= 0.02 * GPU_NQ


def _fake_pointer():
    raw = ctypes.create_string_buffer(4096 + 256)
    return raw, (ctypes.addressof(raw) + 255) // 256 * 256            # non-null, aligned, never dereferenced


def test_eligible_entries_refuse_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    raw, p = _fake_pointer()

    def fp32(k=5, nq=1, tags=p, ma=p, my=p, dim=256):
        return lib.amdrec_flat_search_eligible(p, 10, 256, dim, p, nq, 256, k, 0, p, p, None, 0, None, None, tags, ma, my)

    def mixed(k=5, nq=1, tags=p, ma=p, my=p, dim=256):
        return lib.amdrec_flat_search_mixed_eligible(p, 10, 256, dim, p, 256, p, p, nq, 256, k, 0, p, p, None, 0, None, None,
                                                     tags, ma, my)
    for call in (fp32, mixed):
        assert call(tags=None) == -1 and b"tags is null" in lib.amdrec_last_error()
        assert call(ma=None) == -1 and b"require_all" in lib.amdrec_last_error()
        assert call(my=None) == -1 and b"require_any" in lib.amdrec_last_error()
        assert call(tags=p + 4) == -1 and b"8-byte aligned" in lib.amdrec_last_error()
        assert call(k=0) == -1 and b"k=0" in lib.amdrec_last_error()
        assert call(k=_lib.MAX_K + 1) == -1 and b"k=" in lib.amdrec_last_error()
        assert call(dim=250) == -1 and b"multiple of" in lib.amdrec_last_error()
        assert call(nq=0, tags=None, ma=None, my=None) == 0               # nq = 0: nothing to do
        # every argument good: the next refusal is the (missing) workspace, still before the first HIP call
        assert call() != 0 and b"workspace" in lib.amdrec_last_error()
    del raw


@pytest.mark.parametrize("index_type", ["IVF", "IVFPQ"])
def test_ivf_indexes_refuse_masks_before_the_library_is_touched(index_type, monkeypatch):
    """The refusal does not depend on a device or on the library: an index object that was never constructed (only its type
    is set) raises from every search entry, and the message names the follow-up."""
    from amdrec.index import FAISSIndex
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    idx = object.__new__(FAISSIndex)
    idx.index_type = index_type
    q = np.zeros((2, 8), dtype=np.float32)
    for call in (lambda: idx.search_device(q, 3, require_all=torch.zeros(2, dtype=torch.int64)),
                 lambda: idx.search_device(q, 3, require_any=torch.zeros(2, dtype=torch.int64)),
                 lambda: idx.search(q, 3, require_all=[1, 1]), lambda: idx.batch_search(q, 3, require_any=1)):
        with pytest.raises(NotImplementedError, match="follow-up"):
            call()
