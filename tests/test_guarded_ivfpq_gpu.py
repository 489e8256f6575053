"""GPU: IVFPQ build, code search, refine and the corpus edit inside guarded exact-size buffers (tests/guarded.py).

Build (amdrec_ivf_kmeans_step, amdrec_ivfpq_train_step, amdrec_ivf_assign's 8 * rows + 256, the encode batches) and the
corpus edit (amdrec_remove_plan) take their workspaces from ``_lib.WORKSPACE``: run under ``both_ways``.  The code search
carves the scan workspace in Python: run with every field in a block of its own (SplitScanWorkspace; the distance tables
are ``extra``) and guarded outputs.  amdrec_ivfpq_rerank's key slots and tickets never go through ``_lib.WORKSPACE``:
installed as guarded tensors of exactly their size.  Each search case is also held against its float64 oracle
(ivfpq_oracle.adc_search, ivfpq_refine_oracle.check_rerank) through the helpers of the IVFPQ surface and refine tests.

A 72-wide index has no valid ``pq_m`` (check_pq_m wants dimension / pq_m to be a multiple of 4 with pq_m in 4, 8, 16, 32):
asserted below; the second dimension here is 96 with pq_m 8 (sub-spaces of 12), the nearest shape that is not a power of two."""
import numpy as np
import pytest
import torch

from amdrec import _lib
from tests.guarded import SplitScanWorkspace, both_ways, guarded
from tests.test_ivfpq_gpu import _clustered, _normalized_on_device
from tests.test_ivfpq_refine_gpu import EXCUSED_CAP, _check, _pair
from tests.test_ivfpq_surface_gpu import _check_scaled

pytestmark = pytest.mark.gpu

ROWS, NLIST, NPROBE, M = 3000, 16, 4, 8
DIMS = (64, 96)


def test_dimension_72_has_no_product_quantizer():
    from amdrec import ivfpq
    from amdrec.index import FAISSIndex
    for m in ivfpq.PQ_M:
        with pytest.raises(ValueError, match="pq_m must be one of"):
            FAISSIndex(72, index_type="IVFPQ", nlist=NLIST, pq_m=m)


@pytest.mark.parametrize("d", DIMS)
def test_ivfpq_train_and_add_in_exact_workspaces(d, monkeypatch):
    """train + add of 3000 rows in three encode batches, both ways: centroids, codebooks, codes and assignment bit-equal,
    every workspace served at exactly the queried size with both guards intact."""
    import ctypes as C
    from amdrec import index
    from amdrec.index import FAISSIndex
    monkeypatch.setattr(index, "ADD_BATCH", 1100)
    xb = _clustered(ROWS, d, 20, 300 + d)

    def run():
        idx = FAISSIndex(d, index_type="IVFPQ", nlist=NLIST, nprobe=NPROBE, pq_m=M)
        idx.add(xb)
        pq = idx._pq
        assert pq.ntotal == ROWS
        return pq.centroids, pq.codebooks, pq.codes, pq.assign
    arena = both_ways(run)
    sizes = [s[2] for s in arena.served]
    lib, n = _lib.load(), C.c_size_t(0)
    _lib.check(lib.amdrec_ivfpq_train_workspace(ROWS, d, M, C.byref(n)))
    assert n.value in sizes
    _lib.check(lib.amdrec_ivf_kmeans_workspace(ROWS, d, NLIST, C.byref(n)))
    assert n.value in sizes
    assert 8 * ROWS + 256 in sizes                                   # assign_rows of the PQ training sample
    assert sizes.count(8 * 1100 + 256) == 2 and 8 * 800 + 256 in sizes     # ... and of the three add batches


@pytest.fixture(scope="module")
def plain():
    made = {}

    def get(d):
        if d not in made:
            from amdrec.index import FAISSIndex
            idx = FAISSIndex(d, index_type="IVFPQ", nlist=NLIST, nprobe=NPROBE, pq_m=M)
            idx.add(_clustered(ROWS, d, 20, 300 + d))
            made[d] = idx
        return made[d]
    return get


@pytest.mark.parametrize("k", [1, 10, 700])
@pytest.mark.parametrize("nq,chunk", [(5, None), (40, None), (45, 7)])
@pytest.mark.parametrize("d", DIMS)
def test_ivfpq_code_search_in_split_buffers(plain, d, nq, chunk, k, monkeypatch):
    """IVFPQState._search_codes: tables -> group -> scan -> select with every workspace field in its own guarded block and
    guarded outputs; (45, 7): TABLE_BYTES allows 7 queries per chunk, so the tables in ``extra`` are rewritten per chunk and
    the tail chunk holds 3.  k = 700 is past the smallest probed pool."""
    from amdrec import ivfpq
    idx = plain(d)
    pq = idx._pq
    if chunk:
        monkeypatch.setattr(ivfpq, "TABLE_BYTES", chunk * NPROBE * M * ivfpq.KSUB * 4)
    xq = _clustered(nq, d, 20, 400 + d + nq)
    qn = _normalized_on_device(idx, xq)
    pos0, D0, _, _ = _check_scaled(idx, xq, k, NPROBE, qn=qn)       # the product's workspace, against adc_search
    split = SplitScanWorkspace().install(monkeypatch)
    D1, P1 = guarded((nq, k), torch.float32, qn.device, "output"), guarded((nq, k), torch.int64, qn.device, "output")
    pq._search_codes(qn, k, NPROBE, D1, P1)
    split.check()
    D1.check()
    P1.check()
    (got_chunk, _, pool_ld, coarse_bytes, extra_bytes), = split.calls
    assert got_chunk == (chunk or nq) and (chunk is None or (chunk < nq and nq % chunk))
    assert extra_bytes == got_chunk * NPROBE * M * ivfpq.KSUB * 4 and coarse_bytes > 0
    assert np.array_equal(P1.cpu().numpy(), pos0) and np.array_equal(D1.cpu().numpy().view(np.uint32), D0.view(np.uint32))
    if k == 700:
        assert (pos0 < 0).any()


@pytest.fixture(scope="module")
def refined():
    made = {}

    def get(d, kind):
        if (d, kind) not in made:
            made[d, kind] = _pair(_clustered(ROWS, d, 20, 300 + d), d=d, kind=kind, nlist=NLIST, nprobe=NPROBE, m=M)
        return made[d, kind]
    return get


# (how the launch is taken, nq): the split side; one workgroup per query (RERANK_SPLIT_MAX_QUERIES patched to 0); two
# launches of 7 and 5 queries (RERANK_MAX_QUERIES patched to 7), still with scratch and tickets
@pytest.mark.parametrize("side,nq", [("split", 5), ("one_wg", 5), ("two_launches", 12)])
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
@pytest.mark.parametrize("d", DIMS)
def test_refine_in_guarded_buffers(refined, d, kind, side, nq, monkeypatch):
    """amdrec_ivfpq_rerank behind the code search, k = 50 of k' = 200 candidates (three slices per query on the split
    side): ``_rr_scratch`` exactly nq * k' * 8 bytes and ``_rr_tickets`` exactly nq zeros, both guarded, outputs guarded, the
    code search in split buffers.  Bands intact, tickets zero again, bit-equal to the product's own allocation, and that
    run is the oracle's re-rank of the plain index's candidates."""
    from amdrec import ivfpq
    ref, plain_idx = refined(d, kind)
    pq, k = ref._pq, 50
    kc = ivfpq.refine_candidates(k, ref.refine_factor)
    assert kc == 200
    if side == "one_wg":
        monkeypatch.setattr(ivfpq, "RERANK_SPLIT_MAX_QUERIES", 0)
    if side == "two_launches":
        monkeypatch.setattr(ivfpq, "RERANK_MAX_QUERIES", 7)
    uses_scratch = nq <= ivfpq.RERANK_SPLIT_MAX_QUERIES
    assert uses_scratch == (side != "one_wg") and (nq > ivfpq.RERANK_MAX_QUERIES) == (side == "two_launches")
    xq = _clustered(nq, d, 20, 500 + d + nq)
    pq._rr_scratch = pq._rr_tickets = None
    ex, total, _, pos0, D0 = _check(ref, plain_idx, xq, k)           # the product's own allocation, against check_rerank
    assert ex <= max(2, EXCUSED_CAP * total)
    assert (pq._rr_scratch is not None) == uses_scratch
    assert not bool(pq._rr_tickets.any()), "the product's own tickets were left non-zero"
    qn = _normalized_on_device(ref, xq)
    scratch = guarded((nq * kc * 8,), torch.uint8, qn.device, "scratch")
    tickets = guarded((nq,), torch.int32, qn.device, 0)
    pq._rr_scratch, pq._rr_tickets = scratch, tickets
    try:
        split = SplitScanWorkspace().install(monkeypatch)
        D1, P1 = guarded((nq, k), torch.float32, qn.device, "output"), guarded((nq, k), torch.int64, qn.device, "output")
        pq.search(qn, k, NPROBE, D1, P1)
        split.check()
        for t in (scratch, tickets, D1, P1):
            t.check()
        assert pq._rr_scratch is scratch and pq._rr_tickets is tickets
        assert not bool(tickets.any()), "tickets not zero again on return"
        assert bool((scratch == 0xA5).all()) == (not uses_scratch)   # key slots written on the split side only
    finally:
        pq._rr_scratch = pq._rr_tickets = None
    assert np.array_equal(P1.cpu().numpy(), pos0) and np.array_equal(D1.cpu().numpy().view(np.uint32), D0.view(np.uint32))


@pytest.mark.parametrize("index_type", ["Flat", "IVFPQ"])
def test_remove_then_add_in_exact_workspaces(index_type):
    """remove_ids (amdrec_remove_plan + the row gathers) followed by add, both ways.  3000 rows, the removal set ends in the
    last row and its size leaves a partial last block; what stays is the numpy statement of the edit."""
    from amdrec.index import FAISSIndex
    d = 64
    xb, more = _clustered(ROWS, d, 20, 600), _clustered(333, d, 20, 601)
    ids = np.arange(10_000, 10_000 + ROWS)
    gone = np.concatenate([ids[5:900:7], ids[-37:]])
    new_ids = np.arange(50_000, 50_333)
    xq = _clustered(9, d, 20, 602)

    def run():
        kw = dict(nlist=NLIST, nprobe=NPROBE, pq_m=M) if index_type == "IVFPQ" else {}
        idx = FAISSIndex(d, index_type=index_type, **kw)
        idx.add(xb, ad_ids=ids.tolist())
        removed, kept = idx.remove_ids(gone.tolist(), return_kept=True)
        assert removed == len(gone)
        idx.add(more, ad_ids=new_ids.tolist())
        n = idx.index.ntotal
        assert n == ROWS - len(gone) + 333
        found, D = idx.search_device(torch.from_numpy(xq).cuda(), 20)
        stored = (idx._pq.codes, idx._pq.assign) if index_type == "IVFPQ" else (idx._xb[:n],)
        stay = ~np.isin(ids, gone)
        assert np.array_equal(kept.cpu().numpy(), np.nonzero(stay)[0])
        assert np.array_equal(idx._ids[:n].cpu().numpy(), np.concatenate([ids[stay], new_ids]))
        return (kept, idx._ids[:n], found, D, *stored)
    import ctypes as C
    arena = both_ways(run)
    need = C.c_size_t(0)
    _lib.check(_lib.load().amdrec_remove_plan_workspace(ROWS, C.byref(need)))
    assert need.value in [s[2] for s in arena.served]
