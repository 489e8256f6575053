"""GPU: IVF-Flat search on every scan path with each field of the scan workspace in a guarded block of its own
(tests/guarded.py SplitScanWorkspace), guarded outputs, and the split select's scratch and tickets at exactly their size.

``IVFState.search`` carves ONE allocation into pool, grouping scratch, pair arrays, two offset arrays (and the coarse key
table over the pool's first bytes); an arena around that allocation sees only its outer edges.  Here a scan that writes past
a query's ``pool_ld`` keys, a grouping pass that runs past ``grp``, or an offset array written one entry too far changes a
band.  Every case asserts (i) the path it means to exercise ran (profile tags / the dispatch predicates on the same
arguments), (ii) every band intact, (iii) outputs ``torch.equal`` to the run through the product's own workspace, (iv) that
run within the float64 statement of the IVF surface tests (ivf_oracle.ivf_search_nonfinite given the probes, score_tol /
topk_tau), so that two equal wrong answers do not pass."""
import numpy as np
import pytest
import torch

from amdrec import _lib
from tests import ivf_oracle as io
from tests.guarded import SplitScanWorkspace, guarded
from tests.test_ivf_surface_gpu import (_check_against_float64_nonfinite, _expected_tags, _normalized, _queries, _scan_tags)

pytestmark = pytest.mark.gpu

NLIST = 32
# rows per generating cluster = per list (the centres are installed as the quantizer): nine empty lists, one of 1700 rows
# (past two 256-row tiles, and past the 1536 rows up to which the grouped scan takes 128-row tiles), none a multiple of 256
SIZES = [1700, 0, 37, 300, 0, 130, 260, 500, 65, 0, 90, 1, 200, 0, 150, 77, 45, 0, 120, 33, 99, 0, 180, 60, 25, 0, 140, 70, 10,
         0, 110, 50]
KS = (1, 7, 600)                # k = 1, k % 4 != 0, and more than the smallest probed pool holds (under-filled slots)


def _build(dim, bad_rows):
    from amdrec.index import FAISSIndex
    xb, centres = io.clustered(sum(SIZES), dim, NLIST, 4000 + dim, spread=0.2, sizes=SIZES, return_centres=True)
    if bad_rows:
        xb[11] = np.nan
        xb[2222, 3] = np.inf
    idx = FAISSIndex(dim, index_type="IVF", nlist=NLIST, nprobe=4)
    idx.set_trained_centroids(centres)
    idx.add(xb)
    lens = np.bincount(idx._ivf.assign.cpu().numpy(), minlength=NLIST)
    assert (lens == 0).sum() >= 5 and lens.max() > 1536 and not (lens[lens > 0] % 256 == 0).any(), lens
    return idx, centres


@pytest.fixture(scope="module")
def indexes():
    """(dim, rows with a NaN row and an inf row?) -> (index, cluster centres); built on first use, kept for the module."""
    made = {}

    def get(dim, bad_rows=False):
        if (dim, bad_rows) not in made:
            made[dim, bad_rows] = _build(dim, bad_rows)
        return made[dim, bad_rows]
    return get


def _run(idx, qn, k, nprobe, guard):
    """IVFState.search called directly -> (scores, positions); ``guard``: the outputs are guarded tensors (NaN / sentinel)."""
    nq, dev = qn.shape[0], qn.device
    if guard:
        D, P = guarded((nq, k), torch.float32, dev, "output"), guarded((nq, k), torch.int64, dev, "output")
    else:
        D, P = torch.empty((nq, k), device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)
    idx._ivf.search(idx._xb, idx._n, qn, k, nprobe, D, P)
    return D, P


def _tags_of(run):
    _lib.profile_enable(True)
    try:
        out = run()
        torch.cuda.synchronize()
        tags = {t: int(e["launches"]) for t, e in _lib.profile_report().items()}
    finally:
        _lib.profile_enable(False)
    return out, _scan_tags(tags)


def _both(idx, qn, k, nprobe, monkeypatch, want_tags, chunk=None):
    """One search through the product's workspace (tags, float64 statement), one in split guarded buffers (tags, bands,
    equality).  -> the split workspace and the positions."""
    idx.index.nprobe = nprobe
    (D0, P0), tags = _tags_of(lambda: _run(idx, qn, k, nprobe, False))
    assert tags == want_tags, tags
    _check_against_float64_nonfinite(idx, qn, k, nprobe, P0.cpu().numpy(), D0.cpu().numpy())
    with monkeypatch.context() as m:
        split = SplitScanWorkspace().install(m)
        (D1, P1), tags = _tags_of(lambda: _run(idx, qn, k, nprobe, True))
        split.check()
        D1.check()
        P1.check()
    assert tags == want_tags, tags
    assert len(split.calls) == 1 and (chunk is None or split.calls[0][0] == chunk), split.calls
    assert split.calls[0][3] > 0                                     # the coarse key table had a block of its own
    assert torch.equal(P1, P0) and torch.equal(D1.view(torch.int32), D0.view(torch.int32))
    return split, P0


def _rows_tile(idx):
    """Rows per workgroup of the grouped scan: 128 up to a longest list of 1536 rows, 256 beyond."""
    return 128 if int(torch.bincount(idx._ivf.assign).max()) <= 1536 else 256


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", [64, 72])
def test_pair_scan_and_grouped_one_phase_in_split_buffers(indexes, dim, k, monkeypatch):
    """5 queries x 4 probes: amdrec_ivf_scan (nq < GROUPED_MIN_QUERIES); 40 queries x 4 probes: one unfiltered
    amdrec_ivf_scan_grouped launch on the 32-query tile (160 pairs < SPARSE_PAIRS_PER_LIST * nlist)."""
    from amdrec import ivf
    idx, centres = indexes(dim)
    qn = _normalized(idx, _queries(centres, 5, 10 + dim))
    assert not ivf.use_grouped_scan(5, 4, NLIST)
    _, pos = _both(idx, qn, k, 4, monkeypatch, _expected_tags("pairs"))
    under = bool((pos < 0).any())
    qn = _normalized(idx, _queries(centres, 40, 20 + dim))
    assert ivf.use_grouped_scan(40, 4, NLIST) and 4 < ivf.TWO_PHASE_MIN_PROBES and 160 < ivf.SPARSE_PAIRS_PER_LIST * NLIST
    _, pos = _both(idx, qn, k, 4, monkeypatch, _expected_tags("grouped", 32, _rows_tile(idx)))
    assert (under or bool((pos < 0).any())) == (k == 600)            # k past the smallest probed pool leaves -1 slots


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("nq", [40, 64])
@pytest.mark.parametrize("mixed,bad_rows", [(0, False), (1, False), (1, True)])
@pytest.mark.parametrize("dim", [64, 72])
def test_two_phase_scan_in_split_buffers(indexes, dim, mixed, bad_rows, nq, k, monkeypatch):
    """32 lists, 16 probes: the nearest two probes unfiltered, select, tau, then the other fourteen filtered and appended
    behind the first phase's keys through the fill counter.  40 queries: both phases on the 32-query tile; 64 queries: the
    second phase's 896 pairs reach SPARSE_PAIRS_PER_LIST * nlist and take the 64-query tile.  AMDREC_IVF_MIXED=1: the second
    phase on the bf16 shadow; with a NaN row and an inf row in the lists the shadow's max norm is non-finite, tau_lo is -inf
    and every second-phase row is nominated (the per-lane overflow path).  k = 600: most first phases hold fewer rows, tau is
    -inf and the second phase appends every row it scans - the pool filled to its bound.  That case found the prefilter's
    one-lane re-score (nominations that miss the tile's LDS list, a race for its slots) summing in another order than the
    quarter-wave one: score bits changed from run to run until EpiIvfPrefilter::rescore1 took rescore16's order."""
    from amdrec import ivf
    idx, centres = indexes(dim, bad_rows)
    monkeypatch.setenv("AMDREC_IVF_MIXED", str(mixed))
    nprobe, rows = 16, _rows_tile(idx)
    n_first = ivf.first_phase_probes(nprobe)
    assert ivf.use_grouped_scan(nq, nprobe, NLIST) and nprobe >= ivf.TWO_PHASE_MIN_PROBES and n_first == 2
    sparse = ivf.SPARSE_PAIRS_PER_LIST * NLIST
    assert nq * n_first < sparse and (nq * (nprobe - n_first) >= sparse) == (nq == 64)
    second = 64 if nq == 64 else 32
    assert ivf.use_mixed_scan(idx._n, NLIST, nprobe, k) == bool(mixed) and dim % 8 == 0
    if mixed:
        want = {f"ivf_scan_grouped_32x{rows}": 1, f"ivf_scan_grouped_bf16_{second}x{rows}": 1, "ivf_filter_bounds": 1}
    elif second == 32:
        want = {f"ivf_scan_grouped_32x{rows}": 2}
    else:
        want = {f"ivf_scan_grouped_32x{rows}": 1, f"ivf_scan_grouped_64x{rows}": 1}
    qn = _normalized(idx, _queries(centres, nq, 30 + dim + nq))
    _both(idx, qn, k, nprobe, monkeypatch, want)
    if bad_rows:
        _, mx = idx._ivf._list_shadow()
        assert not bool(torch.isfinite(mx).all())


@pytest.mark.parametrize("dim", [64, 72])
def test_query_chunks_restart_at_pool_row_zero_in_split_buffers(indexes, dim, monkeypatch):
    """POOL_BYTES small enough that chunk < nq with a shorter tail chunk (m changes, the pool is refilled from row 0): 10
    queries in chunks of 3 through the pair scan, 45 queries in chunks of 7 through the two-phase scan (fp32 and mixed).
    The pool block is exactly r256(chunk * pool_ld * 8) bytes."""
    from amdrec import ivf
    idx, centres = indexes(dim)
    st, rows = idx._ivf, _rows_tile(idx)
    for nq, nprobe, chunk, mixed in [(10, 4, 3, 0), (45, 16, 7, 0), (45, 16, 7, 1)]:
        monkeypatch.setenv("AMDREC_IVF_MIXED", str(mixed))
        pool_ld = st.pool_rows_bound(nprobe)
        monkeypatch.setattr(ivf, "POOL_BYTES", chunk * pool_ld * 8 + 8)
        assert st.coarse_table_bytes(nq, nprobe) > 0 and nq % chunk and chunk < nq
        nchunks = -(-nq // chunk)
        if nprobe == 4:
            assert not ivf.use_grouped_scan(nq, nprobe, NLIST)
            want = {"ivf_scan_pairs": nchunks}
        elif mixed:
            want = {f"ivf_scan_grouped_32x{rows}": nchunks, f"ivf_scan_grouped_bf16_32x{rows}": nchunks,
                    "ivf_filter_bounds": nchunks}
        else:
            want = {f"ivf_scan_grouped_32x{rows}": 2 * nchunks}
        qn = _normalized(idx, _queries(centres, nq, 40 + dim + nq))
        split, _ = _both(idx, qn, 50, nprobe, monkeypatch, want, chunk=chunk)
        pool = split.fields[1]
        assert pool.numel() == (chunk * pool_ld * 8 + 255) // 256 * 256


@pytest.fixture(scope="module")
def big_lists():
    """20 000 rows of dim 64 in 4 lists: every list probed, the pool bound is the whole corpus (>= 4 * SELECT_SLICE_KEYS)."""
    from amdrec.index import FAISSIndex
    xb, centres = io.clustered(20_000, 64, 4, 77, return_centres=True)
    idx = FAISSIndex(64, index_type="IVF", nlist=4, nprobe=4)
    idx.set_trained_centroids(centres)
    idx.add(xb)
    return idx, centres


@pytest.mark.parametrize("k", [1, 10, 150])
def test_split_select_scratch_and_tickets_at_exactly_their_size(big_lists, k, monkeypatch):
    """amdrec_ivf_select_split (3 queries, 4 slices each): ``_sel_scratch`` installed as a guarded view of exactly
    m * slices * k * 8 bytes, ``_sel_tickets`` as exactly m guarded zeros.  Bands intact, tickets zero again on return (the
    product's own, usually larger, allocation too), results equal to the run with the product's allocation."""
    from amdrec import ivf
    idx, centres = big_lists
    st, m, nprobe = idx._ivf, 3, 4
    qn = _normalized(idx, _queries(centres, m, 50 + k))
    idx.index.nprobe = nprobe
    st._sel_scratch = st._sel_tickets = None
    (D0, P0), tags = _tags_of(lambda: _run(idx, qn, k, nprobe, False))
    assert tags == _expected_tags("pairs"), tags
    pool_ld = st.pool_rows_bound(nprobe)
    slices = min(ivf.SELECT_MAX_SLICES, pool_ld // ivf.SELECT_SLICE_KEYS, 1024 // m)
    assert pool_ld >= 4 * ivf.SELECT_SLICE_KEYS and slices >= 4
    assert st._sel_scratch is not None and st._sel_tickets.numel() >= m       # the split select ran and allocated them
    assert not bool(st._sel_tickets.any()), "the product's own tickets were left non-zero"
    _check_against_float64_nonfinite(idx, qn, k, nprobe, P0.cpu().numpy(), D0.cpu().numpy())
    scratch = guarded((m * slices * k * 8,), torch.uint8, qn.device, "scratch")
    tickets = guarded((m,), torch.int32, qn.device, 0)
    st._sel_scratch, st._sel_tickets = scratch, tickets
    try:
        with monkeypatch.context() as mp:
            split = SplitScanWorkspace().install(mp)
            D1, P1 = _run(idx, qn, k, nprobe, True)
            split.check()
        for t in (scratch, tickets, D1, P1):
            t.check()
        assert st._sel_scratch is scratch and st._sel_tickets is tickets      # exactly enough: the product kept them
        assert not bool(tickets.any()), "tickets not zero again on return"
        assert not bool((scratch == 0xA5).all())                              # the partial lists were written there
    finally:
        st._sel_scratch = st._sel_tickets = None
    assert torch.equal(P1, P0) and torch.equal(D1.view(torch.int32), D0.view(torch.int32))
