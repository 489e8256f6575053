"""IVF-Flat state for ``FAISSIndex(index_type='IVF')`` (faiss_retrieval.py:50-55): coarse centroids,
list assignment, list-contiguous copy of the corpus, and the search driver over libamdrec's
``amdrec_ivf_coarse_keys`` (coarse probes) + ``amdrec_ivf_group`` + ``amdrec_ivf_scan[_grouped]`` + ``amdrec_ivf_select``.
``InvertedLists`` is the coarse level that IVFPQ shares (amdrec.ivfpq holds one); ``IVFState`` adds the fp32 lists' scans.

Build and search are hand-written HIP: assignment = ``amdrec_ivf_assign`` (fp32-MFMA GEMM with an arg-max epilogue),
training = ``amdrec_ivf_kmeans_step`` x NITER (assignment + order-independent fixed-point centroid sums: training is
bit-reproducible), and a search call launches only libamdrec kernels (no ATen op, no host synchronisation: it can be
captured in a HIP graph).  What stays in torch is build-time data plumbing: drawing the training sample and the one
stable sort that lays the corpus out list-contiguously after an ``add``.
faiss' own k-means (its sub-sampling, seeding and iteration details) is not reproducible offline, so, as SURVEY.md
section 8c says, IVF parity is: (i) the scan is exact over the probed lists given this build's centroids and
assignments (tested against the oracle), (ii) recall@k against the Flat result is reported.
Trainer: spherical Lloyd, max-inner-product assignment (the quantizer is IndexFlatIP), <= 256
training points per centroid, 10 iterations, seed 1234 (faiss' documented defaults).
Search = coarse probes -> [nearest eighth of the probes: grouped scan -> select -> tau] -> [other probes: grouped scan keeping
score >= tau] -> select (exact: tau is the k-th score over a subset of the candidates, hence a lower bound of the final one).
Eligibility masks (opt-in, ``FAISSIndex(list_tags=True)``): ``InvertedLists`` also keeps the tag words in list order and every
scan of a masked search is its ``*_eligible`` twin ("Eligibility masks in the inverted-list scans").
Stage-1 score boosts (opt-in, ``FAISSIndex(list_boosts=True)``): ``InvertedLists`` also keeps the boosts in list order and
every scan of a boosted search is its ``*_boosted`` twin - same probes, same phases, the key s = ip + w_q * boost[r] where
the plain scan files ip ("Stage-1 score boosts in the inverted-list scans").
Aware probes (opt-in, ``FAISSIndex(aware_probes=True)``): ``InvertedLists`` also keeps per-list summaries of those two copies
(``amdrec_ivf_list_summaries``) and the coarse step of a masked / boosted search picks the nprobe best FEASIBLE lists
(``amdrec_ivf_coarse_keys_aware``; amdrec.probes has the rule; DESIGN.md, "Aware probes").  The scans are untouched.
Sharding: the centroids are SHARED by all ranks (``amdrec.sharded.share_ivf_centroids``); a rank
files its own rows under them and holds its slice of every list, so the union of the ranks' scans is exactly the
unsharded scan and the merged top-k is bit-identical to the unsharded IVF result.
"""
from __future__ import annotations

import os
from collections import namedtuple
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .rows_edit import gather_rows

NITER = 10
MAX_POINTS_PER_CENTROID = 256
SEED = 1234
POOL_BYTES = 2 << 30           # candidate-pool workspace per query chunk
GROUPED_MIN_QUERIES = 16       # batches at least this large MAY scan list-major (every list read once per query tile) ...
GROUPED_MIN_PAIRS_PER_LIST = 3.0   # ... if a probed list is shared by at least this many of the batch's queries on average
QTILE = 64                     # queries per grouped-scan tile (ShapeIvf::BP) ...
QTILE_SPARSE = 32              # ... or 32 (ShapeIvf32) when fewer than SPARSE_PAIRS_PER_LIST queries probe a list on average
SPARSE_PAIRS_PER_LIST = 24
MAX_QUERY_TILES = 65535        # grid limit of one amdrec_ivf_scan_grouped launch (pairs / tile + nlist query tiles)
SELECT_SLICE_KEYS = 4096        # amdrec_ivf_select_split: at least this many pool keys per slice,
SELECT_MAX_SLICES = 64          # at most this many slices per query
MIXED_SCAN = True              # second phase of the two-phase scan on a bf16 shadow of the lists (prefilter) + fp32 re-score of
                               # the nominated rows (csrc/ivf.hip EpiIvfPrefilter); the shadow costs half the lists' bytes again.
                               # AMDREC_IVF_MIXED=0 / 1 in the environment forces it off / on (A/B runs)
MIXED_MIN_FIRST_ROWS_PER_K = 32  # ... only when the first phase scans at least this many rows per wanted result: the prefilter
                               # pays when tau is selective (10M ads / 4096 lists, k = 500: 19.5k first-phase rows, second phase
                               # 0.77 -> 0.43 ms); when it is not, every row that passes costs a random 1 KB fp32 row read (a
                               # rank of 8 over the same index, k = 128 against 2440 first-phase rows of weakly separated
                               # 305-row lists: 0.64 -> 0.60 ms, profiles/r04_ivf_mixed_ab.log) - not worth the shadow's bytes
TWO_PHASE_MIN_PROBES = 16      # from here on the scan is split: nearest probes unfiltered, the rest filtered by their k-th score (at 10 probes it loses: 0.78 vs 0.41 ms at 64 queries, nlist 100)


def _normalize(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)


def _assign(x: torch.Tensor, cent: torch.Tensor) -> torch.Tensor:
    """amdrec_ivf_assign: arg max_c <x, c> per row (ties -> lower centroid)."""
    lib = _lib.load()
    x = x.contiguous()
    n = x.shape[0]
    out = torch.empty(n, dtype=torch.int64, device=x.device)
    if n == 0:
        return out
    ws = _lib.WORKSPACE.get(n * 8 + 256, x.device)
    _lib.check(lib.amdrec_ivf_assign(_lib.ptr(x), n, x.stride(0), x.shape[1], _lib.ptr(cent), cent.shape[0],
                                     cent.stride(0), _lib.ptr(out), None, _lib.ptr(ws), ws.numel(),
                                     _lib.stream_ptr(x.device)))
    return out


def first_phase_probes(nprobe: int) -> int:
    """Probes of the two-phase scan's unfiltered first phase: the nearest eighth (AMDREC_IVF_FIRST_DIV overrides the 8 for
    A/B runs)."""
    return max(2, nprobe // max(1, int(os.environ.get("AMDREC_IVF_FIRST_DIV", "8"))))


def use_mixed_scan(n: int, nlist: int, nprobe: int, k: int) -> bool:
    """Second phase of the two-phase scan on the bf16 shadow of the lists (prefilter + fp32 re-score of the rows that pass)?
    Only when the first phase is selective: it scans at least MIXED_MIN_FIRST_ROWS_PER_K rows per wanted result, so its k-th
    score leaves few rows of the second phase to re-score.  AMDREC_IVF_MIXED=0 / 1 forces the answer (A/B runs)."""
    force = os.environ.get("AMDREC_IVF_MIXED")
    if force in ("0", "1"):
        return force == "1"
    return MIXED_SCAN and first_phase_probes(nprobe) * (n / max(1, nlist)) >= MIXED_MIN_FIRST_ROWS_PER_K * k


def use_grouped_scan(nq: int, nprobe: int, nlist: int) -> bool:
    """List-major (grouped) scan or one workgroup set per (query, probe) pair?  The grouped scan reads a probed list once
    per query tile, the pair scan once per probing query - but at the HBM rate whatever the lists' lengths (their rows are
    split over workgroups), where the grouped kernel's (list, query tile, 256 rows) workgroups run ~3x slower than their
    bytes on short or thinly shared lists (1M ads, nlist 4096, nprobe 64, 64 queries: 1.6 queries per probed list -
    0.60 ms grouped, HBM time of the pairs' bytes 0.2).  So: grouped from GROUPED_MIN_QUERIES queries on AND only when
    the batch's (query, probe) pairs outnumber the lists they can fall on GROUPED_MIN_PAIRS_PER_LIST to one."""
    pairs = nq * nprobe
    return nq >= GROUPED_MIN_QUERIES and pairs >= GROUPED_MIN_PAIRS_PER_LIST * min(nlist, pairs)


def search_nprobe(nprobe: int, nlist: int) -> int:
    """The probes a search takes: nprobe clamped to [1, nlist], as faiss's IndexIVF::search clamps it (the stored nprobe
    is left as set).  More than AMDREC_MAX_K probes cannot be selected: refused with the limit named."""
    p = min(max(1, int(nprobe)), nlist)
    if p > _lib.MAX_K:
        raise ValueError(f"nprobe {p} (after clamping to nlist {nlist}) exceeds AMDREC_MAX_K = {_lib.MAX_K}, the most probes "
                         f"a search selects")
    return p


def grouped_chunk_limit(nlist: int, nprobe: int) -> int:
    """Largest query chunk whose grouped scan fits one launch: a launch walks at most pairs / tile + nlist query tiles
    (every list can end in a partial tile) and the tile is re-picked per (chunk, probe-column range) - a phase or a tail
    chunk may fall under the sparse threshold - so the limit is taken with the SMALLEST tile.  A quantizer with more
    lists than the grid has tiles cannot take the grouped path at all."""
    room = MAX_QUERY_TILES - nlist
    if room < 1:
        raise ValueError(f"nlist = {nlist} is beyond the grouped IVF scan's limit ({MAX_QUERY_TILES - 1} lists)")
    return max(1, (room * min(QTILE, QTILE_SPARSE)) // max(1, nprobe))


class ListLayout(NamedTuple):
    """The corpus laid out list-contiguously: rows of a list keep insertion order (flagged rows after the others)."""
    rows: torch.Tensor          # the owner's per-row payload gathered in list order (IVF: fp32 rows, IVFPQ: codes)
    spos: torch.Tensor          # [n] corpus position of every list-order row (the stable sort's permutation)
    off: torch.Tensor           # [nlist + 1] first list-order row of every list
    lens: torch.Tensor          # [nlist] rows per list
    max_len: int                # the longest list's rows
    n: int                      # rows laid out


# Views of one search workspace (InvertedLists.workspace): [pool | grouping scratch | pair arrays and offsets | extra]
ScanWorkspace = namedtuple("ScanWorkspace", "keys pool grp pair_q pair_p goff qtp extra")


class InvertedLists:
    """The coarse level shared by IVF-Flat and IVFPQ: centroids, the per-row list assignment, the list layout, the coarse
    probes, the pool select and the scan workspace.  The only code that touches any of them."""

    def __init__(self, centroids: torch.Tensor):
        self.centroids = centroids.contiguous()                    # [nlist, d], unit rows
        self.nlist, self.dim = centroids.shape
        self.coarse_ld = (self.nlist + 1) // 2 * 2                  # row pitch of the coarse key table
        self.device = centroids.device
        self.assign = torch.empty(0, dtype=torch.int64, device=self.device)   # list of every position
        self.lists: Optional[ListLayout] = None                     # made by layout(), dropped by extend()
        self._top_rows = None                                       # host: rows of the p longest lists (pool_rows_bound)
        self._nlist_count = None                                    # device: nlist per query (the coarse select's pool sizes)
        self._sel_scratch = None                                    # device: amdrec_ivf_select_split's partial lists and tickets
        self._sel_tickets = None
        # Eligibility masks in the list scans (FAISSIndex(list_tags=True)): tag_source() -> the owner's tag words in
        # insertion order (int64 [>= n]); list_tags = those words in LIST order (tags[spos], 8 bytes per row), made with the
        # layout and again when the owner swaps its tag tensor (_list_tags_of: the tensor list_tags was gathered from)
        self.tag_source = None
        self.list_tags: Optional[torch.Tensor] = None
        self._list_tags_of = None
        # Stage-1 score boosts in the list scans (FAISSIndex(list_boosts=True)), kept the same way: boost_source() -> the
        # owner's boosts in insertion order (float32 [>= n], None while it has none); list_boosts = boosts[spos], 4 bytes per row
        self.boost_source = None
        self.list_boosts: Optional[torch.Tensor] = None
        self._list_boosts_of = None
        # Aware probes (FAISSIndex(aware_probes=True); amdrec.probes has the rule): per-list summaries of the two list-order
        # copies - list_tag_or [nlist] int64 (OR of a list's tag words), list_boost_hi / list_boost_lo [nlist] float32 (max /
        # min of its boosts) - made by refresh_list_tags / refresh_list_boosts with the copy they summarise, as NEW tensors
        self.aware_probes = False
        self.list_tag_or: Optional[torch.Tensor] = None
        self.list_boost_hi: Optional[torch.Tensor] = None
        self.list_boost_lo: Optional[torch.Tensor] = None

    # -- build ----------------------------------------------------------------------------
    @classmethod
    def train(cls, x: torch.Tensor, nlist: int):
        """x: fp32 device copy of the training embeddings (un-normalised, as FAISSIndex.add passes
        them to train(), faiss_retrieval.py:107-108)."""
        x = _normalize(x.float())
        n = x.shape[0]
        if n < nlist:
            raise ValueError(f"need at least nlist={nlist} training vectors, got {n}")
        g = torch.Generator(device="cpu")
        g.manual_seed(SEED)
        if n > MAX_POINTS_PER_CENTROID * nlist:
            sel = torch.randperm(n, generator=g)[:MAX_POINTS_PER_CENTROID * nlist].to(x.device)
            x = x[sel]
            n = x.shape[0]
        order = torch.randperm(n, generator=g)
        finite = torch.isfinite(x).all(dim=1).cpu()
        if not bool(finite.all()):
            # a row with a non-finite coordinate never becomes a centroid (its scores are NaN: it would win no row, keep
            # its NaN for every iteration and leave a dead list); with finite rows only, the draw is unchanged
            order = order[finite[order]]
            if order.numel() < nlist:
                raise ValueError(f"need at least nlist={nlist} finite training vectors, got {order.numel()}")
        cent = x[order[:nlist].to(x.device)].clone().contiguous()
        x = x.contiguous()
        lib = _lib.load()
        nbytes = _lib.C.c_size_t(0)
        _lib.check(lib.amdrec_ivf_kmeans_workspace(n, x.shape[1], nlist, _lib.C.byref(nbytes)))
        ws = _lib.WORKSPACE.get(nbytes.value, x.device)
        for _ in range(NITER):                                       # Lloyd iterations, all on libamdrec kernels
            _lib.check(lib.amdrec_ivf_kmeans_step(_lib.ptr(x), n, x.stride(0), x.shape[1], _lib.ptr(cent), nlist,
                                                  cent.stride(0), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
        return cls(cent)

    def assign_rows(self, x_normalised: torch.Tensor) -> torch.Tensor:
        """The list of each L2-normalised row (not yet part of the index: ``extend``)."""
        return _assign(x_normalised, self.centroids)

    def extend(self, assigns):
        """Append the lists of new rows (``assign_rows`` results, in order): drops the layout and its bound together."""
        self.assign = torch.cat([self.assign, *assigns])
        self.lists = None
        self._top_rows = None

    def compact(self, kept: torch.Tensor):
        """Rows were removed (FAISSIndex.remove_ids): keep the list of every row in ``kept`` (old positions, ascending), as
        a NEW tensor, and drop the layout and its bound explicitly - ``lists.n != n`` alone would miss a removal that an
        add of as many rows follows.  Centroids stay: nothing is re-assigned."""
        self.assign = gather_rows(self.assign, kept)
        self.lists = None
        self._top_rows = None

    def layout(self, n: int, rows: torch.Tensor, last: Optional[torch.Tensor] = None) -> ListLayout:
        """(Re)build the list layout of rows [0, n): one stable sort by list (rows of a list keep insertion order; those
        flagged in the bool tensor ``last`` go behind the list's others); ``rows`` is the owner's per-row payload in
        insertion order.  Callers rebuild when ``lists`` is None (rows were added) or was made for another n."""
        a = self.assign[:n]
        order = torch.argsort(a if last is None else a * 2 + last[:n].to(torch.int64), stable=True)
        counts = torch.bincount(a, minlength=self.nlist)
        off = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)
        off[1:] = torch.cumsum(counts, 0)
        self.lists = ListLayout(rows[:n][order].contiguous(), order.contiguous(), off, counts.to(torch.int64),
                                int(counts.max().item()) if n else 0, n)
        # rows of the p longest lists, p = 1 .. nlist: the tight host-side bound of a query's candidate pool
        # (its nprobe probed lists cannot hold more than the nprobe longest; once per list rebuild, like max above)
        self._top_rows = np.cumsum(np.sort(counts.cpu().numpy())[::-1].astype(np.int64))
        self.list_tags = self._list_tags_of = self.list_tag_or = None
        self.refresh_list_tags()
        self.list_boosts = self._list_boosts_of = self.list_boost_hi = self.list_boost_lo = None
        self.refresh_list_boosts()
        return self.lists

    def _summaries(self, list_tags=None, list_boosts=None):
        """amdrec_ivf_list_summaries over the current layout -> (tag_or, boost_hi, boost_lo), new tensors (None where the
        input is None)."""
        dev = self.device
        tag_or = None if list_tags is None else torch.zeros(self.nlist, dtype=torch.int64, device=dev)
        hi = None if list_boosts is None else torch.zeros(self.nlist, dtype=torch.float32, device=dev)
        lo = None if list_boosts is None else torch.zeros(self.nlist, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().amdrec_ivf_list_summaries(_lib.ptr(self.lists.off), self.nlist, _lib.ptr(list_tags),
                                                         _lib.ptr(list_boosts), _lib.ptr(tag_or), _lib.ptr(hi), _lib.ptr(lo),
                                                         _lib.stream_ptr(dev)))
        return tag_or, hi, lo

    def refresh_list_tags(self) -> Optional[torch.Tensor]:
        """list_tags of the current layout from the owner's current tag tensor (amdrec_rows_gather, out of place: a search in
        flight or a captured graph keeps the copy it started with).  Nothing to do without ``tag_source``, before the first
        layout, or while the copy made from this very tensor for this very layout stands (the owner writes a tag tensor in
        place only for rows that no layout holds yet)."""
        if self.tag_source is None or self.lists is None:
            return None
        tags = self.tag_source()
        if self.list_tags is None or self._list_tags_of is not tags:
            self.list_tags = gather_rows(tags, self.lists.spos, self.lists.n)
            self._list_tags_of = tags
            self.list_tag_or = None
        if self.aware_probes and self.list_tag_or is None:           # the summary stands and falls with the copy it summarises
            self.list_tag_or = self._summaries(list_tags=self.list_tags)[0]
        return self.list_tags

    def refresh_list_boosts(self) -> Optional[torch.Tensor]:
        """list_boosts of the current layout from the owner's current boost tensor, under refresh_list_tags' rules
        (amdrec_rows_gather, out of place; a copy stands while it was made from this very tensor for this very layout)."""
        if self.boost_source is None or self.lists is None:
            return None
        boosts = self.boost_source()
        if boosts is None:                                           # an index that never saw a boost keeps no copy
            self.list_boosts = self._list_boosts_of = self.list_boost_hi = self.list_boost_lo = None
            return None
        if self.list_boosts is None or self._list_boosts_of is not boosts:
            self.list_boosts = gather_rows(boosts, self.lists.spos, self.lists.n)
            self._list_boosts_of = boosts
            self.list_boost_hi = self.list_boost_lo = None
        if self.aware_probes and self.list_boost_hi is None:
            _, self.list_boost_hi, self.list_boost_lo = self._summaries(list_boosts=self.list_boosts)
        return self.list_boosts

    def enable_aware_probes(self):
        """From now on the summaries are kept (made here for the list-order copies that already stand)."""
        self.aware_probes = True
        self.refresh_list_tags()
        self.refresh_list_boosts()

    def boost_tail(self, boost, nq: int):
        """``boost`` = (weights device float32 [nq], boost_max) -> f(s): the two trailing pointers of a *_boosted scan for the
        queries from s on (the weights are offset with the queries)."""
        if self.boost_source is None:
            raise ValueError("a stage-1 boost needs list-order boosts: FAISSIndex(list_boosts=True) or enable_list_boosts()")
        lb = self.refresh_list_boosts()
        if lb is None:
            raise ValueError("boost_weight on an index without boosts: give them with add(..., boosts=) or set_boosts()")
        w = _lib.require_gpu(boost[0], "boost_weight", torch.float32)
        if w.shape != (nq,) or not w.is_contiguous():
            raise ValueError(f"boost_weight must be a contiguous float32 [{nq}], got {tuple(w.shape)}")
        if lb.shape != (self.lists.n,):
            raise ValueError("list_boosts does not match the list layout")
        return lambda s: (_lib.ptr(lb), _lib.ptr(w[s:]))

    def elig_tail(self, elig, nq: int):
        """``elig`` = (require_all, require_any) device int64 [nq] -> f(s): the three trailing pointers of an *_eligible scan
        for the queries from s on (the masks are offset with the queries)."""
        if self.tag_source is None:
            raise ValueError("eligibility masks need list-order tags: FAISSIndex(list_tags=True) or enable_list_tags()")
        lt = self.refresh_list_tags()
        ma, my = (_lib.require_gpu(t, name, torch.int64) for t, name in zip(elig, ("require_all", "require_any")))
        for t, name in ((ma, "require_all"), (my, "require_any")):
            if t.shape != (nq,) or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous int64 [{nq}], got {tuple(t.shape)}")
        if lt.shape != (self.lists.n,):
            raise ValueError("list_tags does not match the list layout")
        return lambda s: (_lib.ptr(lt), _lib.ptr(ma[s:]), _lib.ptr(my[s:]))

    def pool_rows_bound(self, nprobe: int) -> int:
        """Upper bound of the rows a query's ``nprobe`` probed lists hold = the ``nprobe`` longest lists' rows.  Round 2
        sized the pool as nprobe x the longest list (9767 x 64 keys = 5 MB per query at 10M / 4096: 512 queries needed two
        chunks of the 2 GB pool); list lengths spread 0 .. 4x the mean, so this is ~1.6x tighter."""
        if self._top_rows is None or len(self._top_rows) == 0:
            return 1
        return max(1, int(self._top_rows[min(int(nprobe), len(self._top_rows)) - 1]))

    # -- search steps ---------------------------------------------------------------------
    def coarse_table_bytes(self, nq: int, nprobe: int) -> int:
        """Bytes of the dense (score, centroid) key table of ``nq`` queries, or 0 when the table does not fit (more than
        POOL_BYTES, more probes than a select takes, 2^24 queries): the probes then come from the flat search."""
        nbytes = nq * self.coarse_ld * 8
        return nbytes if nbytes <= POOL_BYTES and nprobe <= _lib.MAX_K and nq < (1 << 24) else 0

    def aware_table_rows(self, nq: int) -> int:
        """Queries per fill of the aware key table: all of them when their table fits POOL_BYTES, else the chunk that does (the
        flat search, the plain path's way out, cannot apply the rule)."""
        return max(1, min(nq, (1 << 24) - 1, POOL_BYTES // (self.coarse_ld * 8)))

    def aware_table_bytes(self, nq: int) -> int:
        return self.aware_table_rows(nq) * self.coarse_ld * 8

    def _aware_probes(self, q: torch.Tensor, nprobe: int, keys: Optional[torch.Tensor], elig, boost) -> torch.Tensor:
        """coarse_probes under amdrec.probes' rule: amdrec_ivf_coarse_keys_aware + the pool select (a key of 0 - an infeasible
        list - is the empty slot the select skips: fewer feasible lists than nprobe leave a -1 tail), in query chunks of
        ``aware_table_rows`` when the table of all queries does not fit."""
        if not self.aware_probes:
            raise ValueError("masks / a boost weight in the coarse step need the per-list summaries: "
                             "FAISSIndex(aware_probes=True) or enable_aware_probes()")
        if self.lists is None:
            raise ValueError("aware probes need the list layout (made by the first search after an add)")
        if nprobe > _lib.MAX_K:
            raise ValueError(f"nprobe {nprobe} exceeds AMDREC_MAX_K = {_lib.MAX_K}, the most probes a search selects")
        nq = q.shape[0]
        tag_or = ma = my = hi = lo = w = None
        if elig is not None:
            self.elig_tail(elig, nq)                                 # (validates; refreshes list_tags and with it the summary)
            tag_or, (ma, my) = self.list_tag_or, elig
        if boost is not None:
            self.boost_tail(boost, nq)
            hi, lo, w = self.list_boost_hi, self.list_boost_lo, boost[0]
        cs = torch.empty((nq, nprobe), dtype=torch.float32, device=self.device)
        probes = torch.empty((nq, nprobe), dtype=torch.int64, device=self.device)
        if not nq:
            return probes
        lib = _lib.load()
        rows = self.aware_table_rows(nq)
        nbytes = rows * self.coarse_ld * 8
        if keys is None or keys.numel() < nbytes:
            keys = _lib.WORKSPACE.get(nbytes, self.device)
        if self._nlist_count is None or self._nlist_count.numel() < rows:
            self._nlist_count = torch.full((max(rows, 512),), self.nlist, dtype=torch.int64, device=self.device)
        at = lambda t, s: None if t is None else _lib.ptr(t[s:])     # noqa: E731
        for s in range(0, nq, rows):
            m = min(rows, nq - s)
            _lib.check(lib.amdrec_ivf_coarse_keys_aware(
                _lib.ptr(self.centroids), self.nlist, self.centroids.stride(0), self.dim, _lib.ptr(q[s:]), m, q.stride(0),
                _lib.ptr(keys), self.coarse_ld, _lib.ptr(self.lists.lens), _lib.ptr(tag_or), at(ma, s), at(my, s), _lib.ptr(hi),
                _lib.ptr(lo), at(w, s), _lib.stream_ptr(self.device)))
            _lib.check(lib.amdrec_ivf_select(_lib.ptr(keys), self.coarse_ld, _lib.ptr(self._nlist_count), m, nprobe,
                                             _lib.ptr(cs[s:]), _lib.ptr(probes[s:]), _lib.stream_ptr(self.device)))
        return probes

    def coarse_probes(self, q: torch.Tensor, nprobe: int, keys: Optional[torch.Tensor] = None, elig=None,
                      boost=None) -> torch.Tensor:
        """-> int64 [nq, nprobe]: the nprobe best centroids of each query by inner product (IndexFlatIP quantizer; -1 = none).
        A dense key table (in ``keys``, else in ``coarse_table_bytes`` of the shared workspace) + the pool select, or, when
        the table does not fit, the flat search.
        ``elig`` = (require_all, require_any) device int64 [nq] and / or ``boost`` = (weights device float32 [nq], boost_max),
        on an index with ``aware_probes``: the nprobe best FEASIBLE lists under amdrec.probes' rule instead (-1 = fewer
        feasible lists than nprobe); both None: the plain path above, launch for launch."""
        if elig is not None or boost is not None:
            return self._aware_probes(q, nprobe, keys, elig, boost)
        nq, nbytes = q.shape[0], self.coarse_table_bytes(q.shape[0], nprobe)
        cs = torch.empty((nq, nprobe), dtype=torch.float32, device=self.device)
        probes = torch.empty((nq, nprobe), dtype=torch.int64, device=self.device)
        if nq and not nbytes:
            from .index import flat_search
            flat_search(self.centroids, self.nlist, q, nprobe, cs, probes)
        elif nq:
            lib = _lib.load()
            keys = _lib.WORKSPACE.get(nbytes, self.device) if keys is None else keys
            if self._nlist_count is None or self._nlist_count.numel() < nq:
                self._nlist_count = torch.full((max(nq, 512),), self.nlist, dtype=torch.int64, device=self.device)
            _lib.check(lib.amdrec_ivf_coarse_keys(_lib.ptr(self.centroids), self.nlist, self.centroids.stride(0), self.dim,
                                                  _lib.ptr(q), nq, q.stride(0), _lib.ptr(keys), self.coarse_ld,
                                                  _lib.stream_ptr(self.device)))
            _lib.check(lib.amdrec_ivf_select(_lib.ptr(keys), self.coarse_ld, _lib.ptr(self._nlist_count), nq, nprobe,
                                             _lib.ptr(cs), _lib.ptr(probes), _lib.stream_ptr(self.device)))
        return probes

    def workspace(self, chunk: int, nprobe: int, pool_ld: int, coarse_bytes: int, extra_bytes: int = 0) -> ScanWorkspace:
        """One workspace for a search whose scans take ``chunk`` queries at a time, as byte views (int64 for the pair arrays
        and the two nlist + 1 offset arrays): ``keys`` = the first ``coarse_bytes`` for the coarse key table (None if 0; it is
        done with before the first scan writes the pool), ``extra`` = the caller's trailing bytes (IVFPQ's distance tables).
        The C side trusts these sizes."""
        pairs, r256 = chunk * nprobe, lambda b: (b + 255) // 256 * 256      # noqa: E731
        pool_bytes = r256(chunk * pool_ld * 8)
        arr0 = pool_bytes + r256((self.nlist + 1) * 4) + r256(pairs * 4)
        extra0 = arr0 + r256(2 * pairs * 8 + 2 * (self.nlist + 1) * 8)
        ws = _lib.WORKSPACE.get(max(extra0 + extra_bytes + 256, coarse_bytes), self.device)
        arr = ws[arr0:extra0].view(torch.int64)
        goff = 2 * pairs
        return ScanWorkspace(ws[:coarse_bytes] if coarse_bytes else None, ws[:pool_bytes], ws[pool_bytes:arr0],
                             arr[:pairs], arr[pairs:goff], arr[goff:goff + self.nlist + 1],
                             arr[goff + self.nlist + 1:goff + 2 * (self.nlist + 1)], ws[extra0:extra0 + extra_bytes])

    def group(self, w: ScanWorkspace, probes: torch.Tensor, probe_ld: int, m: int, ncol: int, base: torch.Tensor,
              n_out: torch.Tensor, qtile: int):
        """amdrec_ivf_group: pool slots (``base``, ``n_out``) of the first ``ncol`` probe columns of ``m`` queries and
        their (query, probe) pairs grouped by list in tiles of ``qtile`` queries (kernels, no host sync)."""
        _lib.check(_lib.load().amdrec_ivf_group(
            _lib.ptr(probes), probe_ld, m, ncol, self.nlist, _lib.ptr(self.lists.lens), _lib.ptr(base), _lib.ptr(n_out),
            _lib.ptr(w.pair_q), _lib.ptr(w.pair_p), _lib.ptr(w.goff), _lib.ptr(w.qtp), qtile, _lib.ptr(w.grp), w.grp.numel(),
            _lib.stream_ptr(self.device)))

    def select(self, pool, pool_ld: int, n_pool, m: int, k: int, out_scores, out_pos):
        """The k best keys of each query's pool.  Few queries with large pools (one request against nlist 100 / nprobe 10:
        100 000 keys) are selected by several workgroups per query (``amdrec_ivf_select_split``), everything else by one."""
        lib = _lib.load()
        slices = min(SELECT_MAX_SLICES, pool_ld // SELECT_SLICE_KEYS, 1024 // max(1, m))
        if slices < 4:
            _lib.check(lib.amdrec_ivf_select(_lib.ptr(pool), pool_ld, _lib.ptr(n_pool), m, k, _lib.ptr(out_scores),
                                             _lib.ptr(out_pos), _lib.stream_ptr(self.device)))
            return
        need = m * slices * k * 8
        if self._sel_scratch is None or self._sel_scratch.numel() < need:
            self._sel_scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self._sel_tickets is None or self._sel_tickets.numel() < m:
            self._sel_tickets = torch.zeros(max(m, 1024), dtype=torch.int32, device=self.device)   # the kernel leaves them zero
        _lib.check(lib.amdrec_ivf_select_split(_lib.ptr(pool), pool_ld, _lib.ptr(n_pool), m, k, slices, _lib.ptr(out_scores),
                                               _lib.ptr(out_pos), _lib.ptr(self._sel_scratch), self._sel_scratch.numel(),
                                               _lib.ptr(self._sel_tickets), _lib.stream_ptr(self.device)))

    def resident_tensors(self) -> list:
        """Every device tensor kept between calls (a captured graph's kernels point at them)."""
        kept = [self.centroids, self.assign, self._nlist_count, self._sel_scratch, self._sel_tickets, self.list_tags,
                self.list_boosts, self.list_tag_or, self.list_boost_hi, self.list_boost_lo, *(self.lists or ())]
        return [t for t in kept if isinstance(t, torch.Tensor)]

    # -- persistence ----------------------------------------------------------------------
    def export_arrays(self):
        return [("ivf_centroids", self.centroids.cpu().numpy()), ("ivf_assign", self.assign.cpu().numpy())]

    @classmethod
    def from_arrays(cls, arrays, device):
        st = cls(torch.from_numpy(np.array(arrays["ivf_centroids"])).to(device))
        st.assign = torch.from_numpy(np.array(arrays["ivf_assign"])).to(device)
        return st


class IVFState(InvertedLists):
    """IVF-Flat: the lists hold the fp32 rows; second phases may run on a bf16 shadow of them."""

    def __init__(self, centroids: torch.Tensor):
        super().__init__(centroids)
        self._shadow = None                                         # (bf16 copy of lists.rows, its {M, D}): made on first use

    def append(self, x_normalised: torch.Tensor, start: int):
        assert start == self.assign.shape[0]
        self.extend([self.assign_rows(x_normalised)])

    def compact(self, kept: torch.Tensor):
        super().compact(kept)
        self._shadow = None

    def _build_lists(self, xb: torch.Tensor, n: int) -> ListLayout:
        if self.lists is None or self.lists.n != n:
            self.layout(n, xb)
            self._shadow = None
        return self.lists

    def _list_shadow(self):
        """bf16 (round-to-nearest) copy of the list-contiguous corpus and max_norm = {largest row norm, largest row
        rounding-error norm} (amdrec_bf16_rows): the operands of the second-phase prefilter."""
        if self._shadow is None:
            xs = self.lists.rows
            n, d = xs.shape
            xs16 = torch.empty((n, d), dtype=torch.bfloat16, device=self.device)
            mx = torch.zeros(2, dtype=torch.float32, device=self.device)
            if n:
                _lib.check(_lib.load().amdrec_bf16_rows(_lib.ptr(xs), n, xs.stride(0), d, _lib.ptr(xs16), d, _lib.ptr(mx),
                                                        _lib.stream_ptr(self.device)))
            self._shadow = (xs16, mx)
        return self._shadow

    def resident_tensors(self) -> list:
        return super().resident_tensors() + list(self._shadow or ())

    # -- search ---------------------------------------------------------------------------
    def search(self, xb: torch.Tensor, n: int, q: torch.Tensor, k: int, nprobe: int, out_scores: torch.Tensor,
               out_pos: torch.Tensor, pos_offset: int = 0, elig=None, boost=None, aware: bool = False):
        """``elig``: (require_all, require_any) device int64 [nq] -> every scan of the search is its *_eligible twin over
        ``list_tags`` (same probes, same phases, same tiles; the first phase's tau is the k-th ELIGIBLE score); None: the
        plain scans, nothing else.
        ``boost``: (weights device float32 [nq], boost_max) -> every scan is its *_boosted twin over ``list_boosts`` (same
        probes - chosen by similarity alone -, same phases; the first phase's tau is the k-th BOOSTED score and the prefilter's
        bound is amdrec_ivf_filter_bounds_boosted's); with ``elig`` the *_eligible_boosted twins; None: nothing changes.
        ``aware`` (an index with ``aware_probes``): the probes of a search with ``elig`` and / or ``boost`` are chosen under
        amdrec.probes' rule - the coarse step sees the masks and the weight; everything after the probes is what it was."""
        lib = _lib.load()
        nq = q.shape[0]
        if nq == 0:
            return
        if n == 0:
            out_scores.fill_(float("-inf"))
            out_pos.fill_(-1)
            return
        xs, spos, off, _, max_len, _ = self._build_lists(xb, n)
        etail = (lambda s: ()) if elig is None else self.elig_tail(elig, nq)      # noqa: E731
        btail = (lambda s: ()) if boost is None else self.boost_tail(boost, nq)   # noqa: E731
        tail = lambda s: (*etail(s), *btail(s))                                   # noqa: E731
        sfx = ("" if elig is None else "_eligible") + ("" if boost is None else "_boosted")
        nprobe = search_nprobe(nprobe, self.nlist)
        base = torch.empty((nq, nprobe), dtype=torch.int64, device=self.device)
        n_pool = torch.empty((nq,), dtype=torch.int64, device=self.device)
        pool_ld = self.pool_rows_bound(nprobe)
        chunk = max(1, min(nq, 65535, POOL_BYTES // (pool_ld * 8)))
        grouped = use_grouped_scan(nq, nprobe, self.nlist)
        qtile = QTILE_SPARSE if min(chunk, nq) * nprobe < SPARSE_PAIRS_PER_LIST * self.nlist else QTILE
        if grouped:
            chunk = min(chunk, grouped_chunk_limit(self.nlist, nprobe))
        aware = aware and (elig is not None or boost is not None)
        w = self.workspace(chunk, nprobe, pool_ld, self.aware_table_bytes(nq) if aware else self.coarse_table_bytes(nq, nprobe))
        ws, pair_q, pair_p, goff, qtp = w.pool, w.pair_q, w.pair_p, w.goff, w.qtp
        # 1. coarse quantizer: nprobe best centroids per query (key table in the workspace, or the flat search)
        probes = self.coarse_probes(q, nprobe, w.keys, elig=elig, boost=boost) if aware else self.coarse_probes(q, nprobe, w.keys)
        st = lambda: _lib.stream_ptr(self.device)      # noqa: E731  (per call: check() ends the call's device scope)

        def group_and_scan(s, m, col0, ncol, tau=None, fill=None, n_out=None):
            """(query, probe) pairs of probe columns [col0, col0 + ncol) grouped by list, then the grouped scan of those
            lists: unfiltered into the per-probe slots of the pool, or (tau, fill) filtered and appended."""
            qt = QTILE_SPARSE if m * ncol < SPARSE_PAIRS_PER_LIST * self.nlist else QTILE
            if os.environ.get("AMDREC_IVF_QTILE"):                       # A/B runs: "32", "64", or "first,second" per phase
                f = os.environ["AMDREC_IVF_QTILE"].split(",")
                qt = int(f[0] if (tau is None or len(f) == 1) else f[1])
            # 2. pool layout + (query, probe) pairs grouped by list
            self.group(w, probes[s:, col0:], nprobe, m, ncol, base[s:], n_out, qt)
            if tau is not None and mixed:
                # bf16 prefilter: tau_lo = tau - eps_q, nominate on the bf16 shadow, re-score the nominated rows in fp32
                bounds = (_lib.ptr(q[s:]), m, q.stride(0), self.dim, _lib.ptr(q16[s:]), q16.stride(0), _lib.ptr(mx16), _lib.ptr(tau),
                          tau.stride(0), _lib.ptr(tau_lo[s:]), st())
                if boost is None:
                    _lib.check(lib.amdrec_ivf_filter_bounds(*bounds))
                else:                              # widened for the two roundings of the boosted key (csrc/ivf.hip)
                    _lib.check(lib.amdrec_ivf_filter_bounds_boosted(*bounds, btail(s)[1], _lib.C.c_float(float(boost[1]))))
                _lib.check(getattr(lib, "amdrec_ivf_scan_grouped_mixed" + sfx)(
                    _lib.ptr(xs), xs.stride(0), _lib.ptr(xs16), xs16.stride(0), self.dim, _lib.ptr(spos), _lib.ptr(off),
                    self.nlist, max_len, _lib.ptr(q[s:]), q.stride(0), _lib.ptr(q16[s:]), q16.stride(0), _lib.ptr(goff),
                    _lib.ptr(qtp), (m * ncol) // qt + self.nlist, qt, _lib.ptr(pair_q), _lib.ptr(ws), pool_ld, pos_offset,
                    _lib.ptr(tau), tau.stride(0), _lib.ptr(tau_lo[s:]), _lib.ptr(fill), st(), *tail(s)))
                return
            _lib.check(getattr(lib, "amdrec_ivf_scan_grouped" + sfx)(
                _lib.ptr(xs), xs.stride(0), self.dim, _lib.ptr(spos), _lib.ptr(off), self.nlist, max_len,
                _lib.ptr(q[s:]), q.stride(0), _lib.ptr(goff), _lib.ptr(qtp), (m * ncol) // qt + self.nlist, qt,
                _lib.ptr(pair_q), _lib.ptr(pair_p), _lib.ptr(base[s:]), ncol, _lib.ptr(ws), pool_ld, pos_offset,
                _lib.ptr(tau), 0 if tau is None else tau.stride(0), _lib.ptr(fill), st(), *tail(s)))

        # Exact two-phase scan (batches that take the grouped scan, >= TWO_PHASE_MIN_PROBES probes): the nearest eighth of
        # the probes unfiltered -> select -> tau = that subset's k-th score, a LOWER bound of the final k-th score -> the other
        # probes keep only rows with score >= tau, appended behind the first phase's keys -> the final select.  Same
        # result as one unfiltered scan of every probe; the pool that is written and selected from shrinks several-fold.
        two_phase = grouped and nprobe >= TWO_PHASE_MIN_PROBES
        n_first = first_phase_probes(nprobe)
        mixed = two_phase and self.dim % 8 == 0 and use_mixed_scan(n, self.nlist, nprobe, k)
        if mixed:
            xs16, mx16 = self._list_shadow()
            q16 = torch.empty((nq, self.dim), dtype=torch.bfloat16, device=self.device)
            _lib.check(lib.amdrec_bf16_rows(_lib.ptr(q), nq, q.stride(0), self.dim, _lib.ptr(q16), q16.stride(0), None, st()))
            tau_lo = torch.empty((nq,), dtype=torch.float32, device=self.device)
        scratch_n = torch.empty((chunk,), dtype=torch.int64, device=self.device) if two_phase else None
        for s in range(0, nq, chunk):
            m = min(chunk, nq - s)
            if two_phase:
                group_and_scan(s, m, 0, n_first, n_out=n_pool[s:])
                self.select(ws, pool_ld, n_pool[s:], m, k, out_scores[s:], out_pos[s:])
                group_and_scan(s, m, n_first, nprobe - n_first, tau=out_scores[s:, k - 1], fill=n_pool[s:], n_out=scratch_n)
            elif grouped:
                group_and_scan(s, m, 0, nprobe, n_out=n_pool[s:])
            else:
                self.group(w, probes[s:], nprobe, m, nprobe, base[s:], n_pool[s:], qtile)
                _lib.check(getattr(lib, "amdrec_ivf_scan" + sfx)(
                    _lib.ptr(xs), xs.stride(0), self.dim, _lib.ptr(spos), _lib.ptr(off), _lib.ptr(q[s:]), m, q.stride(0),
                    _lib.ptr(probes[s:]), _lib.ptr(base[s:]), nprobe, _lib.ptr(ws), pool_ld, pos_offset, st(), *tail(s)))
            self.select(ws, pool_ld, n_pool[s:], m, k, out_scores[s:], out_pos[s:])
