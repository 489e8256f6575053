"""IVFPQ state for ``FAISSIndex(index_type='IVFPQ')`` (faiss_retrieval.py:56-63: ``faiss.IndexIVFPQ(quantizer, d, nlist,
8, 8)`` with an IndexFlatIP quantizer and no metric argument): the coarse level is the IVF index's (an
``amdrec.ivf.InvertedLists``: same trainer, sample, seed, max-inner-product assignment / probes, list layout, scan
workspace, grouping and pool select), the fine level is a product quantizer of the residuals
x - c[assign(x)] under faiss's default metric, L2 (by_residual, m sub-spaces of 256 codewords, 8-bit codes).  The index
keeps m bytes of codes per row and no fp32 corpus.

Build and search are hand-written HIP (csrc/ivfpq.hip): PQ training = ``amdrec_ivfpq_train_step`` x PQ_NITER (L2 Lloyd with
order-independent fixed-point sums: bit-reproducible), encoding = ``amdrec_ivfpq_encode`` (tiled GEMM with an arg-min
epilogue), search = coarse probes (``amdrec_ivf_coarse_keys`` + ``amdrec_ivf_select``, as IVF) -> ``amdrec_ivfpq_tables``
(one [m][256] distance table per (query, probed list), as faiss builds them for an IP quantizer) -> ``amdrec_ivf_group`` ->
``amdrec_ivfpq_scan_finite`` (table lookups, keys with score = -distance) -> ``amdrec_ivf_select`` ->
``amdrec_ivfpq_distances``.
Refine (opt-in, ``refine='fp32'`` / ``'bf16'``): the index also keeps every L2-normalised row (insertion order: the candidates
arrive as corpus positions); a search for k takes k' = min(k x refine_factor, AMDREC_MAX_K) candidates from the steps above
and ``amdrec_ivfpq_rerank`` orders them by their exact squared L2 distance to the kept row and returns the best k (faiss's
IndexRefineFlat over IndexIVFPQ).  With a bf16 copy the distance is to the bf16-rounded row, widened to fp32.
A search call launches only libamdrec kernels and never synchronises with the host: it can be captured in a HIP graph.
What stays in torch is build-time plumbing: drawing the training sample, gathering the initial codewords and the one stable
sort that lays the codes out list-contiguously (a list's rows with a non-finite coordinate last: the scan gives them -inf
keys, so they rank after every finite row, as IVF-Flat's NaN scores do).
Deviation from faiss: an empty cluster keeps its codeword (faiss splits a large cluster instead).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .rows_edit import gather_rows
from .ivf import (POOL_BYTES, MAX_POINTS_PER_CENTROID, MAX_QUERY_TILES, InvertedLists, _normalize, grouped_chunk_limit,
                  search_nprobe)

KSUB = 256                      # nbits = 8
PQ_NITER = 25                   # faiss ProductQuantizer's default
PQ_SEED = 1234
PQ_MAX_TRAIN = MAX_POINTS_PER_CENTROID * KSUB    # 65 536 sampled residuals
PQ_M = (4, 8, 16, 32)
QTILE = 32                      # queries per amdrec_ivf_group tile (the scan stages 64 KiB of their tables at a time)
TABLE_BYTES = 1 << 30           # distance-table workspace per query chunk
REFINE_KINDS = (None, "fp32", "bf16")
RERANK_MAX_QUERIES = 65535      # queries per amdrec_ivfpq_rerank launch
RERANK_SPLIT_MAX_QUERIES = 512  # up to here the kernel may split a query over workgroups (csrc/ivfpq_refine.hip rerank_slices:
                                # at most ~1024 workgroups, at least two per query) and wants scratch and tickets; the library
                                # takes one workgroup per query whenever it is given none


def check_pq_m(dim: int, m: int):
    if m not in PQ_M or dim % m or (dim // m) % 4:
        raise ValueError(f"pq_m must be one of {PQ_M} with dimension % pq_m == 0 and (dimension / pq_m) % 4 == 0 "
                         f"(dimension {dim}, pq_m {m})")


def check_refine(index_type: str, dim: int, refine, refine_factor):
    """The refine arguments of FAISSIndex: checked before the library is loaded."""
    if refine not in REFINE_KINDS:
        raise ValueError(f"refine must be None, 'fp32' or 'bf16', got {refine!r}")
    if refine is not None and index_type != "IVFPQ":
        raise ValueError(f"refine is an IVFPQ option (a {index_type} index already returns exact scores)")
    if refine == "bf16" and dim % 8:
        raise ValueError(f"refine='bf16' needs a dimension that is a multiple of 8 (the bf16 row kernels), got {dim}")
    if isinstance(refine_factor, bool) or not isinstance(refine_factor, (int, np.integer)) or refine_factor < 1:
        raise ValueError(f"refine_factor must be an integer >= 1, got {refine_factor!r}")


def refine_candidates(k: int, refine_factor: int) -> int:
    """Candidates the code scan hands to the re-rank of a search for k: k x factor, silently clamped to AMDREC_MAX_K (the
    select's and the sort's limit; k itself is within it, so the result is never below k)."""
    return min(k * int(refine_factor), _lib.MAX_K)


def check_nlist(nlist: int):
    """The search always takes the grouped scan, whose launch needs fewer lists than it has query tiles."""
    if not 1 <= nlist < MAX_QUERY_TILES:
        raise ValueError(f"IVFPQ needs 1 <= nlist < {MAX_QUERY_TILES} (the grouped scan's grid limit), got {nlist}")


class IVFPQState:
    def __init__(self, ivf: InvertedLists, codebooks: torch.Tensor, refine=None, refine_factor: int = 4):
        self.ivf = ivf                                              # the coarse level: centroids, assignment, list layout
        self.codebooks = codebooks.contiguous()                     # [m][256][dsub] fp32
        self.m = self.codebooks.shape[0]
        self.nlist, self.dim = ivf.nlist, ivf.dim
        self.device = ivf.device
        self.codes = torch.empty((0, self.m), dtype=torch.uint8, device=self.device)   # insertion order
        self.finite = torch.empty((0,), dtype=torch.bool, device=self.device)          # row has only finite coordinates
        self._nfin = None                                           # finite rows per list (of ivf.lists)
        self.refine, self.refine_factor = refine, int(refine_factor)
        # refine: every L2-normalised row, insertion order, fp32 or bf16 (round to nearest); None: codes only
        self.rows = None if refine is None else torch.empty(
            (0, self.dim), dtype=torch.float32 if refine == "fp32" else torch.bfloat16, device=self.device)
        self._rr_scratch = None                                     # amdrec_ivfpq_rerank's key slots and tickets (small batches)
        self._rr_tickets = None

    @property
    def centroids(self):
        return self.ivf.centroids

    @property
    def assign(self):
        return self.ivf.assign

    @property
    def ntotal(self) -> int:
        return self.codes.shape[0]

    # -- build ----------------------------------------------------------------------------
    @classmethod
    def train(cls, x: torch.Tensor, nlist: int, m: int, refine=None, refine_factor: int = 4) -> "IVFPQState":
        """x: fp32 device copy of the training embeddings (un-normalised, as FAISSIndex.add passes them to train())."""
        n, d = x.shape
        check_pq_m(d, m)
        if n < KSUB:
            raise ValueError(f"IVFPQ training needs at least {KSUB} vectors (one per codeword), got {n}")
        ivf = InvertedLists.train(x, nlist)                         # the IVF index's quantizer, bit for bit
        xn = _normalize(x.float())
        g = torch.Generator(device="cpu")
        g.manual_seed(PQ_SEED)
        if n > PQ_MAX_TRAIN:
            xn = xn[torch.randperm(n, generator=g)[:PQ_MAX_TRAIN].to(x.device)]
            n = xn.shape[0]
        xn = xn.contiguous()
        a = ivf.assign_rows(xn)
        init = torch.randperm(n, generator=g)[:KSUB].to(x.device)  # distinct sample rows
        res0 = xn[init] - ivf.centroids[a[init]]
        cb = res0.view(KSUB, m, d // m).permute(1, 0, 2).contiguous()
        lib = _lib.load()
        nbytes = _lib.C.c_size_t(0)
        _lib.check(lib.amdrec_ivfpq_train_workspace(n, d, m, _lib.C.byref(nbytes)))
        ws = _lib.WORKSPACE.get(nbytes.value, x.device)
        for _ in range(PQ_NITER):
            _lib.check(lib.amdrec_ivfpq_train_step(_lib.ptr(xn), n, xn.stride(0), d, _lib.ptr(a), _lib.ptr(ivf.centroids),
                                                   ivf.centroids.stride(0), nlist, _lib.ptr(cb), m, _lib.ptr(ws), ws.numel(),
                                                   _lib.stream_ptr(x.device)))
        return cls(ivf, cb, refine, refine_factor)

    def encode(self, x_normalised: torch.Tensor, assign: torch.Tensor) -> torch.Tensor:
        x = x_normalised.contiguous()
        codes = torch.empty((x.shape[0], self.m), dtype=torch.uint8, device=self.device)
        if x.shape[0]:
            c = self.centroids
            _lib.check(_lib.load().amdrec_ivfpq_encode(_lib.ptr(x), x.shape[0], x.stride(0), self.dim, _lib.ptr(assign),
                                                       _lib.ptr(c), c.stride(0), self.nlist, _lib.ptr(self.codebooks),
                                                       self.m, _lib.ptr(codes), _lib.stream_ptr(self.device)))
        return codes

    def keep_rows(self, x_normalised: torch.Tensor):
        """The kept form of a batch of L2-normalised rows: None (no refine), the fp32 rows themselves, or their bf16
        (round to nearest) copy made by amdrec_bf16_rows."""
        if self.refine is None:
            return None
        x = x_normalised.contiguous()
        if self.refine == "fp32":
            return x
        y = torch.empty(x.shape, dtype=torch.bfloat16, device=self.device)
        if x.shape[0]:
            _lib.check(_lib.load().amdrec_bf16_rows(_lib.ptr(x), x.shape[0], x.stride(0), self.dim, _lib.ptr(y), y.stride(0),
                                                    None, _lib.stream_ptr(self.device)))
        return y

    def encode_rows(self, x_normalised: torch.Tensor):
        """-> (assign, codes, finite, kept rows or None) of a batch of L2-normalised rows, not yet part of the index
        (``commit``)."""
        a = self.ivf.assign_rows(x_normalised)
        return a, self.encode(x_normalised, a), torch.isfinite(x_normalised).all(1), self.keep_rows(x_normalised)

    def commit(self, batches):
        """Append the (assign, codes, finite, kept rows) batches of ``encode_rows`` in order."""
        if not batches:
            return
        self.ivf.extend([b[0] for b in batches])
        self.codes = torch.cat([self.codes] + [b[1] for b in batches])
        self.finite = torch.cat([self.finite] + [b[2] for b in batches])
        if self.rows is not None:                           # (as the codes: an O(n) copy and, for its duration, twice the bytes)
            self.rows = torch.cat([self.rows] + [b[3] for b in batches])

    def compact(self, kept: torch.Tensor):
        """Rows were removed (FAISSIndex.remove_ids): the assignment, the codes, the finite flags and, with refine, the kept
        rows of the rows in ``kept`` (old positions, ascending), each gathered into a NEW tensor; the list layout is dropped.
        Centroids and codebooks stay: nothing is re-assigned or re-encoded."""
        self.ivf.compact(kept)
        self.codes = gather_rows(self.codes, kept)
        self.finite = gather_rows(self.finite, kept)
        if self.rows is not None:
            self.rows = gather_rows(self.rows, kept)
        self._nfin = None

    def _build_lists(self):
        """-> (the layout: codes list-contiguous, a list's non-finite rows after its finite ones; finite rows per list)."""
        n, ivf = self.ntotal, self.ivf
        if ivf.lists is None or ivf.lists.n != n:
            ivf.layout(n, self.codes, last=~self.finite)
            self._nfin = torch.bincount(self.assign[:n][self.finite[:n]], minlength=self.nlist).to(torch.int64)
        return ivf.lists, self._nfin

    # -- search ---------------------------------------------------------------------------
    def coarse_probes(self, q: torch.Tensor, nprobe: int) -> torch.Tensor:
        """The lists ``search`` probes for the L2-normalised queries q: int64 [nq, nprobe] (-1 = none)."""
        return self.ivf.coarse_probes(q, nprobe)

    def search(self, q: torch.Tensor, k: int, nprobe: int, out_dist: torch.Tensor, out_pos: torch.Tensor,
               pos_offset: int = 0, elig=None, aware: bool = False):
        """``elig``: (require_all, require_any) device int64 [nq] -> the code scan is amdrec_ivfpq_scan_finite_eligible over the
        coarse level's ``list_tags``; with refine the re-rank then orders the best ELIGIBLE candidates and needs no masks.
        ``aware`` (an index with ``aware_probes``): the probes of a masked search are the best FEASIBLE lists (amdrec.probes).
        q: L2-normalised queries.  -> out_dist [nq, k] squared L2 distances (ascending, +inf = unfilled): approximate
        (from the codes), or with refine exact for the kept rows; out_pos [nq, k] positions + pos_offset (-1 = unfilled)."""
        nq = q.shape[0]
        if nq == 0:
            return
        if self.ntotal == 0:
            out_dist.fill_(float("inf"))
            out_pos.fill_(-1)
            return
        if self.rows is None:
            self._search_codes(q, k, nprobe, out_dist, out_pos, pos_offset, elig=elig, aware=aware)
            return
        # steps 1-4 for k' candidates (scores = -approximate distance: only their order matters), then
        # 5. the exact re-rank of those candidates from the kept rows
        kc = refine_candidates(k, self.refine_factor)
        cand_score = torch.empty((nq, kc), dtype=torch.float32, device=self.device)
        cand_pos = torch.empty((nq, kc), dtype=torch.int64, device=self.device)
        self._search_codes(q, kc, nprobe, cand_score, cand_pos, 0, distances=False, elig=elig, aware=aware)
        self.rerank(q, cand_pos, k, out_dist, out_pos, pos_offset)

    def rerank(self, q: torch.Tensor, cand_pos: torch.Tensor, k: int, out_dist: torch.Tensor, out_pos: torch.Tensor,
               pos_offset: int = 0):
        """amdrec_ivfpq_rerank: the k best of each query's candidates (corpus positions, -1 = unfilled) by exact distance to
        the kept rows."""
        lib = _lib.load()
        nq, kc = cand_pos.shape
        rows, n = self.rows, self.ntotal
        if self._rr_tickets is None:                        # the kernel leaves them zero
            self._rr_tickets = torch.zeros(RERANK_SPLIT_MAX_QUERIES, dtype=torch.int32, device=self.device)
        split = nq <= RERANK_SPLIT_MAX_QUERIES              # (beyond: one workgroup per query, no scratch needed)
        need = nq * kc * 8 if split else 0
        if need and (self._rr_scratch is None or self._rr_scratch.numel() < need):
            self._rr_scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        for s in range(0, nq, RERANK_MAX_QUERIES):
            m = min(RERANK_MAX_QUERIES, nq - s)
            _lib.check(lib.amdrec_ivfpq_rerank(
                _lib.ptr(rows), int(self.refine == "bf16"), n, rows.stride(0), self.dim, _lib.ptr(self.finite),
                _lib.ptr(q[s:]), m, q.stride(0), _lib.ptr(cand_pos[s:]), kc, pos_offset, k, _lib.ptr(out_dist[s:]),
                _lib.ptr(out_pos[s:]), _lib.ptr(self._rr_scratch) if split else None, need,
                _lib.ptr(self._rr_tickets) if split else None, _lib.stream_ptr(self.device)))

    def _search_codes(self, q: torch.Tensor, k: int, nprobe: int, out_dist: torch.Tensor, out_pos: torch.Tensor,
                      pos_offset: int = 0, distances: bool = True, elig=None, aware: bool = False):
        """Steps 1-4: the k best rows of the probed lists by the codes' table-lookup distance (``distances`` False: out_dist
        keeps the select's scores, -distance)."""
        lib = _lib.load()
        nq = q.shape[0]
        (codes, spos, off, _, max_len, _), nfin = self._build_lists()
        ivf = self.ivf
        tail = (lambda s: ()) if elig is None else ivf.elig_tail(elig, nq)      # noqa: E731
        scan = lib.amdrec_ivfpq_scan_finite if elig is None else lib.amdrec_ivfpq_scan_finite_eligible
        nprobe = search_nprobe(nprobe, self.nlist)
        st = lambda: _lib.stream_ptr(self.device)      # noqa: E731  (per call: check() ends the call's device scope)
        base = torch.empty((nq, nprobe), dtype=torch.int64, device=self.device)
        n_pool = torch.empty((nq,), dtype=torch.int64, device=self.device)
        pool_ld = ivf.pool_rows_bound(nprobe)
        chunk = max(1, min(nq, 65535, POOL_BYTES // (pool_ld * 8), TABLE_BYTES // (nprobe * self.m * KSUB * 4),
                           grouped_chunk_limit(self.nlist, nprobe)))
        aware = aware and elig is not None
        w = ivf.workspace(chunk, nprobe, pool_ld, ivf.aware_table_bytes(nq) if aware else ivf.coarse_table_bytes(nq, nprobe),
                          extra_bytes=chunk * nprobe * self.m * KSUB * 4)
        tables = w.extra.view(torch.float32)
        # 1. coarse quantizer: the IVF index's (dense key table + pool select, or the flat search beyond its limits)
        probes = ivf.coarse_probes(q, nprobe, w.keys, elig=elig) if aware else ivf.coarse_probes(q, nprobe, w.keys)
        c = self.centroids
        for s in range(0, nq, chunk):
            m = min(chunk, nq - s)
            # 2. one [m][256] distance table per (query, probe)
            _lib.check(lib.amdrec_ivfpq_tables(_lib.ptr(q[s:]), m, q.stride(0), self.dim, _lib.ptr(probes[s:]), nprobe, nprobe,
                                               _lib.ptr(c), c.stride(0), self.nlist, _lib.ptr(self.codebooks), self.m,
                                               _lib.ptr(tables), st()))
            # 3. pool layout + (query, probe) pairs grouped by list, then the table-lookup scan of every probed list
            ivf.group(w, probes[s:], nprobe, m, nprobe, base[s:], n_pool[s:], QTILE)
            _lib.check(scan(_lib.ptr(codes), self.m, _lib.ptr(spos), _lib.ptr(off), _lib.ptr(nfin),
                            self.nlist, max_len, _lib.ptr(tables), nprobe, _lib.ptr(w.goff),
                            _lib.ptr(w.qtp), (m * nprobe) // QTILE + self.nlist, QTILE,
                            _lib.ptr(w.pair_q), _lib.ptr(w.pair_p), _lib.ptr(base[s:]), m * nprobe,
                            _lib.ptr(w.pool), pool_ld, pos_offset, st(), *tail(s)))
            # 4. the k best keys (score = -distance) -> distances
            ivf.select(w.pool, pool_ld, n_pool[s:], m, k, out_dist[s:], out_pos[s:])
        if distances:
            _lib.check(lib.amdrec_ivfpq_distances(_lib.ptr(out_dist), nq, k, _lib.ptr(out_dist), st()))

    def resident_tensors(self) -> list:
        """Every device tensor kept between calls (a captured graph's kernels point at them)."""
        kept = self.ivf.resident_tensors() + [self.codebooks, self.codes, self.finite, self._nfin, self.rows,
                                              self._rr_scratch, self._rr_tickets]
        return [t for t in kept if t is not None]

    # -- persistence ----------------------------------------------------------------------
    def export_arrays(self):
        out = self.ivf.export_arrays() + [("pq_codebooks", self.codebooks.cpu().numpy()),
                                          ("pq_codes", self.codes.cpu().numpy()),
                                          ("pq_finite", self.finite.cpu().numpy().astype(np.uint8))]
        if self.refine == "fp32":
            out.append(("pq_rows", self.rows.cpu().numpy()))
        elif self.refine == "bf16":                                 # numpy has no bf16: the bit patterns
            out.append(("pq_rows", self.rows.view(torch.int16).cpu().numpy().view(np.uint16)))
        return out

    @classmethod
    def from_arrays(cls, arrays, device, refine=None, refine_factor: int = 4) -> "IVFPQState":
        st = cls(InvertedLists.from_arrays(arrays, device), torch.from_numpy(np.array(arrays["pq_codebooks"])).to(device),
                 refine, refine_factor)
        if refine is not None:
            rows = np.array(arrays["pq_rows"])
            st.rows = (torch.from_numpy(rows).to(device) if refine == "fp32"
                       else torch.from_numpy(rows.view(np.int16)).to(device).view(torch.bfloat16)).contiguous()
        st.codes = torch.from_numpy(np.array(arrays["pq_codes"])).to(device)
        fin = arrays.get("pq_finite")                               # (absent from files saved before it was kept)
        st.finite = (torch.ones(st.codes.shape[0], dtype=torch.bool) if fin is None
                     else torch.from_numpy(np.array(fin) != 0)).to(device)
        return st
