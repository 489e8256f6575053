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
from .ivf import (POOL_BYTES, MAX_POINTS_PER_CENTROID, MAX_QUERY_TILES, InvertedLists, _normalize, grouped_chunk_limit,
                  search_nprobe)

KSUB = 256                      # nbits = 8
PQ_NITER = 25                   # faiss ProductQuantizer's default
PQ_SEED = 1234
PQ_MAX_TRAIN = MAX_POINTS_PER_CENTROID * KSUB    # 65 536 sampled residuals
PQ_M = (4, 8, 16, 32)
QTILE = 32                      # queries per amdrec_ivf_group tile (the scan stages 64 KiB of their tables at a time)
TABLE_BYTES = 1 << 30           # distance-table workspace per query chunk


def check_pq_m(dim: int, m: int):
    if m not in PQ_M or dim % m or (dim // m) % 4:
        raise ValueError(f"pq_m must be one of {PQ_M} with dimension % pq_m == 0 and (dimension / pq_m) % 4 == 0 "
                         f"(dimension {dim}, pq_m {m})")


def check_nlist(nlist: int):
    """The search always takes the grouped scan, whose launch needs fewer lists than it has query tiles."""
    if not 1 <= nlist < MAX_QUERY_TILES:
        raise ValueError(f"IVFPQ needs 1 <= nlist < {MAX_QUERY_TILES} (the grouped scan's grid limit), got {nlist}")


class IVFPQState:
    def __init__(self, ivf: InvertedLists, codebooks: torch.Tensor):
        self.ivf = ivf                                              # the coarse level: centroids, assignment, list layout
        self.codebooks = codebooks.contiguous()                     # [m][256][dsub] fp32
        self.m = self.codebooks.shape[0]
        self.nlist, self.dim = ivf.nlist, ivf.dim
        self.device = ivf.device
        self.codes = torch.empty((0, self.m), dtype=torch.uint8, device=self.device)   # insertion order
        self.finite = torch.empty((0,), dtype=torch.bool, device=self.device)          # row has only finite coordinates
        self._nfin = None                                           # finite rows per list (of ivf.lists)

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
    def train(cls, x: torch.Tensor, nlist: int, m: int) -> "IVFPQState":
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
        return cls(ivf, cb)

    def encode(self, x_normalised: torch.Tensor, assign: torch.Tensor) -> torch.Tensor:
        x = x_normalised.contiguous()
        codes = torch.empty((x.shape[0], self.m), dtype=torch.uint8, device=self.device)
        if x.shape[0]:
            c = self.centroids
            _lib.check(_lib.load().amdrec_ivfpq_encode(_lib.ptr(x), x.shape[0], x.stride(0), self.dim, _lib.ptr(assign),
                                                       _lib.ptr(c), c.stride(0), self.nlist, _lib.ptr(self.codebooks),
                                                       self.m, _lib.ptr(codes), _lib.stream_ptr(self.device)))
        return codes

    def encode_rows(self, x_normalised: torch.Tensor):
        """-> (assign, codes, finite) of a batch of L2-normalised rows, not yet part of the index (``commit``)."""
        a = self.ivf.assign_rows(x_normalised)
        return a, self.encode(x_normalised, a), torch.isfinite(x_normalised).all(1)

    def commit(self, batches):
        """Append the (assign, codes, finite) triples of ``encode_rows`` in order."""
        if not batches:
            return
        self.ivf.extend([a for a, _, _ in batches])
        self.codes = torch.cat([self.codes] + [c for _, c, _ in batches])
        self.finite = torch.cat([self.finite] + [f for _, _, f in batches])

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
               pos_offset: int = 0):
        """q: L2-normalised queries.  -> out_dist [nq, k] approximate squared L2 distances (ascending, +inf = unfilled),
        out_pos [nq, k] positions + pos_offset (-1 = unfilled)."""
        lib = _lib.load()
        nq = q.shape[0]
        if nq == 0:
            return
        if self.ntotal == 0:
            out_dist.fill_(float("inf"))
            out_pos.fill_(-1)
            return
        (codes, spos, off, _, max_len, _), nfin = self._build_lists()
        ivf = self.ivf
        nprobe = search_nprobe(nprobe, self.nlist)
        st = lambda: _lib.stream_ptr(self.device)      # noqa: E731  (per call: check() ends the call's device scope)
        base = torch.empty((nq, nprobe), dtype=torch.int64, device=self.device)
        n_pool = torch.empty((nq,), dtype=torch.int64, device=self.device)
        pool_ld = ivf.pool_rows_bound(nprobe)
        chunk = max(1, min(nq, 65535, POOL_BYTES // (pool_ld * 8), TABLE_BYTES // (nprobe * self.m * KSUB * 4),
                           grouped_chunk_limit(self.nlist, nprobe)))
        w = ivf.workspace(chunk, nprobe, pool_ld, ivf.coarse_table_bytes(nq, nprobe),
                          extra_bytes=chunk * nprobe * self.m * KSUB * 4)
        tables = w.extra.view(torch.float32)
        # 1. coarse quantizer: the IVF index's (dense key table + pool select, or the flat search beyond its limits)
        probes = ivf.coarse_probes(q, nprobe, w.keys)
        c = self.centroids
        for s in range(0, nq, chunk):
            m = min(chunk, nq - s)
            # 2. one [m][256] distance table per (query, probe)
            _lib.check(lib.amdrec_ivfpq_tables(_lib.ptr(q[s:]), m, q.stride(0), self.dim, _lib.ptr(probes[s:]), nprobe, nprobe,
                                               _lib.ptr(c), c.stride(0), self.nlist, _lib.ptr(self.codebooks), self.m,
                                               _lib.ptr(tables), st()))
            # 3. pool layout + (query, probe) pairs grouped by list, then the table-lookup scan of every probed list
            ivf.group(w, probes[s:], nprobe, m, nprobe, base[s:], n_pool[s:], QTILE)
            _lib.check(lib.amdrec_ivfpq_scan_finite(_lib.ptr(codes), self.m, _lib.ptr(spos), _lib.ptr(off), _lib.ptr(nfin),
                                                    self.nlist, max_len, _lib.ptr(tables), nprobe, _lib.ptr(w.goff),
                                                    _lib.ptr(w.qtp), (m * nprobe) // QTILE + self.nlist, QTILE,
                                                    _lib.ptr(w.pair_q), _lib.ptr(w.pair_p), _lib.ptr(base[s:]), m * nprobe,
                                                    _lib.ptr(w.pool), pool_ld, pos_offset, st()))
            # 4. the k best keys (score = -distance) -> distances
            ivf.select(w.pool, pool_ld, n_pool[s:], m, k, out_dist[s:], out_pos[s:])
        _lib.check(lib.amdrec_ivfpq_distances(_lib.ptr(out_dist), nq, k, _lib.ptr(out_dist), st()))

    def resident_tensors(self) -> list:
        """Every device tensor kept between calls (a captured graph's kernels point at them)."""
        kept = self.ivf.resident_tensors() + [self.codebooks, self.codes, self.finite]
        return kept if self._nfin is None else kept + [self._nfin]

    # -- persistence ----------------------------------------------------------------------
    def export_arrays(self):
        return self.ivf.export_arrays() + [("pq_codebooks", self.codebooks.cpu().numpy()),
                                           ("pq_codes", self.codes.cpu().numpy()),
                                           ("pq_finite", self.finite.cpu().numpy().astype(np.uint8))]

    @classmethod
    def from_arrays(cls, arrays, device) -> "IVFPQState":
        st = cls(InvertedLists.from_arrays(arrays, device), torch.from_numpy(np.array(arrays["pq_codebooks"])).to(device))
        st.codes = torch.from_numpy(np.array(arrays["pq_codes"])).to(device)
        fin = arrays.get("pq_finite")                               # (absent from files saved before it was kept)
        st.finite = (torch.ones(st.codes.shape[0], dtype=torch.bool) if fin is None
                     else torch.from_numpy(np.array(fin) != 0)).to(device)
        return st
