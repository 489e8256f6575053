"""IVFPQ state for ``FAISSIndex(index_type='IVFPQ')`` (faiss_retrieval.py:56-63: ``faiss.IndexIVFPQ(quantizer, d, nlist,
8, 8)`` with an IndexFlatIP quantizer and no metric argument): the coarse level is exactly the IVF index's (same trainer,
sample, seed and max-inner-product assignment / probes), the fine level is a product quantizer of the residuals
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
from .ivf import (POOL_BYTES, MAX_POINTS_PER_CENTROID, MAX_QUERY_TILES, IVFState, _assign, _normalize,
                  grouped_chunk_limit, search_nprobe)

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
    def __init__(self, ivf: IVFState, codebooks: torch.Tensor):
        self.ivf = ivf                                              # coarse centroids + per-row list assignment
        self.codebooks = codebooks.contiguous()                     # [m][256][dsub] fp32
        self.m = self.codebooks.shape[0]
        self.nlist, self.dim = ivf.nlist, ivf.dim
        self.device = ivf.device
        self.codes = torch.empty((0, self.m), dtype=torch.uint8, device=self.device)   # insertion order
        self.finite = torch.empty((0,), dtype=torch.bool, device=self.device)          # row has only finite coordinates
        self._lists = None          # (codes list-contiguous, spos, list_off, list_len, max_len, n, finite rows per list)

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
        ivf = IVFState.train(x, nlist)                              # the IVF index's quantizer, bit for bit
        xn = _normalize(x.float())
        g = torch.Generator(device="cpu")
        g.manual_seed(PQ_SEED)
        if n > PQ_MAX_TRAIN:
            xn = xn[torch.randperm(n, generator=g)[:PQ_MAX_TRAIN].to(x.device)]
            n = xn.shape[0]
        xn = xn.contiguous()
        a = _assign(xn, ivf.centroids)
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
        a = _assign(x_normalised, self.centroids)
        return a, self.encode(x_normalised, a), torch.isfinite(x_normalised).all(1)

    def commit(self, batches):
        """Append the (assign, codes, finite) triples of ``encode_rows`` in order."""
        if not batches:
            return
        self.ivf.assign = torch.cat([self.ivf.assign] + [a for a, _, _ in batches])
        self.codes = torch.cat([self.codes] + [c for _, c, _ in batches])
        self.finite = torch.cat([self.finite] + [f for _, _, f in batches])
        self._lists = None

    def append(self, x_normalised: torch.Tensor):
        """Assign and encode a batch of L2-normalised rows (their fp32 values are not kept)."""
        self.commit([self.encode_rows(x_normalised)])

    def _build_lists(self):
        n = self.ntotal
        if self._lists is None or self._lists[5] != n:
            a, fin = self.assign[:n], self.finite[:n]
            # rows of a list keep insertion order, its non-finite rows after its finite ones
            order = torch.argsort(a * 2 + (~fin).to(torch.int64), stable=True)
            counts = torch.bincount(a, minlength=self.nlist)
            nfin = torch.bincount(a[fin], minlength=self.nlist).to(torch.int64)
            off = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)
            off[1:] = torch.cumsum(counts, 0)
            self._lists = (self.codes[order].contiguous(), order.contiguous(), off, counts.to(torch.int64),
                           int(counts.max().item()) if n else 0, n, nfin)
            self.ivf._top_rows = np.cumsum(np.sort(counts.cpu().numpy())[::-1].astype(np.int64))
        return self._lists

    # -- search ---------------------------------------------------------------------------
    def _coarse(self, q, nprobe, cs, probes, keys):
        """The nprobe best lists per query by inner product, as the IVF index picks them: a dense (score, centroid) key
        table in ``keys`` + the pool select, or (keys None: beyond the table's limits) the flat search."""
        from .index import flat_search
        lib, ivf, nq = _lib.load(), self.ivf, q.shape[0]
        if keys is None:
            flat_search(self.centroids, self.nlist, q, nprobe, cs, probes)
            return
        if ivf._nlist_count is None or ivf._nlist_count.numel() < nq:
            ivf._nlist_count = torch.full((max(nq, 512),), self.nlist, dtype=torch.int64, device=self.device)
        c = self.centroids
        coarse_ld = (self.nlist + 1) // 2 * 2
        _lib.check(lib.amdrec_ivf_coarse_keys(_lib.ptr(c), self.nlist, c.stride(0), self.dim, _lib.ptr(q), nq, q.stride(0),
                                              _lib.ptr(keys), coarse_ld, _lib.stream_ptr(self.device)))
        _lib.check(lib.amdrec_ivf_select(_lib.ptr(keys), coarse_ld, _lib.ptr(ivf._nlist_count), nq, nprobe, _lib.ptr(cs),
                                         _lib.ptr(probes), _lib.stream_ptr(self.device)))

    def coarse_probes(self, q: torch.Tensor, nprobe: int) -> torch.Tensor:
        """The lists ``search`` probes for the L2-normalised queries q: int64 [nq, nprobe] (-1 = none)."""
        nq = q.shape[0]
        cs = torch.empty((nq, nprobe), dtype=torch.float32, device=self.device)
        probes = torch.empty((nq, nprobe), dtype=torch.int64, device=self.device)
        coarse_ld = (self.nlist + 1) // 2 * 2
        if nq and nq * coarse_ld * 8 <= POOL_BYTES and nprobe <= _lib.MAX_K and nq < (1 << 24):
            self._coarse(q, nprobe, cs, probes, _lib.WORKSPACE.get(nq * coarse_ld * 8, self.device))
        elif nq:
            self._coarse(q, nprobe, cs, probes, None)
        return probes

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
        codes, spos, off, lens, max_len, _, nfin = self._build_lists()
        ivf = self.ivf
        nprobe = search_nprobe(nprobe, self.nlist)
        st = lambda: _lib.stream_ptr(self.device)      # noqa: E731  (per call: check() ends the call's device scope)
        # 1. coarse quantizer: the IVF index's (dense key table + pool select, or the flat search beyond its limits)
        cs = torch.empty((nq, nprobe), dtype=torch.float32, device=self.device)
        probes = torch.empty((nq, nprobe), dtype=torch.int64, device=self.device)
        base = torch.empty((nq, nprobe), dtype=torch.int64, device=self.device)
        n_pool = torch.empty((nq,), dtype=torch.int64, device=self.device)
        pool_ld = ivf.pool_rows_bound(nprobe)
        chunk = max(1, min(nq, 65535, POOL_BYTES // (pool_ld * 8), TABLE_BYTES // (nprobe * self.m * KSUB * 4),
                           grouped_chunk_limit(self.nlist, nprobe)))
        pool_bytes = (chunk * pool_ld * 8 + 255) // 256 * 256
        grp_bytes = ((self.nlist + 1) * 4 + 255) // 256 * 256 + (chunk * nprobe * 4 + 255) // 256 * 256
        arr_bytes = (2 * chunk * nprobe * 8 + 2 * (self.nlist + 1) * 8 + 255) // 256 * 256
        tab_bytes = chunk * nprobe * self.m * KSUB * 4
        coarse_ld = (self.nlist + 1) // 2 * 2
        coarse = nq * coarse_ld * 8 <= POOL_BYTES and nprobe <= _lib.MAX_K and nq < (1 << 24)
        wsall = _lib.WORKSPACE.get(max(pool_bytes + grp_bytes + arr_bytes + tab_bytes + 256,
                                       nq * coarse_ld * 8 if coarse else 0), self.device)
        self._coarse(q, nprobe, cs, probes, wsall if coarse else None)
        ws = wsall[:pool_bytes]
        grp = wsall[pool_bytes:pool_bytes + grp_bytes]
        a0 = pool_bytes + grp_bytes
        arr = wsall[a0:a0 + arr_bytes].view(torch.int64)
        tables = wsall[a0 + arr_bytes:a0 + arr_bytes + tab_bytes].view(torch.float32)
        pair_q, pair_p = arr[:chunk * nprobe], arr[chunk * nprobe:2 * chunk * nprobe]
        goff = arr[2 * chunk * nprobe:2 * chunk * nprobe + self.nlist + 1]
        qtp = arr[2 * chunk * nprobe + self.nlist + 1:2 * chunk * nprobe + 2 * (self.nlist + 1)]
        c = self.centroids
        for s in range(0, nq, chunk):
            m = min(chunk, nq - s)
            # 2. one [m][256] distance table per (query, probe)
            _lib.check(lib.amdrec_ivfpq_tables(_lib.ptr(q[s:]), m, q.stride(0), self.dim, _lib.ptr(probes[s:]), nprobe, nprobe,
                                               _lib.ptr(c), c.stride(0), self.nlist, _lib.ptr(self.codebooks), self.m,
                                               _lib.ptr(tables), st()))
            # 3. pool layout + (query, probe) pairs grouped by list, then the table-lookup scan of every probed list
            _lib.check(lib.amdrec_ivf_group(_lib.ptr(probes[s:]), nprobe, m, nprobe, self.nlist, _lib.ptr(lens),
                                            _lib.ptr(base[s:]), _lib.ptr(n_pool[s:]), _lib.ptr(pair_q), _lib.ptr(pair_p),
                                            _lib.ptr(goff), _lib.ptr(qtp), QTILE, _lib.ptr(grp), grp.numel(), st()))
            _lib.check(lib.amdrec_ivfpq_scan_finite(_lib.ptr(codes), self.m, _lib.ptr(spos), _lib.ptr(off), _lib.ptr(nfin),
                                                    self.nlist, max_len, _lib.ptr(tables), nprobe, _lib.ptr(goff),
                                                    _lib.ptr(qtp), (m * nprobe) // QTILE + self.nlist, QTILE, _lib.ptr(pair_q),
                                                    _lib.ptr(pair_p), _lib.ptr(base[s:]), m * nprobe, _lib.ptr(ws), pool_ld,
                                                    pos_offset, st()))
            # 4. the k best keys (score = -distance) -> distances
            ivf._select(lib, ws, pool_ld, n_pool[s:], m, k, out_dist[s:], out_pos[s:], st())
        _lib.check(lib.amdrec_ivfpq_distances(_lib.ptr(out_dist), nq, k, _lib.ptr(out_dist), st()))

    # -- persistence ----------------------------------------------------------------------
    def export_arrays(self):
        return [("ivf_centroids", self.centroids.cpu().numpy()), ("ivf_assign", self.assign.cpu().numpy()),
                ("pq_codebooks", self.codebooks.cpu().numpy()), ("pq_codes", self.codes.cpu().numpy()),
                ("pq_finite", self.finite.cpu().numpy().astype(np.uint8))]

    @classmethod
    def from_arrays(cls, arrays, device) -> "IVFPQState":
        st = cls(IVFState.from_arrays(arrays, device), torch.from_numpy(np.array(arrays["pq_codebooks"])).to(device))
        st.codes = torch.from_numpy(np.array(arrays["pq_codes"])).to(device)
        fin = arrays.get("pq_finite")                               # (absent from files saved before it was kept)
        st.finite = (torch.ones(st.codes.shape[0], dtype=torch.bool) if fin is None
                     else torch.from_numpy(np.array(fin) != 0)).to(device)
        return st
