"""float64 numpy restatement of IVFPQ search (faiss IndexIVFPQ(IndexFlatIP quantizer, d, nlist, m, 8), metric L2,
by_residual, no precomputed tables): the checker for amdrec.ivfpq given an index's own state (centroids, assignment,
codebooks [m][256][dsub], codes [n][m] in insertion order).

* encode: code[r][s] = arg min_j |(x[r] - c[assign[r]])_s - C_s[j]|^2, ties -> lower j
* tables: LUT[s][j] = |(q - c_l)_s - C_s[j]|^2 for one query and one list
* adc_search: the nprobe lists of largest <q, c> (ties -> lower list), then the k rows of those lists with the smallest
  sum_s LUT[s][code_s] (ties -> lower position; a row marked non-finite has distance +inf, after every finite row);
  unfilled slots (+inf, -1)
* table_tol / dist_tol: how far an fp32 table entry / an fp32 sum of m entries may lie from these float64 values
"""
import numpy as np

U = 2.0 ** -24                  # fp32 unit roundoff
ENCODE_CHUNK_ELEMS = 1 << 23    # float64 elements of one broadcast chunk of ``encode`` (64 MiB)


def table_tol(lut64, dsub, rnorm=2.0, c=2.0):
    """Bound of |LUT32 - LUT64| for an entry sum_i (fl(fl(q_i - c_i) - C_i))^2 summed by one fma chain over dsub terms.
    The chain rounds dsub times (dsub * u * LUT); each difference is off by u * (|q_i - c_i| + |t_i|) (t the exact
    difference), which squares to 2 u |t_i| (|q_i - c_i| + |t_i|) per term: 2 u LUT + 2 u sqrt(LUT) |q_s - c_s| by
    Cauchy-Schwarz, with |q_s - c_s| <= rnorm (2 for unit rows and centroids).  A near-zero entry is bounded by the
    cancellation term, not by a relative one."""
    lut64 = np.abs(np.asarray(lut64, dtype=np.float64))
    return c * U * ((dsub + 2) * lut64 + 2 * rnorm * np.sqrt(lut64)) + 1e-30


def dist_tol(d64, d, m, rnorm=2.0, c=2.0):
    """Bound of |D32 - D64| for a distance summed in fp32 over m table entries: the m table bounds (sum_s sqrt(LUT_s) |r_s|
    <= sqrt(D) |r|) plus m roundings of the running sum, loosened to c u ((d + 2m) D + 2 rnorm sqrt(D))."""
    d64 = np.abs(np.asarray(d64, dtype=np.float64))
    return c * U * ((d + 2 * m) * d64 + 2 * rnorm * np.sqrt(d64)) + 1e-30


def encode(x, assign, centroids, codebooks, chunk=None):
    """chunk: rows per broadcast (default: ENCODE_CHUNK_ELEMS float64 of chunk x 256 x dsub)."""
    x = np.asarray(x, dtype=np.float64)
    cb = np.asarray(codebooks, dtype=np.float64)
    m, ksub, dsub = cb.shape
    if chunk is None:
        chunk = max(1, ENCODE_CHUNK_ELEMS // (ksub * dsub))
    res = x - np.asarray(centroids, dtype=np.float64)[np.asarray(assign)]
    codes = np.empty((x.shape[0], m), dtype=np.uint8)
    for s in range(m):
        C = cb[s]
        for r0 in range(0, x.shape[0], chunk):
            rs = res[r0:r0 + chunk, s * dsub:(s + 1) * dsub]
            d2 = ((rs[:, None, :] - C[None, :, :]) ** 2).sum(-1)
            codes[r0:r0 + chunk, s] = np.argmin(d2, axis=1)        # first minimum: lower j
    return codes


def code_distances(x, assign, centroids, codebooks, rows, s, js):
    """|(x[r] - c)_s - C_s[j]|^2 for paired (rows[i], js[i]) in float64."""
    cb = np.asarray(codebooks, dtype=np.float64)
    dsub = cb.shape[2]
    x = np.asarray(x, dtype=np.float64)[rows]
    res = x - np.asarray(centroids, dtype=np.float64)[np.asarray(assign)[rows]]
    return ((res[:, s * dsub:(s + 1) * dsub] - cb[s][js]) ** 2).sum(-1)


def tables(q, centroid, codebooks):
    cb = np.asarray(codebooks, dtype=np.float64)
    m, ksub, dsub = cb.shape
    r = (np.asarray(q, dtype=np.float64) - np.asarray(centroid, dtype=np.float64)).reshape(m, 1, dsub)
    return ((r - cb) ** 2).sum(-1)                                  # [m][256]


def coarse_probes(centroids, xq, nprobe):
    s = np.asarray(xq, dtype=np.float64) @ np.asarray(centroids, dtype=np.float64).T
    order = np.argsort(-s, axis=1, kind="stable")
    return order[:, :nprobe]


def adc_search(codes, assign, centroids, codebooks, xq, k, nprobe, probes=None, finite=None):
    """finite: bool [n] (None: every row finite); a non-finite row's distance is +inf."""
    codes = np.asarray(codes)
    assign = np.asarray(assign)
    xq = np.asarray(xq)
    if probes is None:
        probes = coarse_probes(centroids, xq, nprobe)
    m = codes.shape[1]
    nq = xq.shape[0]
    D = np.full((nq, k), np.inf)
    I = np.full((nq, k), -1, dtype=np.int64)
    cols = np.arange(m)
    for q in range(nq):
        pos_all, d_all = [], []
        for l in probes[q][:nprobe]:
            if l < 0:
                continue
            rows = np.nonzero(assign == l)[0]
            if rows.size == 0:
                continue
            lut = tables(xq[q], centroids[l], codebooks)
            dl = lut[cols[None, :], codes[rows].astype(np.int64)].sum(1)
            if finite is not None:
                dl = np.where(np.asarray(finite)[rows], dl, np.inf)
            d_all.append(dl)
            pos_all.append(rows)
        if not pos_all:
            continue
        pos, d = np.concatenate(pos_all), np.concatenate(d_all)
        order = np.lexsort((pos, d))[:k]
        D[q, :order.size] = d[order]
        I[q, :order.size] = pos[order]
    return D, I
