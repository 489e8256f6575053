"""IVFPQ refine without a GPU: amdrec_ivfpq_rerank refuses bad arguments before anything is launched, FAISSIndex checks
``refine`` / ``refine_factor`` before the library is loaded, the float64 oracle of the stage (tests/ivfpq_refine_oracle.py)
equals a brute-force restatement, and the property the stage exists for: re-ranking k x factor candidates of the code scan
never lowers recall@k, and more candidates never lower it either."""
import ctypes as C

import numpy as np
import pytest

from tests import ivfpq_oracle
from tests import ivfpq_refine_oracle as ro


def _clustered(n, d, n_clusters, seed, spread=0.35):         # the generator of tests/test_ivfpq_gpu.py
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n_clusters, d)).astype(np.float32)
    x = c[rng.integers(0, n_clusters, n)] + spread * rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_rerank_entry_validates_arguments_without_a_gpu():
    from amdrec import _lib as L
    lib = L.load()
    assert lib.amdrec_abi_version() == 14 and L.ABI_VERSION == 14
    buf = C.create_string_buffer(64)
    p = C.cast(C.addressof(buf) + (-C.addressof(buf)) % 16, C.c_void_p)   # any 16-byte aligned address: nothing launches

    def call(rows=p, bf16=0, nrows=100, ld=256, dim=256, fin=None, q=p, nq=4, ldq=256, cand=p, kc=40, off=0, k=10, od=p,
             op=p, ws=None, wsb=0, tk=None):
        return lib.amdrec_ivfpq_rerank(rows, bf16, nrows, ld, dim, fin, q, nq, ldq, cand, kc, off, k, od, op, ws, wsb, tk, None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        assert word in lib.amdrec_last_error(), (kw, lib.amdrec_last_error())

    assert call(nq=0) == 0                                     # nothing to do
    assert call(nq=0, rows=None, q=None, cand=None, od=None, op=None) == 0
    refused(b"k=0", k=0)
    refused(b"k=41", k=41)                                     # k <= kc
    refused(b"kc=0", kc=0, k=1)
    refused(b"kc=2049", kc=2049)
    refused(b"k=2049", kc=2048, k=2049)
    refused(b"dim=250", dim=250, ld=252)
    refused(b"dim=260", dim=260, ld=260, ldq=260, bf16=1)      # bf16 rows: a multiple of 8
    assert call(dim=260, ld=260, ldq=260, nq=0) == 0           # ... fp32 rows: of 4
    refused(b"dim=4096", dim=4096, ld=4096, ldq=4096)
    refused(b"rows_bf16", bf16=2)
    refused(b"ld_rows", ld=128)
    refused(b"ld_queries", ldq=128)
    refused(b"nrows", nrows=-1)
    refused(b"rows", rows=None)
    refused(b"queries", q=None)
    refused(b"cand_pos", cand=None)
    refused(b"out_dist", od=None)
    refused(b"out_dist", op=None)
    refused(b"nq=70000", nq=70000)
    assert call(kc=2048, k=10, nq=1, ws=p, wsb=8, tk=p) == -3  # a split needs nq * kc * 8 bytes of scratch
    assert b"workspace" in lib.amdrec_last_error()
    misaligned = C.c_void_p(p.value + 4)
    refused(b"aligned", rows=misaligned)


def test_refine_constructor_arguments_are_checked_before_the_device():
    from amdrec import ivfpq
    from amdrec.index import FAISSIndex
    for bad in ("fp16", "", "FP32", 1, True):
        with pytest.raises(ValueError, match="refine"):
            FAISSIndex(256, index_type="IVFPQ", refine=bad)
    for t in ("Flat", "IVF"):
        for kind in ("fp32", "bf16"):
            with pytest.raises(ValueError, match="IVFPQ"):
                FAISSIndex(256, index_type=t, refine=kind)
    for f in (0, -3, 2.5, "4", None, True):
        with pytest.raises(ValueError, match="refine_factor"):
            FAISSIndex(256, index_type="IVFPQ", refine="fp32", refine_factor=f)
    with pytest.raises(ValueError, match="multiple of 8"):                   # (every legal pq_m makes the dimension a multiple
        ivfpq.check_refine("IVFPQ", 132, "bf16", 4)                         # of 16: the check guards the rule itself)
    ivfpq.check_refine("IVFPQ", 132, "fp32", 4)                             # fp32 takes every dimension the index takes
    ivfpq.check_refine("IVFPQ", 256, "bf16", 1)
    ivfpq.check_refine("IVFPQ", 256, None, 4)
    ivfpq.check_refine("Flat", 256, None, 4)
    # k' = min(k x factor, AMDREC_MAX_K): silent clamp, never below k
    assert ivfpq.refine_candidates(500, 4) == 2000 and ivfpq.refine_candidates(500, 8) == 2048
    assert ivfpq.refine_candidates(2048, 4) == 2048 and ivfpq.refine_candidates(7, 1) == 7


def test_oracle_refine_equals_brute_force():
    rng = np.random.default_rng(11)
    n, d, nq, kc, k = 300, 24, 9, 40, 25
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[5] = rows[4]                                          # an exact tie: the lower position first
    finite = np.ones(n, bool)
    finite[[7, 250]] = False
    rows[250, 3] = np.nan
    rows[99, 0] = np.inf                                       # not flagged: its distance is not finite all the same
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    cand = np.stack([rng.permutation(n)[:kc] for _ in range(nq)]).astype(np.int64)
    cand[0, :6] = [4, 5, 7, 250, 99, 17]
    cand[1, 30:] = -1                                          # unfilled tail
    cand[2, ::2] = -1                                          # unfilled slots anywhere
    cand[3, :] = -1
    D, I = ro.refine(rows, finite, xq, cand, k)
    for q in range(nq):
        items = []
        for p in cand[q]:
            if p < 0:
                continue
            dd = sum((float(xq[q, i]) - float(rows[p, i])) ** 2 for i in range(d))
            bad = (not finite[p]) or not np.isfinite(dd)
            items.append((1 if bad else 0, 0.0 if bad else dd, int(p)))
        items.sort()
        exp = items[:k]
        for i in range(k):
            if i < len(exp):
                assert I[q, i] == exp[i][2]
                if exp[i][0]:
                    assert D[q, i] == np.inf
                else:
                    assert abs(D[q, i] - exp[i][1]) <= 1e-12 * max(1.0, exp[i][1])
            else:
                assert I[q, i] == -1 and D[q, i] == np.inf
    assert (I[3] == -1).all()
    # bf16 rounding: round to nearest even on the 16 dropped bits
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.14159], np.float32)
    r = ro.bf16_round(x)
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == np.float32(1.0 + 2.0 ** -6) and r[3] == np.float32(1.0 + 2.0 ** -7)
    assert (r.view(np.uint32) & 0xFFFF == 0).all() and abs(r[4] + 3.14159) < 2.0 ** -7
    # check_rerank accepts the oracle itself and refuses a wrong order
    ex, total, _ = ro.check_rerank(rows, finite, xq, cand, k, I, D.astype(np.float32), d)
    assert ex == 0 and total == nq * k
    J = I.copy()
    J[4, [0, 9]] = J[4, [9, 0]]
    with pytest.raises(AssertionError):
        ro.check_rerank(rows, finite, xq, cand, k, J, D.astype(np.float32), d)


def test_refined_recall_is_never_below_unrefined_and_grows_with_the_factor():
    """Clustered corpus of the IVFPQ tests (20 000 x 256, 40 clusters), nlist 100, nprobe 10, m = 8, k = 100, the oracle's own
    codes.  Every true neighbour among the k' >= k candidates has at most k - 1 candidates ahead of it in exact distance,
    so it survives the re-rank: refined recall@k >= the code scan's recall@k, and the candidates of a larger factor are a
    superset.  Asserted without a margin (exact ties aside, and the generator has none)."""
    n, d, nlist, nprobe, m, k, nq = 20_000, 256, 100, 10, 8, 100, 32
    xb, xq = _clustered(n, d, 40, 7), _clustered(nq, d, 40, 8)
    cent, assign, cb, codes = ro.train_state(xb, nlist, m, seed=3)
    x64, q64 = xb.astype(np.float64), xq.astype(np.float64)
    truth = np.argsort(((q64 * q64).sum(1)[:, None] - 2 * q64 @ x64.T + (x64 * x64).sum(1)[None, :]), axis=1,
                       kind="stable")[:, :k]
    probes = ivfpq_oracle.coarse_probes(cent, xq, nprobe)
    _, plain = ivfpq_oracle.adc_search(codes, assign, cent, cb, xq, k, nprobe, probes=probes)
    base = ro.recall(plain, truth)
    recalls = []
    for factor in (1, 2, 4, 8):
        _, cand = ivfpq_oracle.adc_search(codes, assign, cent, cb, xq, k * factor, nprobe, probes=probes)
        _, ids = ro.refine(xb, None, xq, cand, k)
        recalls.append(ro.recall(ids, truth))
    print(f"recall@{k} vs exact: code scan {base:.4f}; refined at factors 1, 2, 4, 8: "
          + ", ".join(f"{r:.4f}" for r in recalls))
    assert recalls[0] >= base
    assert all(b >= a for a, b in zip(recalls, recalls[1:]))
    assert recalls[-1] > base                                   # and the stage does something on this corpus


def test_seed_check_of_the_exactness_test_with_the_bound_perturbed_oracle(capsys):
    """The corpus and query seeds of tests/test_ivfpq_refine_gpu.py's exactness test (21 / 22), an index of the same shape
    trained in numpy, factor 4: the float64 oracle's own order after every distance has moved by a uniform draw from
    +- scale x dist_bound, held against the unperturbed order by check_rerank's rule.  Recorded per k and scale: slots
    excused (near-tied rank neighbours, k-th boundary), slots the rule refuses, and both as a share of all slots.
    Asserted: what holds for any corpus (a returned candidate lies within two bounds of the oracle's at its slot), that
    k = 1 and 10 stay exact on these seeds even at the whole bound, and the cause of what the record shows at k = 100 and
    500: more than 1 % of the gaps between rank neighbours are below one bound (more near-tied pairs than the cap could
    excuse, some in runs of three and more), which is a property of 2000 candidates of one query on this corpus, not of
    the seeds.  A kernel whose error is a hundredth of the bound stays far under the cap with nothing refused."""
    n, d, nq = 20_000, 256, 64
    xb, xq = _clustered(n, d, 40, 21), _clustered(nq, d, 40, 22)
    cent, assign, cb, codes = ro.train_state(xb, 100, 8, seed=3)
    probes = ivfpq_oracle.coarse_probes(cent, xq, 10)
    lines = []
    for k in (1, 10, 100, 500):
        _, cand = ivfpq_oracle.adc_search(codes, assign, cent, cb, xq, 4 * k, 10, probes=probes)
        fD, fI = ro.refine(xb, None, xq, cand, 4 * k)
        for scale in (1.0, 0.1, 0.01):
            gI, _ = ro.perturbed_order(fD, fI, k, scale, d, np.random.default_rng(k))
            ex, refused, worst = ro.order_differences(fD, fI, gI, k, d)
            lines.append(f"k {k:3d} scale {scale:4.2f}: excused {ex:4d} ({ex / (nq * k):.4f}), refused {refused:3d} "
                         f"({refused / (nq * k):.4f}) of {nq * k} slots")
            assert worst <= 2.0 * scale * (1 + 1e-6), (k, scale, worst)
            if k <= 10:
                assert ex == 0 and refused == 0, (k, scale)
        if k >= 100:
            gaps = np.diff(fD[:, :k], axis=1)
            share = float((gaps < ro.dist_bound(fD[:, 1:k], d)).mean())
            lines.append(f"k {k:3d}: {share:.3f} of the gaps between rank neighbours among the best k are below one bound")
            assert share > 0.01                                # more near-tied pairs than the cap could excuse
    with capsys.disabled():
        print("\n" + "\n".join(lines))
