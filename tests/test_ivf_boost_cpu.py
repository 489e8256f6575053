"""CPU: the host side of stage-1 score boosts in the inverted-list scans - the opt-in flag of FAISSIndex and its refusals
(before the library is touched), the seven *_boosted exports and their refusals (every C call returns before its first HIP
call), the flag's place in the saved header, R1b's condition on the shapes of the GPU cases, and the host oracle against a
slot-by-slot loop.  No GPU."""
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

from amdrec import _lib
from tests import eligible_oracle as eo, ivf_boost_oracle as bo, ivf_eligible_oracle as io

TWINS = {"amdrec_ivf_scan_boosted": "amdrec_ivf_scan", "amdrec_ivf_scan_eligible_boosted": "amdrec_ivf_scan_eligible",
         "amdrec_ivf_scan_grouped_boosted": "amdrec_ivf_scan_grouped",
         "amdrec_ivf_scan_grouped_eligible_boosted": "amdrec_ivf_scan_grouped_eligible",
         "amdrec_ivf_scan_grouped_mixed_boosted": "amdrec_ivf_scan_grouped_mixed",
         "amdrec_ivf_scan_grouped_mixed_eligible_boosted": "amdrec_ivf_scan_grouped_mixed_eligible",
         "amdrec_ivf_filter_bounds_boosted": "amdrec_ivf_filter_bounds"}


def _fake_pointer():
    raw = ctypes.create_string_buffer(4096 + 256)
    return raw, (ctypes.addressof(raw) + 255) // 256 * 256            # non-null, aligned, never dereferenced


def _bare(index_type, **attrs):
    """An index object that was never constructed: the refusals depend on neither a device nor the library."""
    from amdrec.index import FAISSIndex
    idx = object.__new__(FAISSIndex)
    idx.index_type = index_type
    for k, v in attrs.items():
        setattr(idx, k, v)
    return idx


# ---- the flag ---------------------------------------------------------------------------------------------------------------------
def test_ivfpq_with_the_flag_is_refused_before_the_library_is_touched(monkeypatch):
    from amdrec.index import FAISSIndex
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    with pytest.raises(NotImplementedError, match="IVFPQ"):
        FAISSIndex(64, index_type="IVFPQ", nlist=8, nprobe=2, list_boosts=True)
    with pytest.raises(NotImplementedError, match="IVFPQ"):
        _bare("IVFPQ").enable_list_boosts()
    idx = _bare("IVFPQ", list_boosts=True)                              # however the attribute got there: IVFPQ takes no boost
    with pytest.raises(NotImplementedError, match="follow-up"):
        idx._check_boost(1.0)


def test_check_boost_follows_the_flag_without_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    q = np.zeros((2, 8), dtype=np.float32)
    # flagged, with boosts: passes, masked or not (an IVF index with both flags composes them)
    idx = _bare("IVF", list_boosts=True, _boosts=torch.zeros(4), _boost_max=1.0)
    assert idx._check_boost(1.0) is True and idx._check_boost(torch.zeros(2)) is True
    assert idx._check_boost(1.0, masked=True) is True
    assert idx._check_boost(None) is False and idx._check_boost(None, masked=True) is False
    # flagged, without boosts: ValueError
    for call in (lambda: _bare("IVF", list_boosts=True)._check_boost(1.0),
                 lambda: _bare("IVF", list_boosts=True).search_device(q, 3, boost_weight=1.0),
                 lambda: _bare("IVF", list_boosts=True).search(q, 3, boost_weight=[1.0, 2.0]),
                 lambda: _bare("IVF", list_boosts=True).batch_search(q, 3, boost_weight=0.5)):
        with pytest.raises(ValueError, match="without boosts"):
            call()
    # non-finite scalar weights, a wrong weight count
    for w in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            idx._check_boost(w)
        with pytest.raises(ValueError, match="finite"):
            idx.search(q, 3, boost_weight=[1.0, w])
    with pytest.raises(ValueError, match="3 boost weights for 2 queries"):
        idx.search(q, 3, boost_weight=[1.0, 2.0, 3.0])
    with pytest.raises(TypeError):
        idx._check_boost(True)
    # not flagged: what it always raised, whatever it holds
    for other in (_bare("IVF"), _bare("IVF", list_boosts=False), _bare("IVF", _boosts=torch.zeros(4)), _bare("IVFPQ")):
        for call in (lambda: other._check_boost(1.0), lambda: other.search_device(q, 3, boost_weight=1.0),
                     lambda: other.add(q, boosts=[1.0, 2.0]), lambda: other.set_boosts([1.0, 2.0])):
            with pytest.raises(NotImplementedError, match="follow-up") as e:
                call()
            assert "Flat index only" in str(e.value)
        assert other._check_boost(None) is False
    # Flat ignores the flag, and keeps refusing a boost together with masks
    flat = _bare("Flat", list_boosts=True, _boosts=torch.zeros(4), _boost_max=1.0)
    assert flat._check_boost(1.0) is True
    with pytest.raises(NotImplementedError, match="follow-up"):
        flat._check_boost(1.0, masked=True)


def test_pipeline_calls_follow_the_flag_without_the_library(monkeypatch):
    from amdrec.pipeline import AdRecommenderInference, TwoStageRetriever
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    rec = object.__new__(AdRecommenderInference)
    rec.heads_mode = "all"
    rec.faiss_index = _bare("IVF", list_boosts=True)                    # flagged, no boosts yet
    z = torch.zeros((2, 3))
    for call in (lambda: rec.recommend_device(z, z, stage1_boost=1.0), lambda: rec.batch_recommend([{}], stage1_boost=1.0),
                 lambda: rec.recommend_ads({}, stage1_boost=1.0), lambda: rec.recommend_tensors(z, z, stage1_boost=1.0)):
        with pytest.raises(ValueError, match="without boosts"):
            call()
    two = object.__new__(TwoStageRetriever)
    two.faiss_index = rec.faiss_index
    with pytest.raises(ValueError, match="without boosts"):
        two.retrieve_and_rank(z, z, stage1_boost=1.0)
    rec.faiss_index = _bare("IVF", list_boosts=True, _boosts=torch.zeros(4), _boost_max=0.0)
    with pytest.raises(ValueError, match="finite"):
        rec.recommend_device(z, z, stage1_boost=float("nan"))


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
def test_the_seven_exports_exist_and_are_bound():
    lib = _lib.load()
    for name, twin in TWINS.items():
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == len(getattr(lib, twin).argtypes) + 2, name
    assert lib.amdrec_ivf_filter_bounds_boosted.argtypes[-1] is ctypes.c_float
    assert lib.amdrec_abi_version() == 14 == _lib.ABI_VERSION


def test_boosted_entries_refuse_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    raw, p = _fake_pointer()
    E = (p, p, p)                                                       # list_tags, require_all, require_any

    def pairs(nq=2, lb=p, w=p, e=()):
        f = lib.amdrec_ivf_scan_eligible_boosted if e else lib.amdrec_ivf_scan_boosted
        return f(p, 64, 64, p, p, p, nq, 64, p, p, 4, p, 100, 0, None, *e, lb, w)

    def grouped(nq=2, lb=p, w=p, e=()):           # nq = 0 <-> nothing to scan: no query tiles
        f = lib.amdrec_ivf_scan_grouped_eligible_boosted if e else lib.amdrec_ivf_scan_grouped_boosted
        return f(p, 64, 64, p, p, 8, 100, p, 64, p, p, 10 if nq else 0, 32, p, p, p, 4, p, 100, 0, None, 0, None, None, *e, lb, w)

    def mixed(nq=2, lb=p, w=p, e=()):
        f = lib.amdrec_ivf_scan_grouped_mixed_eligible_boosted if e else lib.amdrec_ivf_scan_grouped_mixed_boosted
        return f(p, 64, p, 64, 64, p, p, 8, 100, p, 64, p, 64, p, p, 10 if nq else 0, 32, p, p, 100, 0, p, 1, p, p, None, *e, lb, w)

    for call in (pairs, grouped, mixed):
        for e in ((), E):
            for kw, word in ((dict(lb=None), b"list_boosts is null"), (dict(w=None), b"weight is null"),
                             (dict(lb=p + 2), b"list_boosts must be 4-byte aligned"),
                             (dict(w=p + 1), b"weight must be 4-byte aligned")):
                assert call(e=e, **kw) == -1 and word in lib.amdrec_last_error(), (call.__name__, kw, lib.amdrec_last_error())
            assert call(nq=0, lb=None, w=None, e=e) == 0                # nothing to scan: AMDREC_OK, as the twins
        # the eligibility pointers are still refused by name, in front of the boost's
        assert call(e=(None, p, p), lb=None) == -1 and b"list_tags is null" in lib.amdrec_last_error()
        assert call(e=(p, p, p + 4)) == -1 and b"require_any must be 8-byte aligned" in lib.amdrec_last_error()
    # the twins' own refusals still come first
    assert lib.amdrec_ivf_scan_boosted(p, 64, 62, p, p, p, 2, 64, p, p, 4, p, 100, 0, None, None, None) == -1
    assert b"multiple of 4" in lib.amdrec_last_error()

    def bounds(nq=2, w=p, bmax=1.0, q=p, dim=64):
        return lib.amdrec_ivf_filter_bounds_boosted(q, nq, 64, dim, p, 64, p, p, 1, p, None, w, bmax)
    for kw, word in ((dict(w=None), b"weight is null"), (dict(w=p + 2), b"weight must be 4-byte aligned"),
                     (dict(bmax=-1.0), b"boost_max"), (dict(bmax=float("inf")), b"boost_max"),
                     (dict(bmax=float("nan")), b"boost_max"), (dict(q=None), b"null pointer"), (dict(dim=60), b"multiple of 8")):
        assert bounds(**kw) == -1 and word in lib.amdrec_last_error(), (kw, lib.amdrec_last_error())
    assert bounds(nq=0, w=None) == 0
    del raw


# ---- the saved header ------------------------------------------------------------------------------------------------------------
class _NoDevice:
    """Stands in for the device side of save(): FAISSIndex.save only calls .cpu().numpy() on slices."""

    def __init__(self, a):
        self.a = a

    def __getitem__(self, s):
        return _NoDevice(self.a[s])

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def _header(path):
    with open(path, "rb") as f:
        f.read(9)
        (hl,) = struct.unpack("<Q", f.read(8))
        return json.loads(f.read(hl).decode())


@pytest.mark.parametrize("index_type, flag, want", [("IVF", True, True), ("IVF", False, False), ("Flat", True, False)])
def test_saved_header_carries_the_flag(index_type, flag, want, tmp_path):
    idx = _bare(index_type, list_boosts=flag, list_tags=False, dimension=8, nlist=4, nprobe=2, pq_m=8, refine=None,
                refine_factor=4, verbose=False, _n=0, _ids=_NoDevice(np.zeros(0, np.int64)),
                _xb=_NoDevice(np.zeros((0, 8), np.float32)), _keeps_rows=True, _tags=None, _state=None, _identity=True,
                _host_ids=None)
    path = str(tmp_path / "ix")
    idx.save(path)
    h = _header(path)
    assert h.get("list_boosts", False) is want and ("list_boosts" in h) == want      # absent when off: an earlier file


def test_load_reads_the_flag_with_a_default(tmp_path, monkeypatch):
    """load() sets the flag from the header before it creates the index; a header without the field gives False."""
    from amdrec.index import FAISSIndex, _MAGIC
    seen = []

    class Reached(Exception):
        pass

    def create(self):
        seen.append(self.list_boosts)
        raise Reached
    monkeypatch.setattr(FAISSIndex, "_create_index", create)
    for field, want in (({}, False), ({"list_boosts": True}, True), ({"list_boosts": False}, False), ({"list_tags": True}, False)):
        header = dict(dimension=8, index_type="IVF", nlist=4, nprobe=2, ntotal=0, identity_ids=True, arrays=[], **field)
        hj = json.dumps(header).encode()
        path = str(tmp_path / f"ix{len(seen)}")
        with open(path, "wb") as f:
            f.write(_MAGIC + struct.pack("<Q", len(hj)) + hj)
        idx = _bare("IVF", pq_m=8, list_boosts=not want)
        with pytest.raises(Reached):
            idx.load(path)
        assert seen[-1] is want


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, nprobe", io.R1_SHAPES)
def test_r1b_condition_holds_for_the_gpu_shapes(name, nprobe):
    """No query's probed lists can fill the 2048 slots of the plain search: the nprobe longest lists (float64 assignment to
    the given centres) hold fewer rows."""
    x, c, nlist = io.corpus(name)
    assert len(c) == nlist
    rows = io.longest_lists_rows(x, c, nprobe)
    print(f"{name} nprobe {nprobe}: the {nprobe} longest lists hold {rows} rows")
    assert rows < bo.PLAIN_K


def test_patterns_and_weights():
    assert bo.weights_for(8).tolist() == [np.float32(v) for v in (0, 1, -1, 0.25, 4, 1e-3, 0, 1)]
    n = 4096
    for name in bo.PATTERNS:
        b = bo.pattern(name, n)
        assert b.dtype == np.float32 and b.shape == (n,) and np.isfinite(b).all()
    assert (bo.pattern("quantised", n) == 64.0).sum() == n // 10 and (bo.pattern("sparse_half", n) == 0.5).sum() == n // 100
    s = bo.pattern("signed", n)
    assert (s == 0.5).sum() == n // 20 and (s == -1.0).sum() == n // 10 - n // 20


def test_rekey_matches_a_slot_by_slot_loop():
    rng = np.random.default_rng(11)
    n, nq, filled = 500, 13, 300
    tags = eo.tags_for(n, 3)
    a, y = io.masks_cycle(nq)
    w = bo.weights_for(nq)
    pos = np.full((nq, bo.PLAIN_K), -1, dtype=np.int64)
    sc = np.full((nq, bo.PLAIN_K), -np.inf, dtype=np.float32)
    for q in range(nq):
        pos[q, :filled] = rng.permutation(n)[:filled]
        sc[q, :filled] = np.sort(rng.standard_normal(filled).astype(np.float32))[::-1]
        sc[q, filled - 3:filled] = -np.inf                              # NaN rows of the plain search: filed as -inf ...
        pos[q, filled - 3:filled] = np.sort(pos[q, filled - 3:filled])  # ... and, like every tie, in position order
    for name in bo.PATTERNS:
        boost = bo.pattern(name, n)
        for k in (10, 100, 400):
            for masks in ((), (tags, a, y)):
                D, I = bo.rekey(pos, sc, boost, w, k, *masks)
                rD, rI = bo.rekey_loops(pos, sc, boost, w, k, *masks)
                assert np.array_equal(I, rI) and np.array_equal(D, rD), (name, k, bool(masks))
            D, I = bo.rekey(pos, sc, boost, w, k)
            have = min(k, filled)
            assert np.array_equal(I[0, :have], pos[0, :have]) and (I[:, have:] == -1).all()       # w = 0: the plain order
            assert np.array_equal(D[0, :have], sc[0, :have])
    # exact ties under the quantised pattern at w = 4: settled by position
    boost = bo.pattern("quantised", n)
    near = np.where(np.isfinite(sc), sc * np.float32(1e-4), sc)         # inner products a few ulps of 256 apart
    D, I = bo.rekey(pos, near, boost, w, 100)
    rD, rI = bo.rekey_loops(pos, near, boost, w, 100)
    assert np.array_equal(I, rI) and np.array_equal(D, rD)
    top = D[4] > 200                                                    # query 4: w = 4, the boosted rows lead at 256 + ip
    assert 10 < top.sum() and len(np.unique(D[4][top])) < top.sum()     # exact ties ...
    for v in np.unique(D[4][top]):
        assert (np.diff(I[4][D[4] == v]) > 0).all()                     # ... settled by position
    full = pos.copy()
    full[:, -1] = 7
    with pytest.raises(AssertionError, match="whole probed set"):
        bo.rekey(full, sc, boost, w, 10)
