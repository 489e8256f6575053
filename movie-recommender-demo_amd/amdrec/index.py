"""Device-resident retrieval index: drop-in for the reference's ``FAISSIndex`` wrapper
(faiss_retrieval.py:14-256) with the faiss calls replaced by libamdrec HIP kernels.

Same constructor arguments, method names, argument meaning and return conventions:
``search`` returns ``(ad_ids, distances)`` in that order (faiss_retrieval.py:164-166),
numpy in / numpy out, inputs are never mutated (the wrapper copies via ``astype``,
:114, :146), default ids are a running ``arange`` (:121-123), unknown ``index_type`` raises
``ValueError`` (:73).  Extra, for the on-device pipeline: ``search_device`` takes and returns
device tensors and never synchronises with the host.

Layout in HBM: corpus ``[capacity, dimension]`` float32 row-major, rows L2-normalised at
``add`` time, 1 KiB per row at d=256 (1.024 GB per 1M ads: the whole 10M corpus of
BASELINE config 4 is 10.24 GB, 3.6 % of one MI355X's 288 GB); ids int64 ``[capacity]``.
An IVFPQ index keeps no fp32 corpus: ``pq_m`` bytes of codes per row plus the row's list (amdrec.ivfpq), and its
``search`` returns approximate squared L2 distances (ascending), faiss IndexIVFPQ's default metric.  With ``refine`` it also
keeps every normalised row (fp32 or bf16, insertion order) and re-ranks the codes' candidates by exact distance.
"""
from __future__ import annotations

import json
import os
import struct
import time
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib, boost as _boost, auction as _auction, eligible as _eligible, exclude as _exclude, group_cap as _group_cap, include as _include, ivf, ivfpq, probes as _probes, rows_edit as _rows_edit

_MAGIC = b"AMDRECIX1"
ADD_BATCH = 1 << 18            # IVFPQ add: rows normalised and encoded per batch (256 MB of fp32 at d = 256)
INDEX_TYPES = ("Flat", "IVF", "IVFPQ", "HNSW")


def _encode_id(x):
    """JSON form of one arbitrary ad id (the reference pickles id_map, faiss_retrieval.py:208-218; this format never
    unpickles): [tag, value] with tag i / f / s / n.  Other types are refused at save time."""
    if isinstance(x, (bool, np.bool_)):
        raise TypeError("ad ids of type bool cannot be saved; use int or str")
    if isinstance(x, (int, np.integer)):
        return ["i", int(x)]
    if isinstance(x, (float, np.floating)):
        return ["f", float(x)]
    if isinstance(x, str):
        return ["s", x]
    if x is None:
        return ["n", None]
    raise TypeError(f"ad ids of type {type(x).__name__} cannot be saved; use int, float, str or None")


def _decode_id(e):
    if isinstance(e, str):            # files written by the round-1 format (ids stringified)
        return e
    tag, v = e
    return {"i": int, "f": float, "s": str, "n": lambda _: None}[tag](v)


class _Handle:
    """The attributes of a faiss index object that the reference touches
    (``index.ntotal``, ``index.is_trained``, ``index.nprobe``: faiss_retrieval.py:90, :127, :150)."""

    def __init__(self, owner):
        self._o = owner

    @property
    def ntotal(self):
        return self._o._n

    @property
    def is_trained(self):
        return self._o._trained

    @property
    def nprobe(self):
        if self._o.index_type not in ("IVF", "IVFPQ"):
            raise AttributeError("nprobe")
        return self._o.nprobe

    @nprobe.setter
    def nprobe(self, v):
        self._o.nprobe = int(v)


class FAISSIndex:
    def __init__(self, dimension: int, index_type: str = "IVF", nlist: int = 100, nprobe: int = 10,
                 use_gpu: bool = False, device=None, verbose: bool = False, prefilter: str = "bf16", pq_m: int = 8,
                 refine: Optional[str] = None, refine_factor: int = 4, list_tags: bool = False,
                 list_boosts: bool = False, aware_probes: bool = False):
        """``use_gpu`` is accepted for signature compatibility; the index always lives on the
        HIP device (``device`` or the current one) - there is no CPU engine.
        ``prefilter`` (Flat only): "bf16" keeps a bf16 copy of the corpus next to the fp32 one and searches with
        amdrec_flat_search_mixed (bf16 MFMA filter, fp32 re-score, certified exact); "fp32" = amdrec_flat_search.
        ``pq_m`` (IVFPQ only): sub-quantizers of 8 bits each, 4 / 8 / 16 / 32; 8 is the reference's value.
        ``refine`` (IVFPQ only): None = codes only; "fp32" / "bf16" also keep every normalised row in that format (1024 /
        512 bytes per ad at d = 256; "bf16" needs dimension % 8 == 0) and a search for k re-ranks the
        min(k * ``refine_factor``, 2048) best candidates of the code scan by their exact squared L2 distance to the kept row
        (for "bf16": to the bf16-rounded row), as faiss's IndexRefineFlat does.  The clamp to 2048 (AMDREC_MAX_K) is silent.
        ``list_tags`` (IVF / IVFPQ; ignored for Flat, which takes masks anyway): the index also keeps its tag words in list
        order (8 bytes per ad next to the lists, rebuilt with the list layout) and its searches take ``require_all`` /
        ``require_any``: the predicate is tested inside the list scans.  Without it an IVF / IVFPQ index refuses masks;
        ``enable_list_tags()`` opts in an index that is already built or loaded.
        ``list_boosts`` (IVF; ignored for Flat, which takes boosts anyway; IVFPQ raises NotImplementedError): the index also
        keeps its stage-1 score boosts in list order (4 bytes per ad next to the lists, rebuilt with the list layout) and takes
        ``add(boosts=)`` / ``set_boosts`` / ``boost_weight=``: the key s = ip + w_q * boost[r] is evaluated inside the list
        scans (amdrec.boost has the rule).  Without it an IVF index refuses boosts; ``enable_list_boosts()`` opts in an index
        that is already built or loaded.
        ``aware_probes`` (IVF / IVFPQ; ignored for Flat): the index also keeps per-list summaries of its list-order tags and
        boosts (24 bytes per list) and a search that carries masks and / or a boost weight chooses its ``nprobe`` lists among
        those that can hold an eligible row, by similarity plus the list's best boost term (amdrec.probes has the rule); a
        search with neither, and ``probe_policy="similarity"``, probe as always.  ``enable_aware_probes()`` opts in an index
        that is already built or loaded."""
        if index_type == "IVFPQ" and list_boosts:
            raise NotImplementedError(_boost.LIST_BOOSTS_IVFPQ)
        if prefilter not in ("bf16", "fp32"):
            raise ValueError("prefilter must be 'bf16' or 'fp32'")
        self.prefilter = prefilter
        self.dimension = int(dimension)
        self.index_type = index_type
        self.nlist = int(nlist)
        self.nprobe = int(nprobe)
        self.pq_m = int(pq_m)
        self.refine, self.refine_factor = refine, refine_factor
        self.list_tags = bool(list_tags)
        self.list_boosts = bool(list_boosts)
        self.aware_probes = bool(aware_probes)
        self.use_gpu = use_gpu
        self.verbose = verbose
        self.device = torch.device(device if device is not None else "cuda")
        self._create_index()

    # -- construction ---------------------------------------------------------------
    def _create_index(self):
        if self.index_type not in INDEX_TYPES:
            raise ValueError(f"Unknown index type: {self.index_type}")          # :73
        if self.index_type == "HNSW":
            raise NotImplementedError(
                f"{self.index_type} is outside the MI355X hot path (SURVEY.md §2 #12): use 'Flat', 'IVF' or 'IVFPQ'")
        if self.dimension % 4 or not (4 <= self.dimension <= 2048):
            raise ValueError("dimension must be a multiple of 4 in [4, 2048]")
        if self.index_type == "IVFPQ":
            ivfpq.check_pq_m(self.dimension, self.pq_m)
            ivfpq.check_nlist(self.nlist)
        ivfpq.check_refine(self.index_type, self.dimension, self.refine, self.refine_factor)
        _lib.load()
        self._xb = torch.empty((0, self.dimension), dtype=torch.float32, device=self.device)
        self._ids = torch.empty((0,), dtype=torch.int64, device=self.device)
        self._n = 0
        # bf16 shadow of the corpus + its largest row norm (the mixed search's error bound)
        self._mixed = self.index_type == "Flat" and self.prefilter == "bf16" and self.dimension % 8 == 0
        self._xb16 = torch.empty((0, self.dimension), dtype=torch.bfloat16, device=self.device)
        self._maxnorm = torch.zeros(2, dtype=torch.float32, device=self.device)     # [max row norm, max row rounding-error norm]
        self._tags: Optional[torch.Tensor] = None    # int64 [capacity] eligibility tags (amdrec.eligible), allocated on first use
        self._groups: Optional[torch.Tensor] = None  # int64 [capacity] group keys (amdrec.group_cap), allocated on first use
        self._bids: Optional[torch.Tensor] = None    # float32 [capacity] bids (amdrec.auction), allocated on first use
        self._boosts: Optional[torch.Tensor] = None  # float32 [capacity] stage-1 score boosts (amdrec.boost), allocated on first use
        self._boost_max = 0.0                        # host: >= max |boost| over every value ever stored (the search's error bound)
        self._identity = True          # ids == arange(n): remap is the identity
        self._nonfinite = False        # Flat: a stored row holds a NaN, so a search can leave slots unfilled with k <= n
        self.n_fixup_out: Optional[torch.Tensor] = None    # Flat: device int32[1] that receives the C entry's n_fixup (diagnostics)
        self._host_ids: Optional[list] = None   # only for non-integer ids
        self._host_pos = None          # (len(_host_ids), {id: [positions]}) for exclusion lists, built on first use
        self._id_table = None          # custom integer ids: (sorted ids, their positions) for include lists, built on first use
        self._default_ids_ok = True    # False once remove_ids has moved rows: a default id (= position) could repeat a kept id
        self._trained = self.index_type == "Flat"
        self._keeps_rows = self.index_type != "IVFPQ"    # IVFPQ: codes only, no fp32 corpus on the device
        self._state = None             # set by train(): the IVFState / IVFPQState behind ...
        self._ivf = None               # ... an IVF index, or the coarse level of ...
        self._pq = None                # ... an IVFPQ index
        self.index = _Handle(self)
        self._log(f"Created {self.index_type} index with dimension {self.dimension}")

    def _log(self, msg):
        if self.verbose:
            print(msg)

    # -- helpers --------------------------------------------------------------------
    def _to_device_f32(self, a) -> torch.Tensor:
        """fp32 device COPY of the input (``astype('float32')`` at :114 / :146 copies)."""
        if isinstance(a, torch.Tensor):
            t = a.detach().to(device=self.device, dtype=torch.float32, copy=True)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32)).to(self.device)
        if t.dim() != 2 or t.shape[1] != self.dimension:
            raise ValueError(f"expected [n, {self.dimension}] embeddings, got {tuple(t.shape)}")
        return t.contiguous()

    def _normalize_(self, t: torch.Tensor) -> torch.Tensor:
        lib = _lib.load()
        if t.shape[0] == 0:
            return t
        _lib.check(lib.amdrec_l2_normalize(_lib.ptr(t), t.stride(0), _lib.ptr(t), t.stride(0), t.shape[0],
                                           self.dimension, _lib.stream_ptr(self.device)))
        return t

    def _reserve(self, n):
        cap = self._ids.shape[0]                      # ids and rows grow together
        if n <= cap:
            return
        new_cap = max(n, int(cap * 1.5), 1024)

        def grown(t):
            new = torch.empty((new_cap,) + t.shape[1:], dtype=t.dtype, device=self.device)
            new[:self._n].copy_(t[:self._n])
            return new
        self._ids = grown(self._ids)
        if self._tags is not None:
            self._tags = grown(self._tags)
        if self._groups is not None:
            self._groups = grown(self._groups)
        if getattr(self, "_bids", None) is not None:
            self._bids = grown(self._bids)
        if getattr(self, "_boosts", None) is not None:
            self._boosts = grown(self._boosts)
        if self._keeps_rows:
            self._xb = grown(self._xb)
            if self._mixed:
                self._xb16 = grown(self._xb16)

    def _state_class(self):
        """-> (class of the trained state behind this index type, its train() arguments after nlist); (None, ()) for Flat."""
        return {"IVF": (ivf.IVFState, ()),
                "IVFPQ": (ivfpq.IVFPQState, (self.pq_m, self.refine, self.refine_factor))}.get(self.index_type, (None, ()))

    def _set_state(self, state):
        self._state = state
        self._pq = None if self._keeps_rows else state
        self._ivf = state if self._keeps_rows else state.ivf
        self._trained = True
        if getattr(self, "list_tags", False):
            self._ivf.tag_source = self._ensure_tags
        if self._takes_list_boosts():
            self._ivf.boost_source = self._boost_tensor
        if self._aware():
            self._ivf.aware_probes = True

    def _aware(self) -> bool:
        """An IVF / IVFPQ index that opted into aware probes (``aware_probes=True`` / ``enable_aware_probes()``)."""
        return bool(getattr(self, "aware_probes", False)) and self.index_type != "Flat"

    def enable_aware_probes(self):
        """Opt an IVF / IVFPQ index that is already built (or was loaded from a file saved without the flag) into aware probes
        (amdrec.probes): from now on it keeps the per-list summaries of its list-order tags and boosts (made here when those
        copies stand, else with them) and a search with masks and / or a boost weight chooses its probes among the feasible
        lists.  The flag is saved with the index.  Nothing to do for Flat."""
        self.aware_probes = True
        if self._ivf is not None and self.index_type != "Flat":
            self._ivf.enable_aware_probes()

    def enable_list_tags(self):
        """Opt an IVF / IVFPQ index that is already built (or was loaded from a file saved without the flag) into eligibility
        masks: from now on it keeps its tags in list order (made here when the lists are laid out, else with the layout) and
        its searches take ``require_all`` / ``require_any``.  The flag is saved with the index.  Nothing to do for Flat."""
        self.list_tags = True
        if self._ivf is not None:
            self._ivf.tag_source = self._ensure_tags
            self._ivf.refresh_list_tags()

    def _takes_list_boosts(self) -> bool:
        """An IVF index that opted into boosts in its list scans (``list_boosts=True`` / ``enable_list_boosts()``)."""
        return self.index_type == "IVF" and getattr(self, "list_boosts", False)

    def _takes_boosts(self) -> bool:
        return self.index_type == "Flat" or self._takes_list_boosts()

    def _boost_tensor(self) -> Optional[torch.Tensor]:
        """The boosts [capacity], or None for an index that never saw one (it keeps no list-order copy either)."""
        return getattr(self, "_boosts", None)

    def enable_list_boosts(self):
        """Opt an IVF index that is already built (or was loaded from a file saved without the flag) into stage-1 score
        boosts: from now on it keeps its boosts in list order (made here when the lists are laid out, else with the layout)
        and takes ``add(boosts=)`` / ``set_boosts`` / ``boost_weight=``.  The flag is saved with the index.  Nothing to do for
        Flat; IVFPQ raises NotImplementedError (its scan holds L2 distances of codes: out of scope)."""
        if self.index_type == "IVFPQ":
            raise NotImplementedError(_boost.LIST_BOOSTS_IVFPQ)
        self.list_boosts = True
        if self._ivf is not None and self.index_type == "IVF":
            self._ivf.boost_source = self._boost_tensor
            self._ivf.refresh_list_boosts()

    def _shadow_rows(self, lo, hi):
        """(Re)build rows [lo, hi) of the bf16 shadow from the fp32 rows and fold their norms into _maxnorm."""
        if not self._mixed or hi <= lo:
            return
        lib = _lib.load()
        x, y = self._xb[lo:hi], self._xb16[lo:hi]
        _lib.check(lib.amdrec_bf16_rows(_lib.ptr(x), hi - lo, x.stride(0), self.dimension, _lib.ptr(y), y.stride(0),
                                        _lib.ptr(self._maxnorm), _lib.stream_ptr(self.device)))

    def _check_masks(self, require_all, require_any) -> bool:
        """Were eligibility masks passed?  A Flat index takes them, an IVF / IVFPQ index only when it keeps list-order tags
        (``list_tags=True`` / ``enable_list_tags()``); checked before the library is touched."""
        if require_all is None and require_any is None:
            return False
        if self.index_type != "Flat" and not getattr(self, "list_tags", False):
            raise NotImplementedError(
                f"eligibility masks (require_all / require_any) on an {self.index_type} index need its list-order tags: construct "
                "it with list_tags=True or call enable_list_tags().  Without them only the Flat index takes masks; the "
                "list scans are the follow-up that this opt-in switches on (DESIGN.md, 'Eligibility masks in the "
                "inverted-list scans')")
        return True

    def _ensure_tags(self) -> torch.Tensor:
        """The tag words [capacity], allocated on first use: rows that were never given a tag have tag 0."""
        if self._tags is None:
            self._tags = torch.zeros((self._ids.shape[0],), dtype=torch.int64, device=self.device)
        return self._tags

    def set_tags(self, tags):
        """Replace the tag word of every row: ``tags`` [ntotal] (anything amdrec.eligible.as_words takes, or a device int64
        tensor).  Out of place - a new tensor is swapped in and the old one is never written -, so a search in flight or a
        captured graph keeps the tags it started with."""
        words = _eligible.device_words(tags, self._n, self.device)
        new = torch.zeros((self._ids.shape[0],), dtype=torch.int64, device=self.device)
        new[:self._n].copy_(words)
        self._tags = new
        if self._ivf is not None:                                    # list_tags: the list-order copy follows the swap
            self._ivf.refresh_list_tags()

    def get_tags(self) -> torch.Tensor:
        """The tag words, device int64 [ntotal] (a copy; zeros for an index that never saw a tag)."""
        if self._tags is None:
            return torch.zeros((self._n,), dtype=torch.int64, device=self.device)
        return self._tags[:self._n].clone()

    def _ensure_groups(self) -> torch.Tensor:
        """The group keys [capacity], allocated on first use: rows that were never given a key are ungrouped (-1)."""
        if self._groups is None:
            self._groups = torch.full((self._ids.shape[0],), -1, dtype=torch.int64, device=self.device)
        return self._groups

    def set_groups(self, groups):
        """Replace the group key of every row: ``groups`` [ntotal] integers (amdrec.group_cap: advertiser, campaign - the
        caller decides; negative = ungrouped, never capped).  Out of place - a new tensor is swapped in and the old one is
        never written -, so a search in flight or a captured graph keeps the groups it started with."""
        keys = _group_cap.device_keys(groups, self._n, self.device)
        new = torch.full((self._ids.shape[0],), -1, dtype=torch.int64, device=self.device)
        new[:self._n].copy_(keys)
        self._groups = new

    def get_groups(self) -> torch.Tensor:
        """The group keys, device int64 [ntotal] (a copy; -1 everywhere for an index that never saw a group)."""
        if self._groups is None:
            return torch.full((self._n,), -1, dtype=torch.int64, device=self.device)
        return self._groups[:self._n].clone()

    def _ensure_bids(self) -> torch.Tensor:
        """The bids [capacity], allocated on first use: rows that were never given a bid have 1.0."""
        if getattr(self, "_bids", None) is None:
            self._bids = torch.ones((self._ids.shape[0],), dtype=torch.float32, device=self.device)
        return self._bids

    def set_bids(self, bids):
        """Replace the bid of every row: ``bids`` [ntotal] numbers (amdrec.auction: finite, >= 0, the unit is the caller's).
        Out of place - a new tensor is swapped in and the old one is never written -, so a selection in flight or a captured
        graph keeps the bids it started with."""
        vals = _auction.device_bids(bids, self._n, self.device)
        new = torch.ones((self._ids.shape[0],), dtype=torch.float32, device=self.device)
        new[:self._n].copy_(vals)
        self._bids = new

    def get_bids(self) -> torch.Tensor:
        """The bids, device float32 [ntotal] (a copy; 1.0 everywhere for an index that never saw a bid)."""
        if getattr(self, "_bids", None) is None:
            return torch.ones((self._n,), dtype=torch.float32, device=self.device)
        return self._bids[:self._n].clone()

    def _ensure_boosts(self) -> torch.Tensor:
        """The boosts [capacity], allocated on first use: rows that were never given a boost have 0.0."""
        if getattr(self, "_boosts", None) is None:
            self._boosts = torch.zeros((self._ids.shape[0],), dtype=torch.float32, device=self.device)
        return self._boosts

    def set_boosts(self, boosts):
        """Replace the stage-1 score boost of every row: ``boosts`` [ntotal] numbers (amdrec.boost: finite, any sign).  Out
        of place - a new tensor is swapped in and the old one is never written -, so a search in flight or a captured
        graph keeps the boosts it started with.  Flat, and IVF with ``list_boosts`` (the list-order copy follows the swap)."""
        if not self._takes_boosts():
            raise NotImplementedError(_boost.follow_up_index(self.index_type))
        vals, bmax = _boost.device_boosts(boosts, self._n, self.device)
        new = torch.zeros((self._ids.shape[0],), dtype=torch.float32, device=self.device)
        new[:self._n].copy_(vals)
        self._boosts = new
        self._boost_max = bmax
        if self._ivf is not None:                                    # list_boosts: the list-order copy follows the swap
            self._ivf.refresh_list_boosts()

    def get_boosts(self) -> torch.Tensor:
        """The boosts, device float32 [ntotal] (a copy; 0.0 everywhere for an index that never saw a boost)."""
        if getattr(self, "_boosts", None) is None:
            return torch.zeros((self._n,), dtype=torch.float32, device=self.device)
        return self._boosts[:self._n].clone()

    def _check_boost(self, boost_weight, masked: bool = False) -> bool:
        """Was a stage-1 boost weight passed?  Refused before the library is touched: a weight on an IVFPQ index, on an IVF
        index without ``list_boosts``, or on a Flat index together with eligibility masks (NotImplementedError, the
        follow-up; an IVF index with ``list_tags`` and ``list_boosts`` takes both), a weight on an index without boosts, a
        non-finite scalar weight."""
        if boost_weight is None:
            return False
        if not self._takes_boosts():
            raise NotImplementedError(_boost.follow_up_index(self.index_type))
        if masked and self.index_type == "Flat":
            raise NotImplementedError(_boost.FOLLOW_UP_MASKS)
        if getattr(self, "_boosts", None) is None:
            raise ValueError("boost_weight on an index without boosts: give them with add(..., boosts=) or set_boosts()")
        if not isinstance(boost_weight, torch.Tensor):
            if isinstance(boost_weight, (int, float, np.integer, np.floating, bool, np.bool_)):
                _boost.check_weight(boost_weight)
        return True

    def _check_auction(self, rank_by, reserve):
        """The ``rank_by`` / ``reserve`` arguments -> (does the auction run, the reserve as amdrec.auction.check_reserve
        returns it).  Refused before the library is touched: an unknown rank_by, "ecpm" on an index that holds no bids, a
        reserve without "ecpm", a negative or non-finite scalar reserve."""
        auction = _auction.check_rank_by(rank_by)
        if auction and getattr(self, "_bids", None) is None:
            raise ValueError('rank_by="ecpm" on an index without bids: give them with add(..., bids=) or set_bids()')
        return auction, _auction.check_reserve(reserve, auction=auction)

    def _check_group_cap(self, max_per_group, what: str = "max_per_group"):
        """A ``max_per_group`` argument -> the cap as the entries take it, or None for "no cap".  Refused before the library
        is touched: a cap of 0 or below, and a cap on an index that holds no group keys."""
        if max_per_group is None:
            return None
        cap = _group_cap.check_cap(max_per_group, what)
        if getattr(self, "_groups", None) is None:
            raise ValueError(f"{what}={cap} on an index without group keys: give them with add(..., groups=) or set_groups()")
        return cap

    def _note_nonfinite(self, x):
        """Flat: remember whether a stored row is non-finite (one reduction and a host read at add / load time, so that
        search_device needs neither): such a row scores NaN and is never returned, which leaves slots unfilled."""
        if self.index_type == "Flat" and not self._nonfinite and x.shape[0]:
            self._nonfinite = not bool(torch.isfinite(x.sum()))      # normalised rows: a finite sum <=> every entry finite

    # -- reference API ----------------------------------------------------------------
    def train(self, embeddings):
        """faiss_retrieval.py:83-95: trains the coarse quantizer of IVF (and the product quantizer of IVFPQ); no-op for
        Flat."""
        if self._trained:
            return
        t0 = time.time()
        self._log(f"Training index on {len(embeddings)} samples...")
        cls, extra = self._state_class()
        self._set_state(cls.train(self._to_device_f32(embeddings), self.nlist, *extra))
        self._log(f"Index trained in {time.time() - t0:.2f}s")

    def set_trained_centroids(self, centroids):
        """Install an already trained coarse quantizer (IVF): ``centroids`` [nlist, dimension], unit rows.  This is how
        the ranks of a sharded index share ONE quantizer (amdrec.sharded.share_ivf_centroids) -
        faiss would do the same with ``index_ivf.quantizer`` handed to every shard."""
        if self.index_type != "IVF":
            raise ValueError("only an IVF index has a coarse quantizer")
        if self._n:
            raise ValueError("set the centroids before adding vectors")
        c = self._to_device_f32(centroids)
        if c.shape[0] != self.nlist:
            raise ValueError(f"expected {self.nlist} centroids, got {c.shape[0]}")
        self._set_state(ivf.IVFState(c))

    @property
    def centroids(self):
        """The trained coarse quantizer [nlist, dimension] (device tensor), or None."""
        return None if self._ivf is None else self._ivf.centroids

    def add(self, embeddings, ad_ids: Optional[List] = None, tags=None, groups=None, bids=None, boosts=None):
        """faiss_retrieval.py:97-127.  A Flat index also checks the added rows for non-finite values (_note_nonfinite: one
        reduction over them and a host read, i.e. add() synchronises), so that search_device never has to.
        ``tags``: one 64-bit eligibility word per added row (amdrec.eligible); without it the rows get tag 0, and an index
        that never sees a tag keeps no tag tensor at all.
        ``groups``: one int64 group key per added row (amdrec.group_cap; negative = ungrouped); without it the rows get -1,
        and an index that never sees a group keeps no group tensor at all.
        ``bids``: one float32 bid per added row (amdrec.auction; finite, >= 0); without it the rows get 1.0, and an index
        that never sees a bid keeps no bid tensor at all.
        ``boosts`` (Flat; IVF with ``list_boosts``): one float32 stage-1 score boost per added row (amdrec.boost; finite, any sign); without it the
        rows get 0.0, and an index that never sees a boost keeps no boost tensor at all."""
        if boosts is not None and not self._takes_boosts():
            raise NotImplementedError(_boost.follow_up_index(self.index_type))
        if ad_ids is None and not self._default_ids_ok:
            raise ValueError("add() without ad_ids after remove_ids(): default ids are corpus positions, and the removal has "
                             "moved the positions under the ids that stayed; pass ad_ids")
        if not self._trained:
            self.train(embeddings)                                   # :107-108 (un-normalised input)
        t0 = time.time()
        # fp32 copy of the input straight into index storage, renormalised there (:114-118): the
        # caller's array is never modified and no second device copy is made
        if isinstance(embeddings, torch.Tensor):
            src = embeddings.detach()
        else:
            src = torch.from_numpy(np.ascontiguousarray(np.asarray(embeddings), dtype=np.float32))
        if src.dim() != 2 or src.shape[1] != self.dimension:
            raise ValueError(f"expected [n, {self.dimension}] embeddings, got {tuple(src.shape)}")
        m = src.shape[0]
        new_tags = None if tags is None else _eligible.device_words(tags, m, self.device)    # (refused before anything changes)
        new_groups = None if groups is None else _group_cap.device_keys(groups, m, self.device)
        new_bids = None if bids is None else _auction.device_bids(bids, m, self.device)
        new_boosts = None if boosts is None else _boost.device_boosts(boosts, m, self.device)     # ``boosts``: amdrec.boost, 0.0 without
        self._reserve(self._n + m)
        if not self._keeps_rows:
            # normalised and encoded batch by batch: only the codes stay (and, with refine, the kept form of the rows).
            # Nothing is committed to the PQ state before the ids below are accepted (a rejected add must leave the index
            # as it was)
            pq_new = [self._pq.encode_rows(self._normalize_(
                src[b:b + ADD_BATCH].to(device=self.device, dtype=torch.float32, copy=True).contiguous()))
                for b in range(0, m, ADD_BATCH)]
        else:
            x = self._xb[self._n:self._n + m]
            x.copy_(src)                                             # casts + moves to the device
            self._normalize_(x)
            self._shadow_rows(self._n, self._n + m)
            self._note_nonfinite(x)
        if ad_ids is None:                                           # :121-122
            new_ids = torch.arange(self._n, self._n + m, dtype=torch.int64, device=self.device)
            if self._host_ids is not None:
                self._host_ids.extend(range(self._n, self._n + m))
        else:
            if len(ad_ids) != m:
                raise ValueError("len(ad_ids) != len(embeddings)")
            try:
                arr = np.asarray(ad_ids)
                if arr.dtype.kind not in "iu":
                    raise TypeError
                new_ids = torch.from_numpy(arr.astype(np.int64)).to(self.device)
                ident = bool(m == 0 or (arr[0] == self._n and np.array_equal(arr, np.arange(self._n, self._n + m))))
                self._identity = self._identity and ident
                if self._host_ids is not None:
                    self._host_ids.extend(arr.tolist())
            except TypeError:
                # arbitrary Python objects as ids: keep them on the host (plumbing, not compute)
                if self._host_ids is None:
                    self._host_ids = self._ids[:self._n].tolist()
                self._host_ids.extend(list(ad_ids))
                self._identity = False
                new_ids = torch.full((m,), -1, dtype=torch.int64, device=self.device)
        self._ids[self._n:self._n + m].copy_(new_ids)                # :123
        if new_tags is not None:
            self._ensure_tags()[self._n:self._n + m].copy_(new_tags)
        elif self._tags is not None:
            self._tags[self._n:self._n + m].zero_()
        if new_groups is not None:
            self._ensure_groups()[self._n:self._n + m].copy_(new_groups)
        elif self._groups is not None:
            self._groups[self._n:self._n + m].fill_(-1)
        if new_bids is not None:
            self._ensure_bids()[self._n:self._n + m].copy_(new_bids)
        elif getattr(self, "_bids", None) is not None:
            self._bids[self._n:self._n + m].fill_(1.0)
        if new_boosts is not None:
            self._ensure_boosts()[self._n:self._n + m].copy_(new_boosts[0])
            self._boost_max = max(self._boost_max, new_boosts[1])
        elif getattr(self, "_boosts", None) is not None:
            self._boosts[self._n:self._n + m].zero_()
        if self._pq is not None:
            self._pq.commit(pq_new)
        elif self._ivf is not None:
            self._ivf.append(x, self._n)
        self._n += m
        self._id_table = None
        self._log(f"Added embeddings in {time.time() - t0:.2f}s")
        self._log(f"Total index size: {self._n}")

    def remove_ids(self, ad_ids, return_kept: bool = False):
        """Remove every row whose id is in ``ad_ids`` -> the number of rows removed (``return_kept``: also ``kept``, device
        int64 [ntotal after the call], the old position of every row that stays).  No counterpart in the reference, whose
        wrapper can only add.

        Ids need not be unique in the index: every row that carries a listed id goes.  Ids that no row has and duplicates
        in the list are ignored; an empty list (or one that hits nothing) touches nothing.  The rows that stay keep their
        relative order - so the tie rule "lower position first" and the insertion order inside IVF lists give what a fresh
        index over the same rows gives - and they keep their ids: an index with default ids stops being one whose ids are
        its positions, and the id remap of custom ids takes over.  For that reason ``add`` without ``ad_ids`` raises
        ValueError from then on (a default id is a position, and the positions have moved under the ids that stayed); with
        explicit ids it works as before.  Removing every row leaves a trained, empty index in its initial id state.
        Integer ids are matched on the device; non-integers then raise TypeError and negatives ValueError.  With host-side
        object ids the list is resolved to positions on the host.

        Nothing is recomputed: IVF centroids, PQ codebooks, list assignments and codes stay as they are, and every stored
        array (rows, ids, assignments, codes, finite flags, refine rows) is gathered by ``kept`` with amdrec_rows_gather.
        Only a Flat index's bf16 shadow and its norm bound are rebuilt from the compacted rows (amdrec_bf16_rows), and its
        "a stored row is non-finite" state is taken again from the rows that stay; IVF lists are laid out again by the next
        search.  Always out of place: each array is gathered into a NEW tensor that then replaces the old one, which is
        never written - a search in flight or a captured graph (which pins the tensors it was captured with) keeps reading
        the index as it was: stale, never half-compacted.  Peak extra memory: one copy of the arrays being rebuilt.
        The call reads the number of survivors back, i.e. it synchronises with the host."""
        n = self._n
        if self._host_ids is not None:
            where = self._host_positions()
            remove = np.unique(np.asarray([p for x in dict.fromkeys(ad_ids) for p in where.get(x, ())], dtype=np.int64))
            keys = None                                              # the list holds positions
        else:
            remove = _rows_edit.removal_list(ad_ids)
            keys = None if self._identity else self._ids
        removed = 0
        if n and remove.size:
            kept, removed = _rows_edit.plan_for(keys, n, remove, self.device)
        if not removed:
            return (0, torch.arange(n, dtype=torch.int64, device=self.device)) if return_kept else 0
        m = n - removed

        def gather(t):
            return _rows_edit.gather_rows(t, kept, n)
        if self._host_ids is not None:
            self._host_ids = [self._host_ids[p] for p in kept.cpu().tolist()]
        self._host_pos = None                    # (keyed by len(_host_ids) alone: a later add of as many rows would revive it)
        self._id_table = None
        self._ids = gather(self._ids)
        if self._tags is not None:
            self._tags = gather(self._tags)
        if self._groups is not None:
            self._groups = gather(self._groups)
        if getattr(self, "_bids", None) is not None:
            self._bids = gather(self._bids)
        if getattr(self, "_boosts", None) is not None:           # (_boost_max stays: a bound of what is left)
            self._boosts = gather(self._boosts)
        if self._keeps_rows:
            self._xb = gather(self._xb)
        self._n = m
        if self._mixed:
            self._xb16 = torch.empty((m, self.dimension), dtype=torch.bfloat16, device=self.device)
            self._maxnorm = torch.zeros(2, dtype=torch.float32, device=self.device)
            self._shadow_rows(0, m)
        if self.index_type == "Flat":
            self._nonfinite = False
            self._note_nonfinite(self._xb[:m])
        if self._state is not None:
            self._state.compact(kept)
        self._identity = False
        self._default_ids_ok = False
        if m == 0:                               # empty again: positions restart, no id is left to collide with
            self._identity, self._default_ids_ok, self._host_ids = True, True, None
        self._log(f"Removed {removed} vectors; total index size: {self._n}")
        return (removed, kept) if return_kept else removed

    def resident_tensors(self) -> list:
        """Every device tensor the index keeps between calls (a captured graph's kernels point at them)."""
        return ([self._xb, self._ids, self._xb16, self._maxnorm] + ([] if self._tags is None else [self._tags]) +
                ([] if self._groups is None else [self._groups]) +
                ([] if getattr(self, "_bids", None) is None else [self._bids]) +
                ([] if getattr(self, "_boosts", None) is None else [self._boosts]) +
                list(getattr(self, "_id_table", None) or ()) +
                (self._state.resident_tensors() if self._state else []))

    @property
    def id_map(self) -> list:
        if self._host_ids is not None:
            return self._host_ids
        return self._ids[:self._n].tolist()

    def search_device(self, queries: torch.Tensor, k: int, normalize: bool = True,
                      return_positions: bool = False, pos_offset: int = 0, exclude: Optional[torch.Tensor] = None,
                      _exclude_positions: bool = False, require_all: Optional[torch.Tensor] = None,
                      require_any: Optional[torch.Tensor] = None, max_per_group: Optional[int] = None,
                      group_overfetch: int = 2, boost_weight=None, probe_policy: Optional[str] = None,
                      include: Optional[torch.Tensor] = None, return_injected: bool = False,
                      _include_positions: bool = False):
        """Device-to-device search, asynchronous on the current stream.
        -> (ids int64 [nq,k], scores float32 [nq,k]) on the device.  ``return_positions``: corpus
        positions (+ ``pos_offset``, the shard's first global row) instead of ids, -1 = unfilled.
        IVFPQ: the scores are squared L2 distances, ascending (+inf = unfilled): approximate, or exact with refine.
        Non-finite input (Flat): a row whose score against the query is NaN - it holds a NaN, or the query does - is never
        returned; the result is the exact top-k of the other rows and the tail stays unfilled: score -inf, position -1.
        As an id an unfilled slot reads ``id_map[-1]``, as in the reference, with default and with custom ids alike when
        the cause is a stored row (known since add / load).  A NaN QUERY on a finite index with default ids is not
        detected without a launch more per search: its slots come back as -1 there, as ``ids[n - 1]`` with custom ids.
        With the bf16 prefilter a non-finite row makes the shadow's norms non-finite and every query takes the exact
        fix-up scan (n_fixup of the C entry = nq).
        ``exclude``: device int64 [nq, E], per query the ad ids that must not be returned (negative = padding): the
        unfiltered search for k + E with those ids removed, order kept, cut to k (amdrec.exclude has the contract;
        k + E <= AMDREC_MAX_K).  It applies to ids also under ``return_positions``.  None or E = 0: the plain search, not
        one launch more.
        ``require_all`` / ``require_any`` (Flat; IVF / IVFPQ with ``list_tags``): device int64 [nq], the queries' eligibility
        masks against the rows' tags (amdrec.eligible has the contract): the exact top-k of each query's eligible rows, the tail unfilled when
        fewer than k are eligible.  Where one is given the other defaults to 0; both None: the plain search, not one
        launch more.  With ``exclude`` the filtered search runs for k + E.  IVF / IVFPQ: the index's own result restricted
        to eligible rows - the exact top-k, in its own order and with its own scores, of the eligible rows of the probed
        lists (IVFPQ refine re-ranks the best eligible candidates); without ``list_tags`` they raise NotImplementedError.
        The probed lists are the most similar ones whatever the masks, unless the index opted into ``aware_probes``
        (``probe_policy`` below): then they are the most similar lists that can hold an eligible row.
        ``max_per_group`` (None: no cap, not one launch more): at most that many rows of one group (``add(groups=)`` /
        ``set_groups``; negative keys are never capped) per query, greedy in the result's order (amdrec.group_cap).  The
        search runs as above - masks and exclusion included - for ``K1 = min(k * group_overfetch, AMDREC_MAX_K - E)``
        positions (E: the exclusion width, 0 without one; ValueError when K1 < k), and amdrec_group_cap_compact cuts them to
        ``k``.  The result is by definition the cap rule applied to the index's own top-K1 - for Flat, IVF and IVFPQ alike,
        with or without refine -, so a row can come back short (unfilled tail) although the corpus holds more ads of other
        groups beyond its K1 best.  An index without group keys and a cap <= 0 raise ValueError before the library is
        touched.
        ``boost_weight`` (Flat; IVF with ``list_boosts``; None: the plain search, not one launch more): a number or a device
        float32 [nq], the queries' weights w_q on the per-ad boosts (``add(boosts=)`` / ``set_boosts``): the exact top-k under
        s = ip + w_q * boost[r], s returned as the score (amdrec.boost has the rule), evaluated inside the corpus pass.
        IVF: the index's own result under that key - the exact top-k under s of the rows of the lists the PLAIN search
        probes (the probes are chosen by similarity alone: a boosted ad in an unprobed list is not found - unless the index
        opted into ``aware_probes``, whose coarse key adds w_q times the list's best boost); with masks on an index that also
        has ``list_tags``, of the eligible ones.
        ``exclude`` and ``max_per_group`` wrap the boosted search; on Flat together with masks, on IVF without
        ``list_boosts`` and on IVFPQ it raises NotImplementedError; on an index without boosts ValueError.
        ``probe_policy`` (IVF / IVFPQ; Flat has no probes): None = the index's ``aware_probes`` flag decides; "similarity" =
        the plain probes also on a flagged index (A/B runs); "aware" on an index without the flag raises ValueError before the
        library is touched.  Under the aware policy a search with masks and / or a boost weight probes the ``nprobe`` best
        FEASIBLE lists of amdrec.probes' rule and the result is the masked / boosted result over those lists; a search with
        neither probes as always, launch for launch.
        ``include`` (Flat, IVF; None or I = 0: the plain search, not one launch more): device int64 [nq, I], per query the ad
        ids that must be considered whatever their similarity rank (negative = padding; I <= min(k, 64)): the call's own
        result - masks, exclusion, boost weight and probe policy as given - with every listed ad that is known, eligible,
        not excluded and not NaN-scored merged in at its exact score, the result's lowest-ranked unlisted entries making room
        (amdrec.include has the rule; one launch of amdrec_include_merge behind the search).  Rows are read by position, so
        an IVF index returns a listed ad of an unprobed list too.  Custom integer ids resolve through a table built on first
        use (the lowest position of a repeated id); unknown ids are ignored.  With ``max_per_group`` it raises ValueError
        (the order of cap and injection is undecided), on IVFPQ NotImplementedError.  ``return_injected``: the call returns
        (ids, scores, injected) with ``injected`` bool [nq, k], True where a slot holds a merged-in ad (all False without a
        list)."""
        listed = include is not None and include.shape[-1] > 0
        if listed:                                                   # (refused before the library is touched)
            _include.check_include(k, include.shape[-1])
            if max_per_group is not None:
                raise ValueError(_include.CAP_ORDER)
            if self.index_type == "IVFPQ":
                raise NotImplementedError(_include.IVFPQ)
        aware = _probes.check_policy(probe_policy, self._aware())
        masked = self._check_masks(require_all, require_any)
        boosted = self._check_boost(boost_weight, masked)
        cap = self._check_group_cap(max_per_group)
        if listed:
            return self._search_including(queries, k, normalize, return_positions, pos_offset, exclude, _exclude_positions,
                                          require_all, require_any, boost_weight, probe_policy, include, _include_positions,
                                          return_injected)
        if return_injected:
            ids, scores = self.search_device(queries, k, normalize, return_positions, pos_offset, exclude, _exclude_positions,
                                             require_all, require_any, max_per_group, group_overfetch, boost_weight,
                                             probe_policy)
            return ids, scores, torch.zeros(ids.shape, dtype=torch.bool, device=ids.device)
        if cap is not None:
            return self._search_capped(queries, k, normalize, return_positions, pos_offset, exclude, _exclude_positions,
                                       require_all, require_any, cap, group_overfetch, boost_weight, probe_policy)
        if exclude is not None and exclude.shape[-1] > 0:
            return self._search_excluding(queries, k, normalize, return_positions, pos_offset, exclude, _exclude_positions,
                                          require_all, require_any, boost_weight, probe_policy)
        q = self._search_queries(queries, normalize)
        nq = q.shape[0]
        elig = masks = None
        if masked:
            masks = _eligible.device_masks(require_all, require_any, nq, self.device)
            elig = (self._ensure_tags(), *masks)
        boost = None
        if boosted:
            boost = (self._boosts, _boost.device_weights(boost_weight, nq, self.device), self._boost_max)
        list_boost = boost[1:] if boosted and self.index_type == "IVF" else None
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        pos = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        off = pos_offset if return_positions else 0
        if self.index_type == "IVF":
            self._ivf.search(self._xb, self._n, q, k, self.nprobe, scores, pos, pos_offset=off, elig=masks, boost=list_boost,
                             **({"aware": True} if aware else {}))
        elif self.index_type == "IVFPQ":                              # scores = squared L2 distances, ascending
            self._pq.search(q, k, self.nprobe, scores, pos, pos_offset=off, elig=masks, **({"aware": True} if aware else {}))
        elif self._mixed:
            flat_search_mixed(self._xb, self._xb16, self._maxnorm, self._n, q, k, scores, pos, pos_offset=off,
                              n_fixup=self.n_fixup_out, elig=elig, boost=boost)
        else:
            flat_search(self._xb, self._n, q, k, scores, pos, pos_offset=off, n_fixup=self.n_fixup_out, elig=elig, boost=boost)
        if return_positions or self._identity:
            # identity map: id == position for filled slots; unfilled (-1) slots map to
            # id_map[-1] in the reference (:159) - reproduce that too
            if return_positions:
                return pos, scores
            # a slot can be unfilled: k > n, an IVF probe set, a stored NaN row, fewer than k eligible rows (otherwise only
            # under a NaN query)
            if self._n and (k > self._n or self._state is not None or self._nonfinite or masked):
                pos = torch.where(pos < 0, pos + self._n, pos)
            return pos, scores
        lib = _lib.load()
        ids = torch.empty_like(pos)
        _lib.check(lib.amdrec_remap_ids(_lib.ptr(pos), _lib.ptr(self._ids), self._n, _lib.ptr(ids), pos.numel(),
                                        _lib.stream_ptr(self.device)))
        return ids, scores

    def _search_excluding(self, queries, k, normalize, return_positions, pos_offset, exclude, exclude_positions,
                          require_all=None, require_any=None, boost_weight=None, probe_policy=None):
        """search_device with an exclusion block: the unfiltered search for kc = k + E, the remap to ids where ids are not
        positions, amdrec_exclude_compact on the ids, and the id path's treatment of unfilled slots after that."""
        kc = _exclude.check_exclude(k, exclude.shape[-1])              # (before the library is touched)
        excl = _lib.require_gpu(exclude, "exclude", torch.int64)
        pos_c, sc_c = self.search_device(queries, kc, normalize=normalize, return_positions=True, require_all=require_all,
                                         require_any=require_any, boost_weight=boost_weight, probe_policy=probe_policy)
        fill = float("inf") if self.index_type == "IVFPQ" else float("-inf")
        if self._identity or exclude_positions:                      # the keys to match are the positions themselves
            pos, scores, _ = _exclude.compact(pos_c, sc_c, None, excl, k, fill)
        else:
            lib = _lib.load()
            ids_c = torch.empty_like(pos_c)
            _lib.check(lib.amdrec_remap_ids(_lib.ptr(pos_c), _lib.ptr(self._ids), self._n, _lib.ptr(ids_c), pos_c.numel(),
                                            _lib.stream_ptr(self.device)))
            _, scores, pos = _exclude.compact(ids_c, sc_c, pos_c, excl, k, fill, want_keys=False)
        return self._finish_compacted(pos, scores, return_positions, pos_offset)

    def _search_queries(self, queries, normalize) -> torch.Tensor:
        """The ``queries`` argument of search_device -> the contiguous [nq, dimension] block the kernels read."""
        q = _lib.require_gpu(queries, "queries")
        if q.dim() != 2 or q.shape[1] != self.dimension:
            raise ValueError(f"expected [nq, {self.dimension}] queries, got {tuple(q.shape)}")
        if not normalize:
            return q.contiguous()
        # faiss.normalize_L2 on the wrapper's copy (:146-147): ONE out-of-place launch (a float32 contiguous input is
        # read where it lies; the caller's tensor is never written) instead of a copy launch + an in-place one
        src = q.to(dtype=torch.float32).contiguous()
        q = torch.empty_like(src)
        if src.shape[0]:
            _lib.check(_lib.load().amdrec_l2_normalize(_lib.ptr(src), src.stride(0), _lib.ptr(q), q.stride(0), src.shape[0],
                                                       self.dimension, _lib.stream_ptr(self.device)))
        return q

    def _id_positions(self, ids: torch.Tensor) -> torch.Tensor:
        """Ad ids (int64 tensor on the index's device) -> corpus positions, -1 where no row carries the id (and for the
        negative padding); with repeated ids the lowest position.  Identity ids are their own positions (whoever reads
        them range-checks).  Custom integer ids go through a table that is built on first use - a stable sort of the ids -
        and dropped by add, remove_ids and load."""
        if self._identity:
            return ids
        if self._id_table is None:
            self._id_table = _include.build_id_table(self._ids[:self._n])
        return _include.lookup_positions(self._id_table, ids)

    def _search_including(self, queries, k, normalize, return_positions, pos_offset, exclude, exclude_positions, require_all,
                          require_any, boost_weight, probe_policy, include, include_positions, return_injected):
        """search_device with an include block: the search as it is (masks, exclusion and boost included) by position on
        the queries normalised here, amdrec_include_merge on its result, and the id path's treatment of unfilled slots."""
        if getattr(self, "_host_ids", None) is not None and not include_positions:
            raise TypeError("an include list of ad ids on an index with non-integer ids: search / batch_search resolve such "
                            "ids on the host; search_device takes integer ids only")
        incl = _lib.require_gpu(include, "include", torch.int64)
        q = self._search_queries(queries, normalize)
        nq = q.shape[0]
        if q.dtype != torch.float32:
            raise ValueError(f"queries must be float32, got {q.dtype}")
        if incl.dim() != 2 or incl.shape[0] != nq:
            raise ValueError(f"include must be int64 [{nq}, I], got {tuple(incl.shape)}")
        pos_r, sc_r = self.search_device(q, k, normalize=False, return_positions=True, exclude=exclude,
                                         _exclude_positions=exclude_positions, require_all=require_all,
                                         require_any=require_any, boost_weight=boost_weight, probe_policy=probe_policy)
        excluded = exclude is not None and exclude.shape[-1] > 0
        elig = boost = None
        if require_all is not None or require_any is not None:
            elig = (self._ensure_tags(), *_eligible.device_masks(require_all, require_any, nq, self.device))
        if boost_weight is not None:
            boost = (self._boosts, _boost.device_weights(boost_weight, nq, self.device))
        pos, scores, inj = _include.merge(
            pos_r, sc_r, incl if include_positions else self._id_positions(incl), self._xb, self._n, q, elig=elig,
            exclude=exclude if excluded else None,
            ids=None if (self._identity or exclude_positions or not excluded) else self._ids, boost=boost,
            want_injected=return_injected)
        out = self._finish_compacted(pos, scores, return_positions, pos_offset)
        return (*out, inj.view(torch.bool)) if return_injected else out

    def _search_capped(self, queries, k, normalize, return_positions, pos_offset, exclude, exclude_positions, require_all,
                       require_any, cap, group_overfetch, boost_weight=None, probe_policy=None):
        """search_device under a per-group cap: the search as it is (masks and exclusion included) for K1 positions,
        amdrec_group_cap_compact by position to k, and the id path's treatment of unfilled slots after that."""
        E = 0 if exclude is None else int(exclude.shape[-1])
        k1 = _group_cap.overfetch_k(k, group_overfetch, E)             # (before the library is touched)
        pos_c, sc_c = self.search_device(queries, k1, normalize=normalize, return_positions=True, exclude=exclude,
                                         _exclude_positions=exclude_positions, require_all=require_all, require_any=require_any,
                                         boost_weight=boost_weight, probe_policy=probe_policy)
        fill = float("inf") if self.index_type == "IVFPQ" else float("-inf")
        pos, scores = _group_cap.compact(pos_c, sc_c, self._groups, self._n, cap, k, fill)
        return self._finish_compacted(pos, scores, return_positions, pos_offset)

    def _finish_compacted(self, pos, scores, return_positions, pos_offset):
        """Positions (-1 = unfilled, anywhere) and scores after a compaction -> what search_device returns."""
        if return_positions:
            if pos_offset:
                pos = torch.where(pos < 0, pos, pos + pos_offset)
            return pos, scores
        if self._identity:
            # (after the compaction any slot can be unfilled: -1 reads id_map[-1], as in the plain search)
            return (torch.where(pos < 0, pos + self._n, pos) if self._n else pos), scores
        ids = torch.empty_like(pos)
        _lib.check(_lib.load().amdrec_remap_ids(_lib.ptr(pos), _lib.ptr(self._ids), self._n, _lib.ptr(ids), pos.numel(),
                                                _lib.stream_ptr(self.device)))
        return ids, scores

    def _exclude_block(self, exclude, nq: int) -> Optional[torch.Tensor]:
        """The ``exclude`` argument of search / batch_search -> device int64 [nq, E] (None: no list).  With host-side
        object ids the block holds corpus POSITIONS: every position of each excluded id (ids not in the index are ignored)."""
        if exclude is None:
            return None
        if self._host_ids is None:
            blk = _exclude.as_block(exclude, nq)
        else:
            if len(exclude) != nq:
                raise ValueError(f"{len(exclude)} exclusion lists for {nq} queries")
            where = self._host_positions()
            blk = _exclude.pad_exclusions([[p for x in dict.fromkeys(row) for p in where.get(x, ())] for row in exclude])
            blk = blk if blk.shape[1] else None
        return None if blk is None else torch.from_numpy(blk).to(self.device)

    def _host_positions(self) -> dict:
        """{id: [positions]} of the host-side object ids, built on first use and after every change of their number
        (remove_ids drops it: the number alone would not show a removal followed by an add of as many rows)."""
        if self._host_pos is None or self._host_pos[0] != len(self._host_ids):
            where = {}
            for p, x in enumerate(self._host_ids):
                where.setdefault(x, []).append(p)
            self._host_pos = (len(self._host_ids), where)
        return self._host_pos[1]

    def search(self, query_embeddings, k: int = 100, return_distances: bool = True, exclude=None, require_all=None,
               require_any=None, max_per_group: Optional[int] = None, group_overfetch: int = 2, boost_weight=None,
               probe_policy: Optional[str] = None, include=None):
        """faiss_retrieval.py:129-166.  numpy in, numpy out: (ad_ids, distances).  ``exclude``: one sequence of ad ids per
        query (or an integer array [nq, E], negative = padding) that must not be returned: see search_device.
        ``require_all`` / ``require_any``: the queries' eligibility masks, one 64-bit word each (one int for all queries, a
        sequence of ints, a uint64 / int64 array): see search_device.  ``max_per_group`` / ``group_overfetch``: the per-group
        cap on every query's result: see search_device.  ``boost_weight``: the stage-1 boost weight, one number for every
        query or a sequence of one per query: see search_device.  ``probe_policy``: None / "similarity" / "aware", how an IVF / IVFPQ
        index with ``aware_probes`` chooses its probes: see search_device.  ``include``: one sequence of ad ids per query (or
        an integer array [nq, I], negative = padding) that must be considered whatever their similarity rank: see
        search_device; ids of any type on an index with host-side object ids."""
        nq = len(query_embeddings)
        incl = self._include_block(include, nq, k, max_per_group)
        _probes.check_policy(probe_policy, self._aware())
        masked = self._check_masks(require_all, require_any)
        cap = (self._check_group_cap(max_per_group), group_overfetch)
        w = self._boost_weights(boost_weight, nq, masked)
        return self._search(query_embeddings, k, return_distances, self._exclude_block(exclude, nq),
                            _eligible.device_masks(require_all, require_any, nq, self.device), cap, w, probe_policy,
                            None if incl is None else torch.from_numpy(incl).to(self.device))

    def _include_block(self, include, nq: int, k: int, max_per_group=None) -> Optional[np.ndarray]:
        """The ``include`` argument of search / batch_search -> host int64 [nq, I] (None: no list), refused as search_device
        refuses it, before the library is touched.  With host-side object ids the block holds corpus POSITIONS: the first
        position of each listed id (ids not in the index are ignored)."""
        if include is None:
            return None
        if getattr(self, "_host_ids", None) is None:
            blk = _include.as_block(include, nq)
        else:
            if len(include) != nq:
                raise ValueError(f"{len(include)} include lists for {nq} queries")
            where = self._host_positions()
            blk = _include.pad_inclusions([[where[x][0] for x in dict.fromkeys(row) if x in where] for row in include])
            blk = blk if blk.shape[1] else None
        if blk is not None:
            _include.check_include(k, blk.shape[1])
            if max_per_group is not None:
                raise ValueError(_include.CAP_ORDER)
            if self.index_type == "IVFPQ":
                raise NotImplementedError(_include.IVFPQ)
        return blk

    def _boost_weights(self, boost_weight, nq: int, masked: bool) -> Optional[torch.Tensor]:
        """The ``boost_weight`` argument of search / batch_search -> device float32 [nq] (None: no boost), every value
        validated on the host."""
        if not self._check_boost(boost_weight, masked):
            return None
        return torch.from_numpy(_boost.as_weights(boost_weight, nq)).to(self.device)

    def _search(self, query_embeddings, k, return_distances, excl, masks=(None, None), cap=(None, 2), boost_weight=None,
                probe_policy=None, incl=None):
        """search with the exclusion lists already as a device block (_exclude_block), the masks as device words and the
        per-group cap as (max_per_group or None, group_overfetch)."""
        q = self._to_device_f32(query_embeddings)
        t0 = time.time()
        if self._host_ids is not None:
            pos, scores = self.search_device(q, k, normalize=True, return_positions=True, exclude=excl,
                                             _exclude_positions=True, require_all=masks[0], require_any=masks[1],
                                             max_per_group=cap[0], group_overfetch=cap[1], boost_weight=boost_weight,
                                             **({} if probe_policy is None else {"probe_policy": probe_policy}),
                                             **({} if incl is None else {"include": incl, "_include_positions": True}))
            idm = np.asarray(self._host_ids, dtype=object)
            ad_ids = idm[pos.cpu().numpy()]                          # pos == -1 -> id_map[-1]
        else:
            ids, scores = self.search_device(q, k, normalize=True, exclude=excl, require_all=masks[0], require_any=masks[1],
                                             max_per_group=cap[0], group_overfetch=cap[1], boost_weight=boost_weight,
                                             **({} if probe_policy is None else {"probe_policy": probe_policy}),
                                             **({} if incl is None else {"include": incl}))
            ad_ids = ids.cpu().numpy()
        distances = scores.cpu().numpy()
        self._log(f"Search completed in {(time.time() - t0) * 1000:.2f}ms for {len(q)} queries")
        if return_distances:
            return ad_ids, distances
        return ad_ids

    def batch_search(self, query_embeddings, k: int = 100, batch_size: int = 1000, exclude=None, require_all=None,
                     require_any=None, max_per_group: Optional[int] = None, group_overfetch: int = 2, boost_weight=None,
                     probe_policy: Optional[str] = None, include=None):
        """faiss_retrieval.py:168-194.  ``exclude`` (as in search) is padded once, to the longest list of the whole call,
        and sliced with the queries: the chunking does not change the result.  ``require_all`` / ``require_any`` (as in
        search) are sliced with the queries too.  ``max_per_group`` / ``group_overfetch`` (as in search) hold per query.
        ``include`` (as in search) is padded once, like ``exclude``, and sliced with the queries."""
        all_ids, all_d = [], []
        incl = self._include_block(include, len(query_embeddings), k, max_per_group)
        incl = None if incl is None else torch.from_numpy(incl).to(self.device)
        _probes.check_policy(probe_policy, self._aware())
        masked = self._check_masks(require_all, require_any)
        w = self._boost_weights(boost_weight, len(query_embeddings), masked)      # (sliced with the queries, like the masks)
        cap = (self._check_group_cap(max_per_group), group_overfetch)
        excl = self._exclude_block(exclude, len(query_embeddings))
        ma, my = _eligible.device_masks(require_all, require_any, len(query_embeddings), self.device)
        for i in range(0, len(query_embeddings), batch_size):
            ids, d = self._search(query_embeddings[i:i + batch_size], k, True,
                                  None if excl is None else excl[i:i + batch_size],
                                  (None, None) if ma is None else (ma[i:i + batch_size], my[i:i + batch_size]), cap,
                                  None if w is None else w[i:i + batch_size], probe_policy,
                                  None if incl is None else incl[i:i + batch_size])
            all_ids.append(ids)
            all_d.append(d)
        return np.vstack(all_ids), np.vstack(all_d)

    # -- persistence: own format (faiss' write_index binary is unreadable without faiss) --
    def save(self, filepath: str):
        """faiss_retrieval.py:196-221: index file + ``<path>.metadata`` sidecar.  The index file is
        ``AMDRECIX1 | u64 header_len | json header | raw arrays``; the sidecar is JSON with the
        reference's metadata fields (dimension, index_type, nlist, nprobe) - never pickle."""
        d = os.path.dirname(os.path.abspath(filepath))
        os.makedirs(d, exist_ok=True)
        arrays = [("ids", self._ids[:self._n].cpu().numpy())]
        if self._keeps_rows:
            arrays.insert(0, ("xb", self._xb[:self._n].cpu().numpy()))
        if self._tags is not None:                                   # (absent: an index that never saw a tag, as every earlier file)
            arrays.append(("tags", self._tags[:self._n].cpu().numpy()))
        if getattr(self, "_groups", None) is not None:               # (absent: an index that never saw a group, as every earlier file)
            arrays.append(("groups", self._groups[:self._n].cpu().numpy()))
        if self._state is not None:                                  # IVFPQ: codes, centroids, codebooks, assignment
            arrays += self._state.export_arrays()
        if getattr(self, "_bids", None) is not None:                 # (absent: an index that never saw a bid, as every earlier file)
            arrays.append(("bids", self._bids[:self._n].cpu().numpy()))
        if getattr(self, "_boosts", None) is not None:               # (absent: an index that never saw a boost, as every earlier file)
            arrays.append(("boosts", self._boosts[:self._n].cpu().numpy()))
        header = {"dimension": self.dimension, "index_type": self.index_type, "nlist": self.nlist,
                  "nprobe": self.nprobe, "ntotal": self._n, "identity_ids": self._identity,
                  "arrays": [{"name": n, "dtype": str(a.dtype), "shape": list(a.shape)} for n, a in arrays]}
        if self.index_type == "IVFPQ":
            header["pq_m"] = self.pq_m
            if self.refine is not None:                              # (absent: an unrefined index, as every earlier file)
                header["refine"], header["refine_factor"] = self.refine, int(self.refine_factor)
        if self.index_type != "Flat" and self.list_tags:             # (absent: no list-order tags, as every earlier file)
            header["list_tags"] = True
        if self._takes_list_boosts():                                # (absent: no list-order boosts, as every earlier file)
            header["list_boosts"] = True
        if self._aware():                                            # (absent: probes by similarity alone, as every earlier file)
            header["aware_probes"] = True
        if self._host_ids is not None:
            header["host_ids"] = [_encode_id(x) for x in self._host_ids]     # typed: ids round-trip as what they were
        hj = json.dumps(header).encode()
        with open(filepath, "wb") as f:
            f.write(_MAGIC)
            f.write(struct.pack("<Q", len(hj)))
            f.write(hj)
            for _, a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        with open(filepath + ".metadata", "w") as f:
            json.dump({k: header[k] for k in ("dimension", "index_type", "nlist", "nprobe", "ntotal")}, f)
        self._log(f"Index saved to {filepath}")

    def load(self, filepath: str):
        """faiss_retrieval.py:223-245."""
        with open(filepath, "rb") as f:
            if f.read(len(_MAGIC)) != _MAGIC:
                raise ValueError(f"{filepath} is not an amdrec index file")
            (hl,) = struct.unpack("<Q", f.read(8))
            header = json.loads(f.read(hl).decode())
            arrays = {}
            for spec in header["arrays"]:
                dt = np.dtype(spec["dtype"])
                cnt = int(np.prod(spec["shape"])) if spec["shape"] else 1
                arrays[spec["name"]] = np.frombuffer(f.read(cnt * dt.itemsize), dtype=dt).reshape(spec["shape"])
        self.dimension = header["dimension"]
        self.index_type = header["index_type"]
        self.nlist = header["nlist"]
        self.nprobe = header["nprobe"]
        self.pq_m = int(header.get("pq_m", self.pq_m))
        self.refine, self.refine_factor = header.get("refine"), int(header.get("refine_factor", 4))
        self.list_tags = bool(header.get("list_tags", False))
        self.list_boosts = bool(header.get("list_boosts", False))
        self.aware_probes = bool(header.get("aware_probes", False))
        self._create_index()
        n = header["ntotal"]
        self._reserve(n)
        if self._keeps_rows:
            self._xb[:n].copy_(torch.from_numpy(arrays["xb"].copy()))
        self._ids[:n].copy_(torch.from_numpy(arrays["ids"].copy()))
        if "tags" in arrays:
            self._ensure_tags()[:n].copy_(torch.from_numpy(arrays["tags"].copy()))
        if "groups" in arrays:
            self._ensure_groups()[:n].copy_(torch.from_numpy(arrays["groups"].copy()))
        if "bids" in arrays:
            self._ensure_bids()[:n].copy_(torch.from_numpy(arrays["bids"].copy()))
        if "boosts" in arrays:
            vals, self._boost_max = _boost.device_boosts(arrays["boosts"], n, self.device)
            self._ensure_boosts()[:n].copy_(vals)
        self._n = n
        self._shadow_rows(0, n)
        if self._keeps_rows:
            self._note_nonfinite(self._xb[:n])
        self._identity = header["identity_ids"]
        hid = header.get("host_ids")
        self._host_ids = None if hid is None else [_decode_id(x) for x in hid]
        self._id_table = None
        cls, extra = self._state_class()
        if cls is not None:
            self._set_state(cls.from_arrays(arrays, self.device, *extra[1:]))
        self._log(f"Index loaded from {filepath}")
        self._log(f"Index size: {self._n}")

    def get_stats(self):
        """faiss_retrieval.py:247-256."""
        return {"index_type": self.index_type, "dimension": self.dimension, "num_vectors": self._n,
                "is_trained": self._trained, "nlist": self.nlist, "nprobe": self.nprobe}


def benchmark_faiss_index(dimension: int = 256, num_vectors: int = 1000000, num_queries: int = 100, k: int = 100,
                          device="cuda", seed: int = 1234, index_types=("Flat", "IVF")):
    """The reference's only benchmark (faiss_retrieval.py:372-436): random corpus, add + search timings per
    index type.  ``index_types``: the arms to run, of Flat, IVF and IVFPQ (HNSW is outside the hot path); vectors and
    queries are drawn on the device (randn, as :390-391, seeded here)."""
    configs = {"Flat": {}, "IVF": {"nlist": 100, "nprobe": 10}, "IVFPQ": {"nlist": 100, "nprobe": 10}}
    for t in index_types:
        if t not in configs:
            raise ValueError(f"benchmark_faiss_index: unsupported index type {t!r}")
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    vectors = torch.randn((num_vectors, dimension), generator=g, device=device)
    queries = torch.randn((num_queries, dimension), generator=g, device=device)
    results = {}
    for index_type in index_types:
        config = configs[index_type]
        idx = FAISSIndex(dimension, index_type=index_type, device=device, **config)
        torch.cuda.synchronize()
        t0 = time.time()
        idx.add(vectors)
        torch.cuda.synchronize()
        add_time = time.time() - t0
        idx.search_device(queries, k)                                  # warm-up (lists, workspace)
        torch.cuda.synchronize()
        t0 = time.time()
        idx.search_device(queries, k)
        torch.cuda.synchronize()
        ms = (time.time() - t0) * 1000
        results[index_type] = {"add_time": add_time, "search_time_ms": ms, "per_query_ms": ms / num_queries}
    return results


def _elig_args(elig, n, nq):
    """(tags [>= n], require_all [nq], require_any [nq]) device int64 -> the three trailing pointers of the *_eligible entries."""
    tags, ma, my = (_lib.require_gpu(t, name, torch.int64) for t, name in zip(elig, ("tags", "require_all", "require_any")))
    if tags.dim() != 1 or tags.shape[0] < n or not tags.is_contiguous():
        raise ValueError(f"tags must be a contiguous int64 vector of at least {n} words, got {tuple(tags.shape)}")
    for t, name in ((ma, "require_all"), (my, "require_any")):
        if t.shape != (nq,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int64 [{nq}], got {tuple(t.shape)}")
    return _lib.ptr(tags), _lib.ptr(ma), _lib.ptr(my)


def _boost_args(boost, n, nq):
    """(boosts float32 [>= n], weights float32 [nq], boost_max) -> the three trailing arguments of the *_boosted entries."""
    b, w = (_lib.require_gpu(t, name, torch.float32) for t, name in zip(boost[:2], ("boosts", "boost_weight")))
    if b.dim() != 1 or b.shape[0] < n or not b.is_contiguous():
        raise ValueError(f"boosts must be a contiguous float32 vector of at least {n} values, got {tuple(b.shape)}")
    if w.shape != (nq,) or not w.is_contiguous():
        raise ValueError(f"boost_weight must be a contiguous float32 [{nq}], got {tuple(w.shape)}")
    return _lib.ptr(b), _lib.ptr(w), _lib.C.c_float(float(boost[2]))


def flat_search(xb: torch.Tensor, n: int, q: torch.Tensor, k: int, out_scores: torch.Tensor,
                out_pos: torch.Tensor, pos_offset: int = 0, n_fixup: Optional[torch.Tensor] = None, elig=None, boost=None):
    """amdrec_flat_search on device tensors (rows of xb[:n] and q already L2-normalised).  ``elig``: (tags, require_all,
    require_any) device int64 -> amdrec_flat_search_eligible."""
    lib = _lib.load()
    dev = q.device
    if q.shape[0] == 0:
        return
    nbytes = _lib.C.c_size_t(0)
    _lib.check(lib.amdrec_flat_search_workspace(q.shape[0], n, k, _lib.C.byref(nbytes)))
    ws = _lib.WORKSPACE.get(nbytes.value, dev)
    args = (_lib.ptr(xb), n, xb.stride(0) if xb.dim() == 2 and xb.shape[0] > 0 else xb.shape[-1], xb.shape[-1],
            _lib.ptr(q), q.shape[0], q.stride(0), k, pos_offset, _lib.ptr(out_scores), _lib.ptr(out_pos),
            _lib.ptr(ws), ws.numel(), _lib.ptr(n_fixup))
    if boost is not None:
        if elig is not None:
            raise NotImplementedError(_boost.FOLLOW_UP_MASKS)
        _lib.check(lib.amdrec_flat_search_boosted(*args, _lib.stream_ptr(dev), *_boost_args(boost, n, q.shape[0])))
    elif elig is None:
        _lib.check(lib.amdrec_flat_search(*args, _lib.stream_ptr(dev)))
    else:
        tail = _elig_args(elig, n, q.shape[0])
        _lib.check(lib.amdrec_flat_search_eligible(*args, _lib.stream_ptr(dev), *tail))


def flat_search_mixed(xb: torch.Tensor, xb16: torch.Tensor, max_norm: torch.Tensor, n: int, q: torch.Tensor, k: int,
                      out_scores: torch.Tensor, out_pos: torch.Tensor, pos_offset: int = 0,
                      n_fixup: Optional[torch.Tensor] = None, elig=None, boost=None):
    """amdrec_flat_search_mixed on device tensors: xb16 = amdrec_bf16_rows(xb), max_norm = its largest row norm.  ``elig``:
    (tags, require_all, require_any) device int64 -> amdrec_flat_search_mixed_eligible."""
    lib = _lib.load()
    dev = q.device
    if q.shape[0] == 0:
        return
    d = xb.shape[-1]
    nbytes = _lib.C.c_size_t(0)
    _lib.check(lib.amdrec_flat_search_mixed_workspace(q.shape[0], n, k, d, _lib.C.byref(nbytes)))
    ws = _lib.WORKSPACE.get(nbytes.value, dev)
    has = xb.dim() == 2 and xb.shape[0] > 0
    args = (_lib.ptr(xb), n, xb.stride(0) if has else d, d, _lib.ptr(xb16), xb16.stride(0) if has else d,
            _lib.ptr(max_norm), _lib.ptr(q), q.shape[0], q.stride(0), k, pos_offset, _lib.ptr(out_scores),
            _lib.ptr(out_pos), _lib.ptr(ws), ws.numel(), _lib.ptr(n_fixup))
    if boost is not None:
        if elig is not None:
            raise NotImplementedError(_boost.FOLLOW_UP_MASKS)
        _lib.check(lib.amdrec_flat_search_mixed_boosted(*args, _lib.stream_ptr(dev), *_boost_args(boost, n, q.shape[0])))
    elif elig is None:
        _lib.check(lib.amdrec_flat_search_mixed(*args, _lib.stream_ptr(dev)))
    else:
        tail = _elig_args(elig, n, q.shape[0])
        _lib.check(lib.amdrec_flat_search_mixed_eligible(*args, _lib.stream_ptr(dev), *tail))
