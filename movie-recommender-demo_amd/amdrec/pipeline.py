"""Drop-in for the reference's serving pipeline ``AdRecommenderInference`` (inference.py:21-331).

``recommend_ads(user_data, top_k=10, stage1_k=500, return_scores=True)`` keeps the reference's
argument names / defaults, stage order, ranking key (CTR only, inference.py:263) and result
schema (:272-288).  The whole hot path stays on the device between the feature tensors and
the final ``[B, top_k]`` result: UserTower -> L2 renorm -> exact IP top-``stage1_k`` ->
ranker over the candidates (user row broadcast, ad features gathered from a resident table)
-> top-``top_k``.  The reference crosses the host/device boundary four times per request
(inference.py:225-229, :241-248, :258-260); this path crosses it once each way.

Deviations, each forced by a reference defect:
* candidate ad features come from a real ``ad_features[N, 20]`` table indexed by corpus position
  (the reference draws ``torch.randint`` placeholders, inference.py:246-248);
* unknown categories map to ``'rare'`` if the encoder has it, else class 0 (the reference asks
  the encoder for a ``'missing'`` class that does not exist, inference.py:180);
* numerical features are cast to float32 after scaling (the reference feeds float64 into a
  float32 model, inference.py:193-195);
* the preprocessor sidecar is JSON (``preprocessor.json``), never a pickle.
"""
from __future__ import annotations

import json
import threading
import time
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, boost as _boost, auction as _auction, diversity as _diversity, value as _value, explore as _explore, eligible as _eligible, exclude as _exclude, include as _include, \
    rows_edit as _rows_edit
from .index import FAISSIndex
from .ranker import TransformerRanker
from .towers import TwoTowerModel

USER_COLS = [f"C{i}" for i in range(1, 7)]      # inference.py:46
AD_COLS = [f"C{i}" for i in range(7, 27)]       # inference.py:47
TASKS = ("ctr", "engagement", "revenue")


class Preprocessor:
    """The fitted state of CriteoDataPreprocessor that inference needs (data_preprocessing.py:
    label encoders' classes, numerical column list, StandardScaler mean/scale), as plain data."""

    def __init__(self, classes: Dict[str, List[str]], numerical_cols: List[str], mean, scale):
        self.classes = {c: list(v) for c, v in classes.items()}
        self._lookup = {c: {s: i for i, s in enumerate(v)} for c, v in self.classes.items()}
        self.numerical_cols = list(numerical_cols)
        self.mean = np.asarray(mean, dtype=np.float64)
        self.scale = np.asarray(scale, dtype=np.float64)
        self.feature_dims = {c: len(v) for c, v in self.classes.items()}

    def encode(self, col, value) -> int:
        lut = self._lookup[col]
        if value in lut:
            return lut[value]
        return lut.get("rare", 0)

    def save(self, path):
        with open(path, "w") as f:
            json.dump({"classes": self.classes, "numerical_cols": self.numerical_cols,
                       "mean": self.mean.tolist(), "scale": self.scale.tolist()}, f)

    @classmethod
    def load(cls, path):
        with open(path) as f:
            d = json.load(f)
        return cls(d["classes"], d["numerical_cols"], d["mean"], d["scale"])


def _load_checkpoint(model, path, device):
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    sd = ckpt["model_state_dict"] if isinstance(ckpt, dict) and "model_state_dict" in ckpt else ckpt  # :101-106
    model.load_state_dict(sd)
    return model.to(device).eval()


class AdRecommenderInference:
    def __init__(self, model_dir: Optional[str] = None, device: str = "cuda", *,
                 two_tower_model: Optional[TwoTowerModel] = None,
                 transformer_ranker: Optional[TransformerRanker] = None,
                 faiss_index: Optional[FAISSIndex] = None, ad_features=None,
                 preprocessor: Optional[Preprocessor] = None, verbose: bool = False,
                 cache_ad_projection: bool = True, heads: str = "all", ranker_engine: Optional[str] = None):
        """Either ``model_dir`` (files below) or the components directly.
        model_dir: preprocessor.json, two_tower_{best,final}.pt, transformer_ranker_{best,final}.pt,
        faiss_index.bin (+ .metadata) in this build's format, ad_features.npy [N, 20].
        ``heads`` (``heads_mode``): what stage 2 evaluates.  "all": every head on every candidate.  "ctr_first": the
        candidates are ranked by the CTR logit alone and the other tasks are reported for the winners only
        (inference.py:258-288), so the trunk and the CTR head run on every candidate and the other heads on the
        ``B * top_k`` winners' stored trunk rows (TransformerRanker.score_ctr_first / winner_scores).  ad_ids, scores and
        the CTR logits are bit-identical in both modes; in "ctr_first" ``logits`` holds the CTR row alone.  The mode does
        what it is told wherever it can run (``heads_mode_effective``); it is no tuning switch - DESIGN.md has the
        measured batch sizes at which it pays.
        ``ranker_engine``: the ranker's ``gemm_engine`` (TransformerRanker.ALL_ENGINES), set before its first pack; None leaves
        the ranker as it is.  "f16" is the opt-in single-product fp16 engine (reduced precision: DESIGN.md)."""
        if ranker_engine is not None and ranker_engine not in TransformerRanker.ALL_ENGINES:
            raise ValueError(f"ranker_engine must be None or one of {TransformerRanker.ALL_ENGINES}")
        self.heads_mode = self._check_heads(heads)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AmdrecError("AdRecommenderInference needs a HIP device (no CPU fallback)")
        self.verbose = verbose
        # candidate-side cache of the ranker's ad-half projection (TransformerRanker.cache_ad_projection):
        # N x d_model fp32 next to the ad-feature table, rebuilt when the weights change
        self.cache_ad_projection = cache_ad_projection
        _lib.load()
        if model_dir is not None:
            d = Path(model_dir)
            self.preprocessor = Preprocessor.load(d / "preprocessor.json")
            self.user_feature_dims = {c: self.preprocessor.feature_dims[c] for c in USER_COLS
                                      if c in self.preprocessor.feature_dims}
            self.ad_feature_dims = {c: self.preprocessor.feature_dims[c] for c in AD_COLS
                                    if c in self.preprocessor.feature_dims}
            self.numerical_dim = len(self.preprocessor.numerical_cols)
            tt = TwoTowerModel(self.user_feature_dims, self.ad_feature_dims, self.numerical_dim)   # :84-92
            p = d / "two_tower_best.pt"
            self.two_tower_model = _load_checkpoint(tt, p if p.exists() else d / "two_tower_final.pt", self.device)
            rk = TransformerRanker(self.user_feature_dims, self.ad_feature_dims, self.numerical_dim)  # :114-124
            p = d / "transformer_ranker_best.pt"
            self.transformer_ranker = _load_checkpoint(
                rk, p if p.exists() else d / "transformer_ranker_final.pt", self.device)
            self.faiss_index = FAISSIndex(256, index_type="IVF", nlist=100, nprobe=10, device=self.device)  # :145-151
            self.faiss_index.load(str(d / "faiss_index.bin"))
            ad_features = np.load(d / "ad_features.npy", allow_pickle=False)
        else:
            if two_tower_model is None or transformer_ranker is None or faiss_index is None or ad_features is None:
                raise ValueError("pass model_dir or all of two_tower_model, transformer_ranker, faiss_index, "
                                 "ad_features")
            self.preprocessor = preprocessor
            self.two_tower_model = two_tower_model.to(self.device).eval()
            self.transformer_ranker = transformer_ranker.to(self.device).eval()
            self.faiss_index = faiss_index
        if ranker_engine is not None:
            self.transformer_ranker.gemm_engine = ranker_engine
        if isinstance(ad_features, torch.Tensor):
            self.ad_features = ad_features.to(device=self.device, dtype=torch.int64).contiguous()
        else:
            self.ad_features = torch.from_numpy(np.ascontiguousarray(ad_features, dtype=np.int64)).to(self.device)
        if self.ad_features.shape[0] < self.faiss_index.index.ntotal:
            raise ValueError("ad_features has fewer rows than the index")

    # -- host-side feature prep (inference.py:160-197; CPU string work, not the hot path) -----
    def preprocess_user_features(self, user_data: dict):
        if self.preprocessor is None:
            raise ValueError("no preprocessor loaded")
        pp = self.preprocessor
        cat = [pp.encode(c, user_data["categorical"].get(c, "missing")) for c in USER_COLS if c in pp.classes]
        num = np.array([np.log1p(np.abs(user_data["numerical"].get(c, 0))) for c in pp.numerical_cols],
                       dtype=np.float64)
        num = ((num - pp.mean) / pp.scale).astype(np.float32)
        return torch.tensor([cat], dtype=torch.long), torch.from_numpy(num[None, :])

    def preprocess_batch(self, user_data_list: list, exclude: Optional[np.ndarray] = None,
                         masks: Optional[np.ndarray] = None, weights: Optional[np.ndarray] = None, draws=None):
        """Batch form of preprocess_user_features with the numerical transform on the device: categorical strings
        are label-encoded on the host (dictionary lookups), raw numericals are shipped as one float32 block and
        log1p / standardised by amdrec_prep_numerical.  -> (user_categorical [B,6] int64, user_numerical [B,13]
        float32), both on the device.  ``exclude`` (int64 [B, E], amdrec.exclude.pad_exclusions) rides in the same
        staging block and copy; the result is then (user_categorical, user_numerical, exclude on the device).  ``masks``
        (int64 [2, B]: the users' require_all and require_any words, amdrec.eligible) ride there too and come back last,
        as a device [2, B].  ``weights`` (float32 [B]: the users' stage-1 boost weights, amdrec.boost) ride behind them and
        come back after them, as a device float32 [B].  ``draws`` (amdrec.explore.host_arrays: float32 [B] temperatures and
        uint64 [B] seeds) ride behind those and come back last, as a device float32 [B] and a device int64 [B]."""
        pp = self.preprocessor
        if pp is None:
            raise ValueError("no preprocessor loaded")
        cols = [c for c in USER_COLS if c in pp.classes]
        B, nc, nn_ = len(user_data_list), len(cols), len(pp.numerical_cols)
        dev = self.ad_features.device
        # ONE pinned staging block [categorical int64 | raw numerical float32] and ONE H2D copy per call (two pageable
        # copies cost ~25 us of a 0.4 ms request); the block is reused once its previous copy has completed.  The block is
        # the calling thread's own (_staging): it is filled outside the enqueue lock, beside other threads' device work
        cat_bytes = B * nc * 8
        ex_off = (cat_bytes + B * nn_ * 4 + 7) // 8 * 8                 # the int64 exclusion block, 8-byte aligned
        m_off = ex_off + (0 if exclude is None else exclude.size * 8)   # the int64 mask words
        w_off = m_off + (0 if masks is None else 2 * B * 8)             # the float32 boost weights
        used = w_off + B * 4 if weights is not None else (m_off + 2 * B * 8 if masks is not None else
                                                          (cat_bytes + B * nn_ * 4 if exclude is None else m_off))
        s_off = (used + 7) // 8 * 8                                     # the uint64 seeds, 8-byte aligned, then the temperatures
        t_off = s_off + B * 8
        host, done = self._staging(used if draws is None else t_off + B * 4)
        hv = host.numpy()
        if draws is not None:
            hv[s_off:t_off].view(np.uint64)[:] = draws[1]
            hv[t_off:t_off + B * 4].view(np.float32)[:] = draws[0]
        if nc:
            hv[:cat_bytes].view(np.int64).reshape(B, nc)[:] = [[pp.encode(c, u["categorical"].get(c, "missing")) for c in cols]
                                                               for u in user_data_list]
        if nn_:
            hv[cat_bytes:cat_bytes + B * nn_ * 4].view(np.float32).reshape(B, nn_)[:] = [
                [float(u["numerical"].get(c, 0)) for c in pp.numerical_cols] for u in user_data_list]
        if exclude is not None:
            hv[ex_off:m_off].view(np.int64).reshape(exclude.shape)[:] = exclude
        if masks is not None:
            hv[m_off:m_off + 2 * B * 8].view(np.int64).reshape(2, B)[:] = masks
        if weights is not None:
            hv[w_off:w_off + B * 4].view(np.float32)[:] = weights
        with _lib.GATE.enqueue:
            pp_dev = getattr(self, "_pp_dev", (None,))
            if pp_dev[0] is not pp:
                pp_dev = self._pp_dev = (pp, torch.from_numpy(pp.mean.astype(np.float32)).to(dev),
                                         torch.from_numpy(pp.scale.astype(np.float32)).to(dev))
            blk = host.to(dev, non_blocking=True)
            done.record(torch.cuda.current_stream(dev))
            cat = blk[:cat_bytes].view(torch.int64).view(B, nc)
            x = blk[cat_bytes:cat_bytes + B * nn_ * 4].view(torch.float32).view(B, nn_)
            out = torch.empty_like(x)
            lib = _lib.load()
            _lib.check(lib.amdrec_prep_numerical(_lib.ptr(x), _lib.ptr(pp_dev[1]), _lib.ptr(pp_dev[2]),
                                                 _lib.ptr(out), x.shape[0], x.shape[1], _lib.stream_ptr(dev)))
        res = (cat, out)
        if exclude is not None:
            res += (blk[ex_off:m_off].view(torch.int64).view(exclude.shape),)
        if masks is not None:
            res += (blk[m_off:m_off + 2 * B * 8].view(torch.int64).view(2, B),)
        if weights is not None:
            res += (blk[w_off:w_off + B * 4].view(torch.float32),)
        if draws is not None:
            res += (blk[t_off:t_off + B * 4].view(torch.float32), blk[s_off:t_off].view(torch.int64))
        return res

    def _staging(self, nbytes: int, slot: str = "in"):
        """Pinned host block of at least ``nbytes`` + the event of its last use (waited for before it is handed out again).
        ``slot``: blocks of different slots are different memory, so the inputs ("in"), a separately shipped exclusion
        block ("excl") and the results ("out") of one call never wait for each other.  The blocks belong to the calling
        THREAD (``_per_thread``): a block's event only says that its last copy has completed, not that the thread that
        ordered the copy has finished reading the block, so a block shared by two threads could be overwritten under the
        one still converting its results."""
        st = self._per_thread().__dict__.setdefault("stage_bufs", {})
        size = 256
        while size < nbytes:
            size *= 2
        ent = st.get((slot, size))
        if ent is None:
            ent = st[(slot, size)] = (torch.empty(size, dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
        else:
            ent[1].synchronize()
        return ent[0][:nbytes], ent[1]

    def _per_thread(self):
        """The calling thread's part of this object's state: its pinned staging blocks and its timing events."""
        tl = self.__dict__.get("_thread_state")
        if tl is None:
            tl = self.__dict__.setdefault("_thread_state", threading.local())      # (setdefault: one winner among threads)
        return tl

    HEADS_MODES = ("all", "ctr_first")

    @classmethod
    def _check_heads(cls, heads):
        if heads not in cls.HEADS_MODES:
            raise ValueError(f"heads must be one of {cls.HEADS_MODES}, got {heads!r}")
        return heads

    def heads_mode_effective(self, heads: Optional[str] = None):
        """-> (the mode stage 2 runs for ``heads`` (None: ``heads_mode``), why not the requested one or None).  "ctr_first"
        on a ranker that cannot run it (TransformerRanker.ctr_first_unsupported_reason) runs "all": the results are the
        same by definition, and no call raises or warns for it."""
        mode = self._check_heads(self.heads_mode if heads is None else heads)
        if mode == "ctr_first":
            why = self.transformer_ranker.ctr_first_unsupported_reason()
            if why is not None:
                return "all", why
        return mode, None

    # -- the device hot path ------------------------------------------------------------------
    def _stage1(self, uc, un, stage1_k, check_indices, exclude=None, masks=(None, None), max_per_group=None, boost_weight=None,
                include=None):
        # the tower's launch also applies the search's query normalisation (faiss_retrieval.py:147): one launch fewer
        emb = self.two_tower_model.user_tower.encode(uc, un, check_indices=check_indices, renormalize=True)   # :223-227
        # exclude (device int64 [B, E] ad ids, or None): removed here, so the ranker only ever sees eligible ads
        # masks (device int64 [B] require_all / require_any, or None): tested inside the search, likewise
        # max_per_group (stage1_max_per_group, or None): the per-group cap on the candidate list (FAISSIndex.search_device)
        # boost_weight (stage1_boost: a number or device float32 [B], or None): the retrieval key ip + w * boost[ad], likewise
        # include (include_ad_ids: device int64 [B, I] ad ids, or None): merged into the search's result (amdrec.include); the
        # call then returns (positions, scores, injected)
        if include is not None:
            return self.faiss_index.search_device(emb, stage1_k, normalize=False, return_positions=True, exclude=exclude,
                                                  require_all=masks[0], require_any=masks[1], max_per_group=max_per_group,
                                                  boost_weight=boost_weight, include=include, return_injected=True)
        return self.faiss_index.search_device(emb, stage1_k, normalize=False,                  # :230-232
                                              return_positions=True, exclude=exclude, require_all=masks[0],
                                              require_any=masks[1], max_per_group=max_per_group, boost_weight=boost_weight)

    def _stage2(self, uc, un, cand_pos, top_k, check_indices, ids_are_positions=False, mark=None, out=None,
                excluded=False, heads=None, max_per_group=None, auction=None, diversity=None, head_weights=None, explore=None):
        """Ranker + selection over stage 1's positions ``cand_pos`` [B, stage1_k].  A negative position is a slot the search
        could not fill: no candidate.  The ranker still computes a (finite, unspecified) logit for it - every gather clamps
        the row - and the selection, which is handed the positions, ranks it after every real candidate: it is reported only
        where a user has fewer than ``top_k`` real candidates, as ad id -1 with probability 0.0 for every task.  Validity is
        decided here, by position: ``candidate_ids`` keeps the search's convention for such a slot (``id_map[-1]``; the
        position itself with ``ids_are_positions``), from which it can no longer be told.
        ``max_per_group`` (validated by the caller, None: no cap): the selection is amdrec_select_topk_capped over the index's
        group keys - at most that many winners of one group per user, greedy in the selection's order.
        ``auction`` (validated by the caller, None: rank by CTR): ``(reserve,)`` - the selection is amdrec_select_topk_auction
        over the index's bids (amdrec.auction has the rule), the cap inside it, and the result gains ``ecpm`` / ``prices``.
        ``diversity`` (validated by the caller, None: the selections above): ``(lam, pool)`` - the selection is
        amdrec_select_topk_diverse over the index's rows as they are at this call (amdrec.diversity has the rule), the cap
        inside it, and the result gains ``diversity_values``.
        ``head_weights`` (validated by the caller, None: the selections above): amdrec.value.check_head_weights' result or a
        static [B, n_tasks] buffer - the selection is amdrec_select_topk_value (``_value_auction`` with ``auction``), the cap
        inside it, every head on every candidate whatever ``heads_mode`` says, and the result gains ``values``.
        ``explore`` (validated by the caller, None: the selections above): ``(temperature, seeds, greedy)``, device float32 [B],
        device int64 [B] and the greedy prefix - the selection is amdrec_select_topk_sampled (amdrec.explore has the rule), the
        cap inside it, in either heads mode, and the result gains ``propensities``."""
        lib = _lib.load()
        B, stage1_k = cand_pos.shape
        rk = self.transformer_ranker
        if self.cache_ad_projection:
            rk.ensure_ad_cache(self.ad_features)
        # "ctr_first" (``heads``: a per-call override of ``heads_mode``): the trunk and the CTR head on every candidate, the
        # selection on that one logit row, the other heads on the winners.  A ranker or shape that cannot run it takes the
        # all-heads path below: the same results
        mode = self.heads_mode if heads is None else heads
        ctr_first = head_weights is None and mode != "all" and self.heads_mode_effective(mode)[0] == "ctr_first" and \
            rk.ctr_first_ready(self.ad_features, B * stage1_k, B * top_k)
        if ctr_first:
            tasks = rk._packed.tasks
            ctr, trunk = rk.score_ctr_first(uc, un, cand_pos, self.ad_features, check_indices=check_indices, _ready=True)
            logits = ctr.view(1, -1)
        else:
            tasks, logits = rk.score_candidates(uc, un, cand_pos, self.ad_features,                   # :241-255
                                                check_indices=check_indices, raw=True)
        if mark is not None:                     # amdrec.sharded.StageTimer: the ranker ends here, the selection follows
            mark("ranker")
        if out is not None:                      # (ad_ids, scores) views of one block: the reference API's single D2H copy
            ad_ids, scores = out[0], out[1]      # (under the auction the block also holds ecpm and prices: out[2], out[3])
        else:
            ad_ids = torch.empty((B, top_k), dtype=torch.int64, device=uc.device)
            scores = torch.empty((len(tasks), B, top_k), dtype=torch.float32, device=uc.device)
        idx = self.faiss_index
        if ids_are_positions:
            cand_ids = cand_pos
        elif idx._identity:
            # (else every slot is filled)
            unfilled = idx._n and (stage1_k > idx._n or idx.index_type in ("IVF", "IVFPQ") or excluded)
            # an unfilled slot (-1) reads id_map[-1] like the reference's list indexing (faiss_retrieval.py:159-160): one
            # launch (Python-style remainder: -1 -> n - 1, valid positions unchanged) instead of compare + add + where
            cand_ids = torch.remainder(cand_pos, idx._n) if unfilled else cand_pos
        else:
            cand_ids = torch.empty_like(cand_pos)
            _lib.check(lib.amdrec_remap_ids(_lib.ptr(cand_pos), _lib.ptr(idx._ids), idx._n, _lib.ptr(cand_ids),
                                            cand_pos.numel(), _lib.stream_ptr(uc.device)))
        # mid / tail: what an entry takes between top_k and out_ids / behind out_slots
        mid, ecpm, prices, values = (), None, None, None
        if head_weights is not None:
            # the value entries: the weights, (the bids and the reserve,) the groups in the middle, the values (and eCPMs and
            # prices) behind the slots; no rank_task in the plain one.  The cap (0: none) rides in the same launch
            w = _value.weights_tensor(head_weights, B, uc.device)
            groups = (_lib.ptr(idx._groups) if max_per_group else None, idx._n if max_per_group else 0, max_per_group or 0)
            values = out[2] if out is not None else torch.empty((B, top_k), dtype=torch.float32, device=uc.device)
            if auction is not None:
                reserve = _auction.reserve_tensor(_auction.check_reserve(auction[0], B), B, uc.device)
                if out is not None:
                    ecpm, prices = out[3], out[4]
                else:
                    ecpm = torch.empty((B, top_k), dtype=torch.float32, device=uc.device)
                    prices = torch.empty((B, top_k), dtype=torch.float32, device=uc.device)
                if B:
                    _lib.check(lib.amdrec_select_topk_value_auction(
                        _lib.ptr(logits), logits.stride(0), len(tasks), tasks.index("ctr"), _lib.ptr(cand_ids), _lib.ptr(cand_pos),
                        B, stage1_k, top_k, _lib.ptr(w), _lib.ptr(idx._bids), idx._n, _lib.ptr(reserve), *groups,
                        _lib.ptr(ad_ids), _lib.ptr(scores), None, _lib.ptr(values), _lib.ptr(ecpm), _lib.ptr(prices),
                        _lib.stream_ptr(uc.device)))
            elif B:
                _lib.check(lib.amdrec_select_topk_value(
                    _lib.ptr(logits), logits.stride(0), len(tasks), _lib.ptr(cand_ids), _lib.ptr(cand_pos), B, stage1_k, top_k,
                    _lib.ptr(w), *groups, _lib.ptr(ad_ids), _lib.ptr(scores), None, _lib.ptr(values),
                    _lib.stream_ptr(uc.device)))
            select = None
        elif auction is not None:
            # the auction entry: the selection's arguments with the bids, the reserve and the groups in the middle and two
            # outputs more; the cap (0: none) rides in the same launch
            select = lib.amdrec_select_topk_auction
            reserve = _auction.reserve_tensor(_auction.check_reserve(auction[0], B), B, uc.device)
            mid = (_lib.ptr(idx._bids), idx._n, _lib.ptr(reserve), _lib.ptr(idx._groups) if max_per_group else None,
                   idx._n if max_per_group else 0, max_per_group or 0)
            if out is not None and len(out) == 4:
                ecpm, prices = out[2], out[3]
            else:
                ecpm = torch.empty((B, top_k), dtype=torch.float32, device=uc.device)
                prices = torch.empty((B, top_k), dtype=torch.float32, device=uc.device)
            tail = (_lib.ptr(ecpm), _lib.ptr(prices))
        elif diversity is not None:
            # the diversified entry: the rows, lam, the pool and the groups in the middle, one output more; the cap (0: none)
            # rides in the same launch.  The rows are read from the index now: nothing is cached across corpus edits
            select = lib.amdrec_select_topk_diverse
            mid = (_lib.ptr(idx._xb), idx._n, idx._xb.stride(0), idx.dimension, diversity[0], diversity[1],
                   _lib.ptr(idx._groups) if max_per_group else None, idx._n if max_per_group else 0, max_per_group or 0)
            values = out[2] if out is not None and len(out) == 3 else \
                torch.empty((B, top_k), dtype=torch.float32, device=uc.device)
            tail = (_lib.ptr(values),)
        elif explore is not None:
            # the sampled entry: the capped one's arguments (cap 0: none), then the temperatures, the seeds, the prefix and one
            # output more
            select = lib.amdrec_select_topk_sampled
            values = out[2] if out is not None and len(out) == 3 else \
                torch.empty((B, top_k), dtype=torch.float32, device=uc.device)
            tail = (_lib.ptr(idx._groups) if max_per_group else None, idx._n if max_per_group else 0, max_per_group or 0,
                    _lib.ptr(explore[0]), _lib.ptr(explore[1]), explore[2], _lib.ptr(values))
        elif max_per_group is None:
            select, tail = lib.amdrec_select_topk, ()
        else:                                    # the same arguments, then the groups: the cap runs inside the selection
            select, tail = lib.amdrec_select_topk_capped, (_lib.ptr(idx._groups), idx._n, max_per_group)
        if select is None:
            pass                                 # (launched above)
        elif B and ctr_first:
            # the selection as ever, on the one logit row: ad ids, plane 0 of scores and the winning slots; then the winners'
            # other tasks into planes 1 ..
            slots = torch.empty((B, top_k), dtype=torch.int32, device=uc.device)
            _lib.check(select(_lib.ptr(logits), logits.stride(0), 1, 0, _lib.ptr(cand_ids), _lib.ptr(cand_pos),
                              B, stage1_k, top_k, *mid, _lib.ptr(ad_ids), _lib.ptr(scores), _lib.ptr(slots), *tail,
                              _lib.stream_ptr(uc.device)))
            rk.winner_scores(trunk, slots, stage1_k, scores)
        elif B:
            _lib.check(select(_lib.ptr(logits), logits.stride(0), len(tasks), tasks.index("ctr"),
                              _lib.ptr(cand_ids), _lib.ptr(cand_pos), B, stage1_k, top_k, *mid,
                              _lib.ptr(ad_ids), _lib.ptr(scores), None, *tail, _lib.stream_ptr(uc.device)))
        res = {"ad_ids": ad_ids, "scores": scores, "tasks": tasks, "candidate_ids": cand_ids, "logits": logits,
               "logit_tasks": ("ctr",) if ctr_first else tuple(tasks)}
        if auction is not None:
            res["ecpm"], res["prices"] = ecpm, prices
        if diversity is not None:
            res["diversity_values"] = values
        if head_weights is not None:
            res["values"] = values
        if explore is not None:
            res["propensities"] = values
        return res

    @torch.no_grad()
    def recommend_device(self, user_categorical: torch.Tensor, user_numerical: torch.Tensor, top_k: int = 10,
                         stage1_k: int = 500, check_indices: bool = False,
                         exclude_ad_ids: Optional[torch.Tensor] = None, heads: Optional[str] = None,
                         require_all: Optional[torch.Tensor] = None, require_any: Optional[torch.Tensor] = None,
                         max_per_group: Optional[int] = None, stage1_max_per_group: Optional[int] = None,
                         rank_by: Optional[str] = None, reserve=None, diversity: Optional[float] = None,
                         diversity_pool: int = 64, stage1_boost=None, head_weights=None,
                         include_ad_ids: Optional[torch.Tensor] = None, explore=None, explore_seed=None,
                         explore_from: int = 0):
        """[B,6] / [B,13] device tensors -> dict of device tensors, no host synchronisation:
        ad_ids [B,top_k] int64, scores [3,B,top_k] float32 (sigmoid of the logits), candidate_ids
        [B,stage1_k], candidate_scores [B,stage1_k], logits [3, B*stage1_k].  candidate_scores are the index's own
        scores: inner products (descending) for Flat / IVF, approximate squared L2 distances (ascending) for IVFPQ.
        ``heads``: "all" / "ctr_first" for this call (None: ``heads_mode``).  Where "ctr_first" runs, ``logits`` is
        [1, B*stage1_k], the CTR row alone; ``logit_tasks`` names the rows of ``logits`` (== ``tasks`` in "all" mode).
        Everything else - ad_ids, all of scores, the CTR logits - is bit-identical in both modes.
        ``exclude_ad_ids``: device int64 [B, E], per user the ad ids that must not be recommended (negative = padding;
        stage1_k + E <= AMDREC_MAX_K): stage 1 searches stage1_k + E and drops them on the device (FAISSIndex.search_device),
        so candidate_ids / candidate_scores and everything after them hold eligible ads only.
        ``require_all`` / ``require_any``: device int64 [B], per user the eligibility masks against the ads' tags
        (amdrec.eligible; Flat index): stage 1 is the exact top-stage1_k of the ads the user may be shown, however many
        are ineligible; a user with fewer eligible ads gets a short candidate list.  Both None: the plain search.
        Short candidate lists: stage 1 leaves a slot unfilled (position -1; candidate_scores -inf, +inf for IVFPQ) when
        stage1_k exceeds the corpus, with narrow IVF / IVFPQ probes, with a stored NaN row or a NaN query, after exclusions,
        under eligibility masks and after remove_ads.  Such a slot is not a candidate: it ranks after every real candidate (those with a NaN logit
        included) and is reported only where a user has fewer than top_k real candidates, as ad_ids == -1 with scores 0.0
        for every task - the same tail that top_k > stage1_k gives.  The real ads of a row are distinct and were all
        retrieved by stage 1.  candidate_ids keeps the search's convention for an unfilled slot (id_map[-1]) and its entry
        of logits is unspecified but finite (for finite weights and user features): mask them with candidate_scores.
        ``max_per_group`` (None: no cap, the launches of ever): at most that many of a user's ``top_k`` ads share one group
        key of the index (FAISSIndex.add(groups=) / set_groups; amdrec.group_cap has the rule: greedy in the selection's
        order, ungrouped ads never capped).  The cap runs inside the selection, on the device; a user whose candidates hold
        fewer than ``top_k`` ads that it lets through gets the -1 / 0.0 tail.  ``stage1_max_per_group``: the same rule on the
        candidate list (FAISSIndex.search_device(max_per_group=): the cap applied to the index's own top
        2 * stage1_k), so that one advertiser's near-duplicate creatives cannot fill the candidates; slots the cap
        leaves empty are unfilled slots as above.  Either on an index without group keys, or <= 0: ValueError.
        ``rank_by`` (None / "ctr": the CTR order, the launches of ever): "ecpm" ranks a user's candidates by bid x pCTR over
        the index's bids (FAISSIndex.add(bids=) / set_bids; amdrec.auction has the rule), inside the selection launch, with
        ``max_per_group`` applied in that order; the dict gains ``ecpm`` and ``prices``, float32 [B, top_k]: each winner's
        expected revenue and its generalised second price (0.0 in the unfilled tail).  ``reserve`` (needs "ecpm"): a Python
        float >= 0 for every user, or a device float32 [B]; candidates whose eCPM does not reach it are dropped and it is
        every price's floor.  "ecpm" on an index without bids, an unknown ``rank_by``, a reserve without "ecpm" and a
        negative or non-finite scalar reserve: ValueError.
        ``diversity`` (None: the selections above, the launches of ever): ``lam`` in [0, 1] re-orders the best
        ``diversity_pool`` accepted candidates greedily by pCTR x (1 - lam x the largest similarity to an ad already chosen),
        similarities being inner products of the index's own rows (amdrec.diversity has the rule; Flat and IVF), inside one
        selection launch, after ``max_per_group`` where that is given; the dict gains ``diversity_values``, float32 [B, top_k]:
        each winner's discounted value (0.0 in the unfilled tail).  ``lam == 0`` is the plain (or capped) result bit for bit.
        A non-number ``lam``: TypeError; ``lam`` outside [0, 1], a pool below ``top_k``, above 128 or with pool x dimension >
        32768, a pool without ``diversity``, and ``diversity`` with "ecpm": ValueError; on an IVFPQ index: NotImplementedError.
        ``stage1_boost`` (None: the plain search, the launches of ever): a number or a device float32 [B], the users' weights
        on the index's per-ad boosts (FAISSIndex.add(boosts=) / set_boosts; amdrec.boost has the rule; Flat index, or IVF with
        ``list_boosts``): stage 1 is the exact top-stage1_k under similarity + w x boost[ad], so an ad with a large bid
        (boost = beta x log(bid)) reaches the ranker - and the auction - from any similarity rank (on IVF: from any rank inside
        the probed lists); candidate_scores are the boosted scores.  Stage 2 never reads them and is unchanged.  On an index
        without boosts, a non-finite number: ValueError; on Flat with masks, on IVF without ``list_boosts``, on IVFPQ:
        NotImplementedError.
        ``head_weights`` (None: the CTR order, the launches of ever): stage 2 orders a user's candidates by the blend
        sum_t w_t x p_t of EVERY head's probability (amdrec.value has the rule), inside the selection launch: a dict by task
        name (a missing task is 0), a sequence of ``len(tasks)`` numbers in the ranker's task order, or a device float32
        [B, n_tasks] tensor of per-user weights (its values are the caller's).  ``max_per_group`` applies in that order; with
        ``rank_by="ecpm"`` the CTR term is bid x pCTR, ``reserve`` is compared with the value and ``prices`` is the smallest
        bid that keeps the rank under the blend.  The dict gains ``values``, float32 [B, top_k] (0.0 in the unfilled tail).
        The blend needs every head on every candidate: an instance whose ``heads_mode`` is "ctr_first" runs such a call on
        all heads (``logit_tasks`` says so).  One-hot CTR weights order by pCTR, which ties where sigmoids saturate: not
        the logit order of the plain call in general.  Bools, non-numbers, a tensor of another dtype or device: TypeError;
        non-finite or all-zero scalars, an unknown task, a wrong length or shape, under "ecpm" a scalar CTR weight <= 0,
        together with ``diversity`` or an explicit ``heads="ctr_first"``: ValueError.
        ``include_ad_ids`` (None or I = 0: the plain search, the launches of ever): device int64 [B, I <= min(stage1_k, 64)],
        per user the ad ids that must reach the ranker whatever their similarity rank (negative = padding): retargeting
        lists, guaranteed campaigns, cart items, freshly added ads, exploration slots.  Stage 1 merges every listed ad that
        is known, eligible under the masks, not excluded and not NaN-scored into its result at its exact (boosted) score,
        the lowest-ranked unlisted candidates making room (amdrec.include has the rule; Flat and IVF - on IVF also from an
        unprobed list); the dict gains ``candidate_injected``, bool [B, stage1_k], True where a candidate came from the
        list alone.  Stage 2 is unchanged: caps, auction, diversity, value ranking and "ctr_first" take the merged
        positions.  Wider than 64 or than stage1_k, or together with ``stage1_max_per_group`` (the order of cap and
        injection is undecided): ValueError; on an IVFPQ index: NotImplementedError.
        ``explore`` (None: the arg-max selections above, the launches of ever): the temperature of a sampled selection
        (amdrec.explore has the rule) - a number >= 0 for every user or a device float32 [B] of the caller's values; a user
        whose temperature is not > 0 is served greedily.  Stage 2 then draws the ``top_k`` ads without replacement with
        probabilities proportional to exp(CTR logit / temperature) (Plackett-Luce, by Gumbel-perturbed keys), inside the
        selection launch, under ``max_per_group`` where that is given and in either heads mode (bit-identical between them);
        the dict gains ``propensities``, float32 [B, top_k]: the conditional probability the policy gave each pick (1.0 for a
        forced pick, 0.0 in the unfilled tail; a pick of vanishing probability may read 0.0).  ``explore_seed`` (required
        with ``explore``): a Python int in [0, 2^64) - user ``u`` draws with ``(seed + u) mod 2^64`` - or a device int64 [B]
        of bit patterns; the noise is keyed on seed and ad id, so the same seed draws the same ads whatever the candidate
        order.  ``explore_from``: the first that many ranks stay the arg-max winners (propensity 1.0) and the draw fills the
        rest.  One without the other, ``explore_from`` without ``explore`` or outside [0, top_k], ``top_k`` > 128, a negative
        or non-finite temperature, a seed outside 64 bits, a wrong shape, together with "ecpm", ``reserve``,
        ``head_weights`` or ``diversity``: ValueError; bools, non-numbers, a tensor of another dtype or device: TypeError.
        ``check_indices``: an out-of-range user index or ad-table row raises IndexError; an unfilled slot does not."""
        if heads is not None:
            self._check_heads(heads)
        listed = self._check_include(include_ad_ids, stage1_k, stage1_max_per_group)
        self.faiss_index._check_boost(stage1_boost, require_all is not None or require_any is not None)
        cap, cap1 = self._check_caps(max_per_group, stage1_max_per_group)          # (before the library is touched)
        auction = self._check_auction(rank_by, reserve)
        div = self._check_diversity(diversity, diversity_pool, top_k, auction)
        hw = self._check_head_weights(head_weights, None if user_categorical is None else user_categorical.shape[0], auction,
                                      diversity, heads)
        ex = _explore.check_explore(explore, explore_seed, explore_from, top_k,
                                    None if user_categorical is None else user_categorical.shape[0], auction is not None,
                                    head_weights is not None, diversity is not None)
        uc = _lib.require_gpu(user_categorical, "user_categorical")
        un = _lib.require_gpu(user_numerical, "user_numerical")
        if ex is not None:
            ex = (_explore.temperature_tensor(ex.temperature, uc.shape[0], uc.device),
                  _explore.seed_tensor(ex.seed, uc.shape[0], uc.device), ex.greedy)
        excluded = exclude_ad_ids is not None and exclude_ad_ids.shape[-1] > 0
        masked = require_all is not None or require_any is not None
        # one calling thread at a time enqueues (amdrec._lib.Gate): the launches below hand their intermediate results to
        # each other through the process-wide workspace, and the lazily built state is built in here
        with _lib.GATE.serving(), _lib.GATE.enqueue:
            cand_pos, cand_scores, *injected = self._stage1(uc, un, stage1_k, check_indices, exclude_ad_ids if excluded else None,
                                                            (require_all, require_any), cap1, stage1_boost,
                                                            include_ad_ids if listed else None)
            # (excluded: "a slot can be unfilled" - true after a filtered stage 1 as well)
            out = self._stage2(uc, un, cand_pos, top_k, check_indices, excluded=excluded or masked or cap1 is not None,
                               heads=heads, max_per_group=cap, auction=auction, diversity=div, head_weights=hw, explore=ex)
        out["candidate_scores"] = cand_scores
        if injected:
            out["candidate_injected"] = injected[0]
        return out

    def _check_include(self, include, stage1_k, stage1_max_per_group) -> bool:
        """Was an include list passed (a block [B, I] with I > 0)?  Refused before the library is touched, as
        FAISSIndex.search_device refuses it: a list wider than 64 or than stage1_k, a list together with the stage-1 cap,
        a list on an IVFPQ index."""
        if include is None or include.shape[-1] == 0:
            return False
        _include.check_include(stage1_k, include.shape[-1])
        if stage1_max_per_group is not None:
            raise ValueError(_include.CAP_ORDER)
        if self.faiss_index.index_type == "IVFPQ":
            raise NotImplementedError(_include.IVFPQ)
        return True

    def capture(self, batch_size: int, top_k: int = 10, stage1_k: int = 500, warmup: int = 2,
                max_exclude: int = 0, eligibility: bool = False, max_per_group: Optional[int] = None,
                stage1_max_per_group: Optional[int] = None, rank_by: Optional[str] = None,
                reserve: bool = False, diversity: Optional[float] = None,
                diversity_pool: int = 64, stage1_boost: bool = False, head_weights: bool = False,
                max_include: int = 0, explore: bool = False, explore_from: int = 0) -> "GraphedRecommender":
        """Capture one recommend_device call for a fixed batch shape into a HIP graph (the ~40 kernel
        launches of a request are host-launch-bound at small batch: 1.76 ms eager at B = 1) and return a
        replayer.  Weights, index and ad table must not change afterwards.  ``max_exclude`` > 0: the graph also holds a
        static [batch_size, max_exclude] exclusion buffer (stage 1 always searches stage1_k + max_exclude) that the
        replayer's ``exclude`` argument fills; 0 captures the graph without the exclusion step.  ``eligibility``: the graph
        holds static [batch_size] mask buffers and runs the filtered search (the replayer's ``require_all`` /
        ``require_any`` fill them; the tags are those of capture time); False captures the graph as ever.
        ``max_per_group`` / ``stage1_max_per_group`` (recommend_device): scalars fixed at capture; the group keys are those
        of capture time.  ``rank_by`` (recommend_device) is fixed at capture too, and the bids are those of capture time;
        ``reserve=True`` (needs "ecpm") gives the graph a static [batch_size] float32 reserve buffer that the replayer's
        ``reserve`` argument fills.  ``diversity`` / ``diversity_pool`` (recommend_device): scalars fixed at capture, like
        ``max_per_group``; the rows are those of capture time.  ``stage1_boost=True``: the graph holds a static
        [batch_size] float32 weight buffer and runs the boosted search (the replayer's ``stage1_boost`` fills it, zeros
        without one; the boosts are those of capture time); False captures the graph as ever.  ``head_weights=True``: the
        graph holds a static [batch_size, n_tasks] float32 weight buffer and runs the value selection of recommend_device
        (the replayer's ``head_weights`` fills it; until then, and without one, it holds 1.0 for the CTR head and 0.0 for the
        others); False captures the graph as ever.  ``max_include`` > 0: the graph also holds a static
        [batch_size, max_include] include buffer (-1 = padding until filled) and the merge step of recommend_device's
        ``include_ad_ids``, which the replayer's ``include`` argument fills; the id table is that of capture time; 0
        captures the graph as ever.  ``explore=True``: the graph runs the sampled selection of recommend_device with the
        greedy prefix ``explore_from`` (a scalar fixed at capture) and holds static [batch_size] temperature and seed buffers
        that the replayer's ``explore`` / ``explore_seed`` fill (zeros until then: every user is served greedily); a replay
        without them redraws with the buffers as they stand - the same seeds, hence the same draw for the same candidates.
        False captures the graph as ever."""
        return GraphedRecommender(self, batch_size, top_k, stage1_k, warmup, max_exclude, eligibility, max_per_group,
                                  stage1_max_per_group, rank_by, reserve, diversity, diversity_pool, stage1_boost, head_weights,
                                  max_include, explore, explore_from)

    # -- live corpus: ads leave and enter without a rebuild of the index or of the ranker's per-ad caches ------------------
    def remove_ads(self, ad_ids) -> int:
        """Retire every ad whose id is in ``ad_ids`` -> the number of ads removed.  The index drops their rows
        (FAISSIndex.remove_ids has the contract), the ad-feature table becomes its gather by the rows that stay, and the
        ranker's per-ad caches are moved along bit for bit (TransformerRanker.compact_ad_cache): bytes move, nothing is
        projected again.  Rows of the table beyond the index's old ntotal (a table longer than the corpus) are dropped.
        Out of place throughout: a graph captured before the call keeps replaying the corpus it was captured with (stale,
        consistent); capture again to serve the new one.  Synchronises with the host once (the survivor count)."""
        with _lib.GATE.enqueue:                  # (index, table and caches change together under a serving thread's feet)
            removed, kept = self.faiss_index.remove_ids(ad_ids, return_kept=True)
            if not removed:
                return 0
            old = self.ad_features
            new = _rows_edit.gather_rows(old, kept)
            self.transformer_ranker.compact_ad_cache(old, kept, new)
            self._swap_ad_table(old, new)
            return removed

    def add_ads(self, embeddings, ad_features, ad_ids=None, tags=None, groups=None, bids=None, boosts=None) -> None:
        """Insert ads: ``embeddings`` [m, d] go to the index (FAISSIndex.add: ``ad_ids`` as there; required once ads have been
        removed; ``tags``: the ads' 64-bit eligibility words, ``groups``: their int64 group keys, ``bids``: their float32 bids, ``boosts``: their stage-1 score boosts, as there), ``ad_features`` [m, n_ad_feat] integer rows are
        appended to the ad-feature table, and the ranker's per-ad
        caches grow by projecting the m new rows only (TransformerRanker.extend_ad_cache).  The feature rows are checked
        against the ranker's ad embedding tables first (IndexError, as an embedding lookup would raise), and a rejected call
        - bad features, or ids the index refuses - leaves index, table and caches as they were.  Out of place, as
        remove_ads.  A table that was longer than the corpus is cut to it first (the new rows' positions follow the
        corpus), and the caches are then rebuilt lazily instead of extended."""
        idx = self.faiss_index
        feats = ad_features if isinstance(ad_features, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ad_features))
        if feats.is_floating_point() or feats.dtype == torch.bool:
            raise TypeError(f"ad_features must be integers, got {feats.dtype}")
        feats = feats.to(device=self.device, dtype=torch.int64).contiguous()
        old = self.ad_features
        if feats.dim() != 2 or feats.shape[1] != old.shape[1] or feats.shape[0] != len(embeddings):
            raise ValueError(f"ad_features must be [{len(embeddings)}, {old.shape[1]}], got {tuple(feats.shape)}")
        cards = torch.tensor([e.weight.shape[0] for e in self.transformer_ranker.ad_embeddings.values()],
                             dtype=torch.int64, device=self.device)
        if feats.numel() and bool(((feats < 0) | (feats >= cards)).any().item()):
            raise IndexError("index out of range in self: an ad_features row is outside the ranker's ad embedding tables")
        with _lib.GATE.enqueue:
            old = self.ad_features
            n_old = idx.index.ntotal
            idx.add(embeddings, ad_ids, tags=tags, groups=groups, bids=bids, boosts=boosts)   # (refuses before it commits anything)
            new = torch.cat([old[:n_old], feats])
            if old.shape[0] == n_old:
                self.transformer_ranker.extend_ad_cache(old, new)
            self._swap_ad_table(old, new)

    def _swap_ad_table(self, old, new):
        """Install ``new`` as the ad-feature table.  A "valid" verdict of the once-per-table check (_ad_table_valid) is
        carried over: rows gathered from a valid table are valid, and add_ads has checked what it appended."""
        c = self.__dict__.get("_ad_ok")
        self.ad_features = new
        if c is not None and c[0][2] is old and c[0][3] == old._version and c[0][0] == _lib._REG_EPOCH[0] and \
                c[0][1] is self.transformer_ranker and c[1]:
            self.__dict__["_ad_ok"] = ((c[0][0], c[0][1], new, new._version), c[1])

    # -- reference API ------------------------------------------------------------------------
    def recommend_ads(self, user_data: dict, top_k: int = 10, stage1_k: int = 500,
                      return_scores: bool = True, exclude_ad_ids=None, require_all: int = 0, require_any: int = 0,
                      max_per_group: Optional[int] = None, stage1_max_per_group: Optional[int] = None,
                      rank_by: Optional[str] = None, reserve=None, diversity: Optional[float] = None,
                      diversity_pool: int = 64, stage1_boost=None, head_weights=None, include_ad_ids=None, explore=None,
                      explore_seed=None, explore_from: int = 0) -> dict:
        """inference.py:199-288.  ``exclude_ad_ids``: the ad ids this user must not be shown (a sequence of integers).
        ``require_all`` / ``require_any``: this request's eligibility masks (64-bit integers; 0 and 0: no constraint, the
        plain search).  ``max_per_group`` / ``stage1_max_per_group``: the per-group caps of recommend_device.  ``rank_by`` /
        ``reserve``: the auction of recommend_device (the dict gains ``ecpm`` and ``prices``).  ``diversity`` /
        ``diversity_pool``: its diversified selection (the dict gains ``diversity_values``).  ``stage1_boost``: this request's
        weight on the per-ad boosts in stage 1 (a number; recommend_device).  ``head_weights``: the value ranking of
        recommend_device, a dict by task name or a sequence of numbers (the dict gains ``values``).  ``include_ad_ids``: the
        ad ids that must reach the ranker for this user whatever their similarity rank (a sequence of integers;
        recommend_device).  ``explore`` / ``explore_seed`` / ``explore_from``: the sampled selection of recommend_device for
        this request - a temperature, a seed in [0, 2^64), the greedy prefix; the dict gains a ``"propensities"`` list: log
        it with the impression.  Fewer than ``top_k`` real candidates: as batch_recommend."""
        masked = bool(require_all) or bool(require_any)
        return self.batch_recommend([user_data], top_k=top_k, stage1_k=stage1_k, return_scores=return_scores,
                                    exclude_ad_ids=None if exclude_ad_ids is None else [exclude_ad_ids],
                                    require_all=[require_all] if masked else None,
                                    require_any=[require_any] if masked else None, max_per_group=max_per_group,
                                    stage1_max_per_group=stage1_max_per_group, rank_by=rank_by, reserve=reserve,
                                    diversity=diversity, diversity_pool=diversity_pool, stage1_boost=stage1_boost,
                                    head_weights=head_weights,
                                    include_ad_ids=None if include_ad_ids is None else [include_ad_ids], explore=explore,
                                    explore_seed=explore_seed, explore_from=explore_from)[0]

    def batch_recommend(self, user_data_list: list, top_k: int = 10, stage1_k: int = 500,
                        return_scores: bool = True, exclude_ad_ids=None, require_all=None, require_any=None,
                        max_per_group: Optional[int] = None, stage1_max_per_group: Optional[int] = None,
                        rank_by: Optional[str] = None, reserve=None, diversity: Optional[float] = None,
                        diversity_pool: int = 64, stage1_boost=None, head_weights=None, include_ad_ids=None, explore=None,
                        explore_seed=None, explore_from: int = 0) -> list:
        """inference.py:290-331 - but one device pass for the whole list instead of a serial loop.
        ``timing`` reports the batch's stage times divided by the number of users.  ``exclude_ad_ids``: one sequence of
        ad ids per user (recommend_device has the meaning); the padded block travels in the input staging block.
        ``require_all`` / ``require_any``: one 64-bit eligibility mask per user each (one int for all, a sequence, a uint64 /
        int64 array; where one is given the other defaults to 0), in the same staging block: no synchronisation more.
        ``ad_ids`` and every list of ``scores`` always have length ``top_k``: where stage 1 retrieved fewer than ``top_k``
        ads for a user (a corpus smaller than top_k, exclusions, narrow probes, a NaN feature) the tail reads ad id -1
        with score 0.0 for every task, and no ad appears that stage 1 did not retrieve for that user.
        ``max_per_group`` / ``stage1_max_per_group``: the per-group caps of recommend_device, for every user of the list (a
        user with fewer than ``top_k`` ads that the cap lets through gets the same tail).  ``rank_by`` / ``reserve``: the
        auction of recommend_device; every user's dict gains ``"ecpm"`` and ``"prices"`` lists of length ``top_k``, which travel
        in the same result block: no copy and no synchronisation more.  ``diversity`` / ``diversity_pool``: the diversified
        selection of recommend_device; every user's dict gains a ``"diversity_values"`` list of length ``top_k``, in the same
        block.  ``stage1_boost``: the stage-1 boost weight of recommend_device, one number for every user or a sequence of
        one per user; the weights travel in the input staging block: no copy and no synchronisation more.
        ``head_weights``: the value ranking of recommend_device, for every user of the list; every user's dict gains a
        ``"values"`` list of length ``top_k``, in the same result block.  ``include_ad_ids``: one sequence of ad ids per user
        (or an integer array [n, I], negative = padding) that must reach the ranker (recommend_device); the padded block
        travels through pinned memory like the exclusions: no synchronisation more.  ``explore`` / ``explore_seed`` /
        ``explore_from``: the sampled selection of recommend_device - one temperature for every user or a sequence of one per
        user, one seed (user ``u`` of the list draws with ``(seed + u) mod 2^64``) or a sequence of one per user; both travel in
        the input staging block, and every user's dict gains a ``"propensities"`` list of length ``top_k``, in the same
        result block: no copy and no synchronisation more."""
        incl = self._host_inclusions(include_ad_ids, len(user_data_list), stage1_k, stage1_max_per_group)
        self.faiss_index._check_boost(stage1_boost, require_all is not None or require_any is not None)
        self._check_caps(max_per_group, stage1_max_per_group)
        auction = self._check_auction(rank_by, reserve)
        self._check_diversity(diversity, diversity_pool, top_k, auction)
        self._check_head_weights(head_weights, len(user_data_list) or None, auction, diversity)
        ex = _explore.check_explore(explore, explore_seed, explore_from, top_k, len(user_data_list) or None, auction is not None,
                                    head_weights is not None, diversity is not None, per_user=True)
        if not user_data_list:
            return []
        n = len(user_data_list)
        excl = self._host_exclusions(exclude_ad_ids, n, stage1_k)
        masks = self._host_masks(require_all, require_any, n)
        wts = None if stage1_boost is None else _boost.as_weights(stage1_boost, n)
        draws = None if ex is None else _explore.host_arrays(ex, n)
        with _lib.GATE.serving():
            uc, un, *rest = self.preprocess_batch(user_data_list, excl, masks, wts, draws)
            excl = rest.pop(0) if excl is not None else None
            masks = rest.pop(0) if masks is not None else None
            wts = rest.pop(0) if wts is not None else None
            kw = {}
            if draws is not None:                # (the device views of the staged temperatures and seeds: checked above)
                kw = dict(explore=rest[0], explore_seed=rest[1], explore_from=ex.greedy)
            return self.recommend_tensors(uc, un, top_k, stage1_k, return_scores, _encoded=True, _exclude_dev=excl,
                                          _masks_dev=masks, _boost_dev=wts, max_per_group=max_per_group,
                                          stage1_max_per_group=stage1_max_per_group, rank_by=rank_by, reserve=reserve,
                                          diversity=diversity, diversity_pool=diversity_pool, head_weights=head_weights,
                                          _include_host=incl, **kw)

    def _check_caps(self, max_per_group, stage1_max_per_group):
        """The two cap arguments -> (cap or None, stage-1 cap or None); refusals before the library is touched."""
        idx = self.faiss_index
        return idx._check_group_cap(max_per_group), idx._check_group_cap(stage1_max_per_group, "stage1_max_per_group")

    def _check_auction(self, rank_by, reserve):
        """The ``rank_by`` / ``reserve`` arguments -> None (rank by CTR) or ``(reserve or None,)``; refusals before the library
        is touched (FAISSIndex._check_auction)."""
        auction, reserve = self.faiss_index._check_auction(rank_by, reserve)
        return (reserve,) if auction else None

    def _check_diversity(self, diversity, diversity_pool, top_k, auction):
        """The ``diversity`` / ``diversity_pool`` arguments -> None (today's selection) or ``(lam, pool)``; refusals before the
        library is touched (amdrec.diversity.check_diversity).  ``auction``: _check_auction's result."""
        return _diversity.check_index_diversity(self.faiss_index, diversity, diversity_pool, top_k, auction is not None)

    def _check_head_weights(self, head_weights, n_users, auction, diversity, heads=None):
        """The ``head_weights`` argument -> None (today's selections) or amdrec.value.check_head_weights' result; refusals before
        the library is touched.  ``auction``: _check_auction's result; ``diversity``: the caller's argument."""
        if head_weights is None:
            return None
        return _value.check_head_weights(head_weights, self.transformer_ranker.prediction_heads.keys(), n_users,
                                         auction is not None, diversity is not None, heads)

    def _host_masks(self, require_all, require_any, n: int) -> Optional[np.ndarray]:
        """The two mask arguments of the reference-API calls -> int64 [2, n] on the host (None: neither given)."""
        if require_all is None and require_any is None:
            return None
        self.faiss_index._check_masks(require_all, require_any)
        return np.stack([_eligible.as_words(0 if require_all is None else require_all, n),
                         _eligible.as_words(0 if require_any is None else require_any, n)])

    @staticmethod
    def _host_exclusions(exclude_ad_ids, n: int, stage1_k: int) -> Optional[np.ndarray]:
        """One id list per user -> the padded int64 [n, E] host block (None: no list, or every list empty)."""
        blk = _exclude.as_block(exclude_ad_ids, n)
        if blk is not None:
            _exclude.check_exclude(stage1_k, blk.shape[1])
        return blk

    def _host_inclusions(self, include_ad_ids, n: int, stage1_k: int, stage1_max_per_group=None) -> Optional[np.ndarray]:
        """One id list per user -> the padded int64 [n, I] host block (None: no list, or every list empty); refused as
        recommend_device refuses it, before the library is touched."""
        blk = _include.as_block(include_ad_ids, n)
        if blk is not None:
            self._check_include(blk, stage1_k, stage1_max_per_group)
        return blk

    def _user_limits(self):
        """Per user column, the number of rows of the SMALLER of the tower's and the ranker's embedding tables: an index is
        valid iff it is below it (torch raises IndexError otherwise, two_tower_model.py:44 / transformer_ranker.py:318)."""
        key = (_lib._REG_EPOCH[0], self.two_tower_model, self.transformer_ranker)
        c = self.__dict__.get("_limits")
        if c is None or c[0][0] != key[0] or c[0][1] is not key[1] or c[0][2] is not key[2]:
            tw = self.two_tower_model.user_tower.embedding_layer.embeddings
            rk = self.transformer_ranker.user_embeddings
            lim = [min(tw[n].weight.shape[0], rk[n].weight.shape[0]) for n in tw.keys()]
            c = self.__dict__["_limits"] = (key, lim, torch.tensor(lim, dtype=torch.int64, device=self.device))
        return c[1], c[2]

    def _encoder_fits(self) -> bool:
        """True when every index the preprocessor can produce is inside the models' tables: the dict API then needs no
        per-request index check (the label encoder's output is its own class count at most)."""
        pp = self.preprocessor
        lim, _ = self._user_limits()
        c = self.__dict__.get("_enc_fit")
        if c is None or c[0] is not pp or c[1] != lim:                    # (the object itself is kept: an id can be reused)
            cols = [c_ for c_ in USER_COLS if c_ in pp.classes]
            ok = len(cols) == len(lim) and all(len(pp.classes[c_]) <= m for c_, m in zip(cols, lim))
            c = self.__dict__["_enc_fit"] = (pp, list(lim), ok)
        return c[2]

    def _ad_table_valid(self) -> bool:
        """The resident ad-feature table against the ranker's ad embedding tables, checked ONCE per table / model (one
        reduction + host read), not per request: round 3 re-validated all N x 20 indices inside every checked request."""
        t = self.ad_features
        key = (_lib._REG_EPOCH[0], self.transformer_ranker, t, t._version)
        c = self.__dict__.get("_ad_ok")
        if c is None or c[0][0] != key[0] or c[0][1] is not key[1] or c[0][2] is not key[2] or c[0][3] != key[3]:
            cards = torch.tensor([e.weight.shape[0] for e in self.transformer_ranker.ad_embeddings.values()],
                                 dtype=torch.int64, device=t.device)
            ok = t.numel() == 0 or not bool(((t < 0) | (t >= cards)).any().item())
            c = self.__dict__["_ad_ok"] = (key, ok)
        return c[1]

    @torch.no_grad()
    def recommend_tensors(self, user_categorical, user_numerical, top_k=10, stage1_k=500, return_scores=True,
                          _encoded=False, exclude_ad_ids=None, _exclude_dev=None, require_all=None, require_any=None,
                          _masks_dev=None, max_per_group=None, stage1_max_per_group=None, rank_by=None, reserve=None,
                          diversity=None, diversity_pool=64, stage1_boost=None, _boost_dev=None, head_weights=None,
                          include_ad_ids=None, _include_host=None, explore=None, explore_seed=None, explore_from=0):
        """Tensor-level entry (cf. TwoStageRetriever.retrieve_and_rank, faiss_retrieval.py:283-369); result dicts follow
        inference.py:272-288.  ONE host synchronisation per call (round 3 had four: the tower's index flag, the stage-1
        timing sync, the ranker's index flag, the result copy - each exposing the launch work queued behind it): indices
        are validated without a read-back in the middle (the verdict travels with the results), the stage times come from
        events, ids + scores + verdict come back in one copy.  An out-of-range index raises IndexError like the reference's
        embedding lookup, before any result is returned.  ``exclude_ad_ids``: one sequence of ad ids per user, shipped as
        one padded block through pinned memory (no synchronisation of its own).  ``require_all`` / ``require_any``: the
        users' eligibility masks as in batch_recommend, shipped the same way.  The lists keep length ``top_k``, with
        -1 / 0.0 in the tail of a user with fewer real candidates (batch_recommend).  ``max_per_group`` /
        ``stage1_max_per_group``: the per-group caps of recommend_device.  ``rank_by`` / ``reserve``: its auction; ``ecpm`` and
        ``prices`` ride in the same result block and copy.  ``diversity`` / ``diversity_pool``: its diversified selection;
        ``diversity_values`` rides there too.  ``stage1_boost``: the users' stage-1 boost weights as in batch_recommend,
        shipped through pinned memory like the masks.  ``head_weights``: its value ranking; ``values`` rides in the result block
        too, behind ``ecpm`` and ``prices`` where the auction runs: still one copy, one synchronisation.
        ``include_ad_ids``: one sequence of ad ids per user that must reach the ranker (recommend_device), shipped as one
        padded block through pinned memory like the exclusions.  ``explore`` / ``explore_seed`` / ``explore_from``: its
        sampled selection - numbers, one number per user (shipped through pinned memory like the boost weights) or device
        tensors; ``propensities`` rides in the result block behind the scores: still one copy, one synchronisation."""
        hi = _include_host
        if hi is None and include_ad_ids is not None and user_categorical is not None:
            hi = self._host_inclusions(include_ad_ids, user_categorical.shape[0], stage1_k, stage1_max_per_group)
        if _boost_dev is None:
            self.faiss_index._check_boost(stage1_boost, require_all is not None or require_any is not None)
        cap, cap1 = self._check_caps(max_per_group, stage1_max_per_group)
        auction = self._check_auction(rank_by, reserve)
        div = self._check_diversity(diversity, diversity_pool, top_k, auction)
        head_w = self._check_head_weights(head_weights, None if user_categorical is None else user_categorical.shape[0], auction,
                                      diversity)
        ex = _explore.check_explore(explore, explore_seed, explore_from, top_k,
                                    None if user_categorical is None else user_categorical.shape[0], auction is not None,
                                    head_weights is not None, diversity is not None, per_user=True)
        t0 = time.time()
        with _lib.GATE.serving():
            # host side first, beside other threads' enqueues: the inputs' copies to the device (torch ops: they use no
            # workspace), the option blocks converted and written into staging blocks that are this thread's own
            dev = self.device
            uc = user_categorical.to(dev)
            un = user_numerical.to(dev)
            n = uc.shape[0]
            if not n:
                return []
            excl = _exclude_dev
            if excl is None and exclude_ad_ids is not None:
                hb = self._host_exclusions(exclude_ad_ids, n, stage1_k)
                if hb is not None:
                    host, done = self._staging(hb.size * 8, "excl")
                    host.numpy().view(np.int64).reshape(hb.shape)[:] = hb
                    excl = host.to(dev, non_blocking=True).view(torch.int64).view(hb.shape)
                    done.record(torch.cuda.current_stream(dev))
            masks = _masks_dev
            if masks is None:
                hm = self._host_masks(require_all, require_any, n)
                if hm is not None:
                    host, done = self._staging(hm.size * 8, "masks")
                    host.numpy().view(np.int64).reshape(hm.shape)[:] = hm
                    masks = host.to(dev, non_blocking=True).view(torch.int64).view(hm.shape)
                    done.record(torch.cuda.current_stream(dev))
            wts = _boost_dev
            if wts is None and stage1_boost is not None:
                hw = _boost.as_weights(stage1_boost, n)
                host, done = self._staging(hw.size * 4, "boost")
                host.numpy().view(np.float32)[:] = hw
                wts = host.to(dev, non_blocking=True).view(torch.float32)
                done.record(torch.cuda.current_stream(dev))
            incl = None
            if hi is not None:
                host, done = self._staging(hi.size * 8, "incl")
                host.numpy().view(np.int64).reshape(hi.shape)[:] = hi
                incl = host.to(dev, non_blocking=True).view(torch.int64).view(hi.shape)
                done.record(torch.cuda.current_stream(dev))
            draw = None
            if ex is not None:
                temp, seed = ex.temperature, ex.seed
                if isinstance(temp, np.ndarray) or isinstance(seed, np.ndarray):     # one per user: [seeds | temperatures], one copy
                    ht, hs = _explore.host_arrays(ex._replace(temperature=0.0 if isinstance(temp, torch.Tensor) else temp,
                                                              seed=0 if isinstance(seed, torch.Tensor) else seed), n)
                    host, done = self._staging(n * 12, "explore")
                    host.numpy()[:n * 8].view(np.uint64)[:] = hs
                    host.numpy()[n * 8:].view(np.float32)[:] = ht
                    blk_e = host.to(dev, non_blocking=True)
                    done.record(torch.cuda.current_stream(dev))
                    temp = temp if isinstance(temp, torch.Tensor) else blk_e[n * 8:].view(torch.float32)
                    seed = seed if isinstance(seed, torch.Tensor) else blk_e[:n * 8].view(torch.int64)
                draw = (_explore.temperature_tensor(temp, n, dev), _explore.seed_tensor(seed, n, dev), ex.greedy)
            # the enqueue, one calling thread at a time (amdrec._lib.Gate); the wait for the device and the list conversion
            # behind it run beside other threads' enqueues, on staging blocks and events that are this thread's own
            with _lib.GATE.enqueue:
                tasks = list(self.transformer_ranker.prediction_heads.keys())        # the ranker's task order (= out["tasks"])
                tl = self._per_thread()                                          # the timing events are the calling thread's own
                ev = getattr(tl, "ev", None)
                if ev is None:
                    ev = tl.ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ids_b, sc_b = n * top_k * 8, len(tasks) * n * top_k * 4
                au_b = 0 if auction is None else n * top_k * 4                       # ecpm, then prices, behind the scores
                dv_b = 0 if div is None else n * top_k * 4                           # diversity_values, there instead (never both)
                va_b = 0 if head_w is None else n * top_k * 4                            # values, behind all of them (never with dv_b)
                pr_b = 0 if draw is None else n * top_k * 4                          # propensities, behind the scores (alone there)
                end_b = ids_b + sc_b + 2 * au_b + dv_b + va_b + pr_b
                blk = torch.empty(end_b + 8, dtype=torch.uint8, device=dev)
                ad_ids = blk[:ids_b].view(torch.int64).view(n, top_k)
                scores = blk[ids_b:ids_b + sc_b].view(torch.float32).view(len(tasks), n, top_k)
                outs = (ad_ids, scores)
                if head_w is not None:                                               # (_stage2 takes out[2] = values, then ecpm, prices)
                    outs += (blk[end_b - va_b:end_b].view(torch.float32).view(n, top_k),)
                if auction is not None:
                    outs += tuple(blk[ids_b + sc_b + i * au_b:ids_b + sc_b + (i + 1) * au_b].view(torch.float32).view(n, top_k)
                                  for i in range(2))
                if div is not None:
                    outs += (blk[ids_b + sc_b:ids_b + sc_b + dv_b].view(torch.float32).view(n, top_k),)
                if draw is not None:
                    outs += (blk[ids_b + sc_b:ids_b + sc_b + pr_b].view(torch.float32).view(n, top_k),)
                verdict = blk[end_b:].view(torch.int32)                              # [2]: nonzero = an index out of range
                trusted = _encoded and self.preprocessor is not None and self._encoder_fits()
                if trusted:
                    verdict.zero_()
                else:
                    if uc.dim() != 2 or uc.shape[1] != len(self._user_limits()[0]):
                        raise ValueError(f"user_categorical must be [B, {len(self._user_limits()[0])}]")
                    ucl = uc.long()
                    verdict.copy_(((ucl < 0) | (ucl >= self._user_limits()[1])).any().to(torch.int32).expand(2))
                if not self._ad_table_valid():
                    raise IndexError("index out of range in self")                    # (the ad-feature table, transformer_ranker.py:322)
                st = torch.cuda.current_stream(dev)
                ev[0].record(st)
                cand_pos, *_ = self._stage1(uc, un, stage1_k, False, excl,
                                            (None, None) if masks is None else (masks[0], masks[1]), cap1, wts, incl)
                ev[1].record(st)
                out = self._stage2(uc, un, cand_pos, top_k, False, out=outs,
                                   excluded=excl is not None or masks is not None or cap1 is not None, max_per_group=cap,
                                   auction=auction, diversity=div, head_weights=head_w, explore=draw)
                assert list(out["tasks"]) == tasks
                host, done = self._staging(blk.numel(), "out")
                host.copy_(blk, non_blocking=True)
                ev[2].record(st)
                done.record(st)
            ev[2].synchronize()
            hv = host.numpy()
            if int(hv[end_b:].view(np.int32)[0]):
                raise IndexError("index out of range in self")                    # torch.nn.Embedding's message
            ids = hv[:ids_b].view(np.int64).reshape(n, top_k).tolist()
            sc = hv[ids_b:ids_b + sc_b].view(np.float32).reshape(len(tasks), n, top_k).tolist() if return_scores else None
            au = None if auction is None else hv[ids_b + sc_b:ids_b + sc_b + 2 * au_b].view(np.float32).reshape(2, n, top_k).tolist()
            dv = None if div is None else hv[ids_b + sc_b:ids_b + sc_b + dv_b].view(np.float32).reshape(n, top_k).tolist()
            va = None if head_w is None else hv[end_b - va_b:end_b].view(np.float32).reshape(n, top_k).tolist()
            pr = None if draw is None else hv[ids_b + sc_b:ids_b + sc_b + pr_b].view(np.float32).reshape(n, top_k).tolist()
            t2 = time.time()
            # stage 1 = its GPU time (tower + search, as the reference brackets them); stage 2 = the rest of the call's wall time
            # (ranker, selection, the copy back and the list conversion: what the reference's second bracket holds)
            total_ms = (t2 - t0) * 1000 / n
            stage1_ms = min(ev[0].elapsed_time(ev[1]) / n, total_ms)
            res = []
            for b in range(n):
                r = {"ad_ids": ids[b],
                     "timing": {"stage1_ms": stage1_ms, "stage2_ms": total_ms - stage1_ms, "total_ms": total_ms}}
                if return_scores:
                    r["scores"] = {t: sc[i][b] for i, t in enumerate(tasks)}
                if au is not None:
                    r["ecpm"], r["prices"] = au[0][b], au[1][b]
                if dv is not None:
                    r["diversity_values"] = dv[b]
                if va is not None:
                    r["values"] = va[b]
                if pr is not None:
                    r["propensities"] = pr[b]
                res.append(r)
            return res


class TwoStageRetriever:
    """Drop-in for faiss_retrieval.py:259-369: the reference's second caller of the same path, taking tensors
    instead of dicts.  ``retrieve_and_rank`` keeps the reference's signature and tuple-of-lists return.
    ``ad_features_lookup``: None -> stage 1 only, returns (candidate ids, distances) exactly like the reference
    (:329-331); otherwise the ``[N, n_ad_feat]`` integer table of ad features indexed by corpus position (the
    reference collects per-id dicts and then scores all-zero placeholders, :338-345 - a documented stub)."""

    def __init__(self, two_tower_model: TwoTowerModel, transformer_ranker: TransformerRanker, faiss_index: FAISSIndex,
                 device: str = "cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AmdrecError("TwoStageRetriever needs a HIP device (no CPU fallback)")
        self.two_tower_model = two_tower_model.to(self.device).eval()
        self.transformer_ranker = transformer_ranker.to(self.device).eval()
        self.faiss_index = faiss_index
        self._rec = None

    @torch.no_grad()
    def retrieve_and_rank(self, user_categorical: torch.Tensor, user_numerical: torch.Tensor, stage1_k: int = 500,
                          stage2_k: int = 10, ad_features_lookup=None, exclude_ad_ids=None,
                          max_per_group: Optional[int] = None, stage1_max_per_group: Optional[int] = None,
                          rank_by: Optional[str] = None, reserve=None, diversity: Optional[float] = None,
                          diversity_pool: int = 64, stage1_boost=None, head_weights=None, include_ad_ids=None, explore=None,
                          explore_seed=None, explore_from: int = 0):
        """``exclude_ad_ids``: the ad ids the (first) user must not be shown, a sequence of integers.  With a table, the two
        lists have length ``stage2_k``; a user with fewer real candidates gets -1 / 0.0 in the tail (batch_recommend).
        ``stage1_max_per_group`` / ``max_per_group``: the per-group caps on the candidates and on the ranked result
        (AdRecommenderInference.recommend_device); without a table only the first applies (there is no stage 2).
        ``rank_by`` / ``reserve``: the auction of recommend_device for the ranked result (the tuple is as ever: ids and CTR
        probabilities, in eCPM order); without a table they are checked and change nothing.  ``diversity`` /
        ``diversity_pool``: the diversified selection of recommend_device for the ranked result (ids and CTR probabilities, in
        pick order); without a table they are checked and change nothing.  ``stage1_boost``: the (first) user's weight on the
        per-ad boosts in stage 1, a number (recommend_device), with or without a table.  ``head_weights``: the value ranking
        of recommend_device for the ranked result (ids and CTR probabilities, in value order); without a table it is checked
        and changes nothing.  ``include_ad_ids``: the ad ids that must be candidates for the (first) user whatever their
        similarity rank, a sequence of integers (recommend_device), with or without a table.  ``explore`` / ``explore_seed`` /
        ``explore_from``: the sampled selection of recommend_device for the ranked result, a temperature, a seed and the
        greedy prefix (ids and CTR probabilities, in pick order; the tuple carries no propensities - a caller that logs them
        uses recommend_ads); without a table they are checked and change nothing."""
        idx = self.faiss_index
        incl = None if include_ad_ids is None else _include.as_block([include_ad_ids], 1)
        if incl is not None:                                                      # (refused before the library is touched)
            _include.check_include(stage1_k, incl.shape[1])
            if stage1_max_per_group is not None:
                raise ValueError(_include.CAP_ORDER)
            if idx.index_type == "IVFPQ":
                raise NotImplementedError(_include.IVFPQ)
        idx._check_boost(stage1_boost)
        cap, cap1 = idx._check_group_cap(max_per_group), idx._check_group_cap(stage1_max_per_group, "stage1_max_per_group")
        auction = idx._check_auction(rank_by, reserve)[0]
        _diversity.check_index_diversity(idx, diversity, diversity_pool, stage2_k, auction)
        if head_weights is not None:
            _value.check_head_weights(head_weights, self.transformer_ranker.prediction_heads.keys(), None, auction,
                                      diversity is not None)
        ex = _explore.check_explore(explore, explore_seed, explore_from, stage2_k, None, bool(auction), head_weights is not None,
                                    diversity is not None)
        uc = user_categorical.to(self.device)
        un = user_numerical.to(self.device, dtype=torch.float32)
        excl = None if exclude_ad_ids is None else [exclude_ad_ids]
        if ad_features_lookup is None:                                            # :329-331
            blk = _exclude.as_block(excl, 1)
            # threads: the enqueue under the process-wide lock, like AdRecommenderInference (amdrec._lib.Gate); the read-back
            # outside it
            with _lib.GATE.serving():
                with _lib.GATE.enqueue:
                    emb = self.two_tower_model.get_user_embeddings(uc, un)
                    ids, dist = self.faiss_index.search_device(
                        emb[:1] if blk is not None or incl is not None else emb, stage1_k,
                        exclude=None if blk is None else torch.from_numpy(blk).to(self.device), max_per_group=cap1,
                        boost_weight=stage1_boost,
                        **({} if incl is None else {"include": torch.from_numpy(incl).to(self.device)}))
                return ids[0].tolist(), dist[0].tolist()
        with _lib.GATE.enqueue:                                                   # (one builder of the lazy recommender)
            rec = self._rec
            if rec is None or self._rec_table is not ad_features_lookup:
                rec = AdRecommenderInference(device=str(self.device), two_tower_model=self.two_tower_model,
                                             transformer_ranker=self.transformer_ranker,
                                             faiss_index=self.faiss_index, ad_features=ad_features_lookup)
                self._rec, self._rec_table = rec, ad_features_lookup
        r = rec.recommend_tensors(uc[:1], un[:1], stage2_k, stage1_k,             # one synchronisation, indices validated
                                        exclude_ad_ids=excl, max_per_group=cap, stage1_max_per_group=cap1,
                                        rank_by=rank_by, reserve=reserve, diversity=diversity,
                                        diversity_pool=diversity_pool, stage1_boost=stage1_boost,
                                        head_weights=head_weights if not isinstance(head_weights, torch.Tensor)
                                        else head_weights[:1], _include_host=incl,
                                        **({} if ex is None else dict(
                                            explore=ex.temperature[:1] if isinstance(ex.temperature, torch.Tensor) else ex.temperature,
                                            explore_seed=ex.seed[:1] if isinstance(ex.seed, torch.Tensor) else ex.seed,
                                            explore_from=ex.greedy)))[0]
        return r["ad_ids"], r["scores"]["ctr"]                                    # :359-369 (ids, ctr probabilities)


class GraphedRecommender:
    """hipGraph replay of AdRecommenderInference.recommend_device for one (batch, top_k, stage1_k) shape.
    The graph owns everything its kernel nodes point at: static input/output tensors (torch's graph
    memory pool) and a private, fixed-size workspace (never the shared grow-only one)."""

    def __init__(self, rec: AdRecommenderInference, batch_size: int, top_k: int, stage1_k: int, warmup: int = 2,
                 max_exclude: int = 0, eligibility: bool = False, max_per_group: Optional[int] = None,
                 stage1_max_per_group: Optional[int] = None, rank_by: Optional[str] = None, reserve: bool = False,
                 diversity: Optional[float] = None, diversity_pool: int = 64, stage1_boost: bool = False,
                 head_weights: bool = False, max_include: int = 0, explore: bool = False, explore_from: int = 0):
        # the capture gate first: while another thread captures, the runtime is in its global capture mode, and the
        # allocations and fills of the static buffers below would already disturb it.  Refused before the device is touched
        with _lib.GATE.capturing():
            self._init(rec, batch_size, top_k, stage1_k, warmup, max_exclude, eligibility, max_per_group, stage1_max_per_group,
                       rank_by, reserve, diversity, diversity_pool, stage1_boost, head_weights, max_include, explore,
                       explore_from)

    def _init(self, rec, batch_size, top_k, stage1_k, warmup, max_exclude, eligibility, max_per_group, stage1_max_per_group,
              rank_by, reserve, diversity, diversity_pool, stage1_boost, head_weights=False, max_include=0, explore=False,
              explore_from=0):
        self.rec, self.batch_size, self.top_k, self.stage1_k = rec, batch_size, top_k, stage1_k
        # the per-group caps: scalars fixed at capture (the group keys are those of capture time, pinned below)
        self.max_per_group, self.stage1_max_per_group = rec._check_caps(max_per_group, stage1_max_per_group)
        caps = dict(max_per_group=self.max_per_group, stage1_max_per_group=self.stage1_max_per_group)
        # the auction: rank_by fixed at capture (the bids are those of capture time, pinned below); reserve=True: a static
        # [batch_size] reserve buffer, zeros = every non-NaN eCPM passes
        self.rank_by = rank_by
        auction = rec._check_auction(rank_by, 0.0 if reserve else None) is not None
        # the diversified selection: lam and the pool fixed at capture (the rows are those of capture time, pinned below)
        self.diversity, self.diversity_pool = diversity, diversity_pool
        if rec._check_diversity(diversity, diversity_pool, top_k, () if auction else None) is not None:
            caps.update(diversity=diversity, diversity_pool=diversity_pool)
        self._reserve = None
        # value ranking: head_weights=True gives the graph a static [batch_size, n_tasks] weight buffer (1.0 for the CTR head
        # until the replayer fills it) and the value selection; the refusals are recommend_device's
        self._head_w, self._auction = None, auction
        if head_weights:
            self._tasks = list(rec.transformer_ranker.prediction_heads.keys())
            self._head_default = tuple(1.0 if t == "ctr" else 0.0 for t in self._tasks)
            _value.check_head_weights(self._head_default, self._tasks, None, auction, diversity is not None)
        # exploration: explore=True gives the graph static [batch_size] temperature and seed buffers (zeros: every user served
        # greedily, until the replayer fills them) and the sampled selection; the prefix is fixed at capture; the refusals
        # are recommend_device's
        if not isinstance(explore, bool):
            raise TypeError(f"capture(explore=) takes True or False (the replayer takes the temperatures), got {explore!r}")
        ex = _explore.check_explore(0.0 if explore else None, 0 if explore else None, explore_from, top_k, None, auction,
                                    bool(head_weights), diversity is not None)
        self._temp = self._seed = None
        self.max_exclude = int(max_exclude)
        _exclude.check_exclude(stage1_k, self.max_exclude)
        # the include list: a static [batch_size, max_include] block (-1 = padding = nothing listed); None: no merge step
        self.max_include = int(max_include)
        if self.max_include < 0:
            raise ValueError(f"max_include={max_include}: the width of the include block, >= 0")
        if self.max_include:
            rec._check_include(torch.empty((0, self.max_include)), stage1_k, stage1_max_per_group)
        dev = rec.ad_features.device
        n_cat = len(rec.two_tower_model.user_tower._names)
        n_num = rec.two_tower_model.user_tower._n_num
        self._uc = torch.zeros((batch_size, n_cat), dtype=torch.int64, device=dev)
        self._un = torch.zeros((batch_size, n_num), dtype=torch.float32, device=dev)
        # static exclusion block (-1 = padding = nothing excluded); None: the graph has no exclusion step
        self._ex = torch.full((batch_size, self.max_exclude), -1, dtype=torch.int64, device=dev) if self.max_exclude else None
        # static eligibility masks (zeros = no constraint); None: the graph runs the plain search
        self.eligibility = bool(eligibility)
        self._masks = torch.zeros((2, batch_size), dtype=torch.int64, device=dev) if self.eligibility else None
        ma, my = (self._masks[0], self._masks[1]) if self.eligibility else (None, None)
        if auction:
            if reserve:
                self._reserve = torch.zeros((batch_size,), dtype=torch.float32, device=dev)
            caps.update(rank_by=rank_by, reserve=self._reserve)
        if head_weights:
            self._head_w = _value.weights_tensor(self._head_default, batch_size, dev)
            caps.update(head_weights=self._head_w)
        # static stage-1 boost weights (zeros = the plain search's positions); None: the graph runs the plain search
        self._boost_w = torch.zeros((batch_size,), dtype=torch.float32, device=dev) if stage1_boost else None
        if stage1_boost:
            rec.faiss_index._check_boost(self._boost_w, self.eligibility)
            caps.update(stage1_boost=self._boost_w)
        self._in = None
        if self.max_include:
            self._in = torch.full((batch_size, self.max_include), -1, dtype=torch.int64, device=dev)
            caps.update(include_ad_ids=self._in)
        if ex is not None:
            self._temp = torch.zeros((batch_size,), dtype=torch.float32, device=dev)
            self._seed = torch.zeros((batch_size,), dtype=torch.int64, device=dev)
            caps.update(explore=self._temp, explore_seed=self._seed, explore_from=ex.greedy)
        # sizing + warm-up pass on the shared workspace (packs weights, sets kernel attributes)
        # the capture swaps the process-wide workspace and the runtime's capture mode is global: not beside other threads'
        # calls (amdrec._lib.Gate: refused, either way round - __init__ holds the gate), and no other thread enqueues in between
        self._replay_lock, self._replay_owner, self._replay_depth = threading.Lock(), None, 0
        with _lib.GATE.enqueue:
            self._capture(rec, dev, top_k, stage1_k, warmup, ma, my, caps)
        # pin every device buffer the kernel nodes point at: a later load_state_dict / index.add() / larger eager search
        # then makes the graph stale (documented) but can never leave it with dangling pointers
        self._pinned = (rec.two_tower_model.user_tower._packed, rec.transformer_ranker._packed, rec.ad_features,
                        rec.transformer_ranker._ad_cache, *rec.faiss_index.resident_tensors())

    def _capture(self, rec, dev, top_k, stage1_k, warmup, ma, my, caps):
        probe = _lib.MeasuringArena(_lib.Workspace())
        with _lib.WORKSPACE.private(probe):
            for _ in range(max(1, warmup)):
                rec.recommend_device(self._uc, self._un, top_k, stage1_k, exclude_ad_ids=self._ex, require_all=ma, require_any=my,
                                     **caps)
        torch.cuda.synchronize(dev)
        self._arena = _lib.FixedArena(probe.high_water, dev)
        with _lib.WORKSPACE.private(self._arena):
            rec.recommend_device(self._uc, self._un, top_k, stage1_k, exclude_ad_ids=self._ex, require_all=ma,
                                 require_any=my, **caps)                                               # one eager pass on the private arena
            torch.cuda.synchronize(dev)
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._out = rec.recommend_device(self._uc, self._un, top_k, stage1_k, exclude_ad_ids=self._ex, require_all=ma,
                                                 require_any=my, **caps)
        torch.cuda.synchronize(dev)

    def replaying(self):
        """The scope of one replay: entered by ``__call__``, and by a caller that wants to keep the static output buffers to
        itself until it has read them.  A second thread that enters while it is held gets AmdrecError - it does not wait:
        one GraphedRecommender serves one thread at a time (threads)."""
        return _lib._Scope(self._enter_replay, self._exit_replay)

    def _enter_replay(self):
        me = threading.get_ident()
        with self._replay_lock:
            if self._replay_owner not in (None, me):
                raise _lib.AmdrecError("this GraphedRecommender is being replayed by another thread: its outputs are static "
                                       "buffers, one thread at a time (INTEGRATION.md, threads)")
            self._replay_owner, self._replay_depth = me, self._replay_depth + 1

    def _exit_replay(self):
        with self._replay_lock:
            self._replay_depth -= 1
            if not self._replay_depth:
                self._replay_owner = None

    def __call__(self, user_categorical: torch.Tensor, user_numerical: torch.Tensor,
                 exclude: Optional[torch.Tensor] = None, require_all: Optional[torch.Tensor] = None,
                 require_any: Optional[torch.Tensor] = None, reserve=None, stage1_boost=None, head_weights=None,
                 include: Optional[torch.Tensor] = None, explore=None, explore_seed=None):
        """One replay - arguments and result: ``_replay`` - inside ``replaying()`` and the serving scope: a replay that
        overlaps another thread's replay of this object, or another thread's capture, raises AmdrecError before it has
        touched the static buffers."""
        with self.replaying(), _lib.GATE.serving():
            return self._replay(user_categorical, user_numerical, exclude, require_all, require_any, reserve, stage1_boost,
                                head_weights, include, explore, explore_seed)

    @torch.no_grad()
    def _replay(self, user_categorical: torch.Tensor, user_numerical: torch.Tensor,
                exclude: Optional[torch.Tensor] = None, require_all: Optional[torch.Tensor] = None,
                require_any: Optional[torch.Tensor] = None, reserve=None, stage1_boost=None, head_weights=None,
                include: Optional[torch.Tensor] = None, explore=None, explore_seed=None):
        """Device tensors [batch_size, ...] -> the same dict as recommend_device (static output buffers,
        overwritten by the next call).  ``exclude``: device int64 [batch_size, E <= max_exclude] ad ids (negative =
        padding), copied into the graph's block; None = nothing excluded (the block is filled with -1).  ``require_all`` /
        ``require_any``: device int64 [batch_size] eligibility masks, copied into the graph's buffers (None = zeros: no
        constraint); a graph captured without ``eligibility`` raises ValueError for them.  ``reserve``: a float >= 0 or a
        device float32 [batch_size], copied into the graph's reserve buffer (None = zeros); a graph captured without
        ``reserve=True`` raises ValueError for it.  ``stage1_boost``: a number or a device float32 [batch_size], copied into
        the graph's weight buffer (None = zeros); a graph captured without ``stage1_boost=True`` raises ValueError for it.
        ``head_weights``: a dict, a sequence or a device float32 [batch_size, n_tasks] as recommend_device takes them, written
        into the graph's weight buffer (None = 1.0 for the CTR head, 0.0 for the others); a graph captured without
        ``head_weights=True`` raises ValueError for it.  ``include``: device int64 [batch_size, I <= max_include] ad ids
        (negative = padding), copied into the graph's include block; None = nothing listed (the block is filled with -1); a
        graph captured without ``max_include`` raises ValueError for it.  ``explore`` / ``explore_seed``: the temperatures
        and seeds as recommend_device takes them, each written into the graph's buffer when given; one that is not given
        leaves its buffer as it stands (a replay without a new seed redraws with the old ones); a graph captured without
        ``explore=True`` raises ValueError for them."""
        if explore is not None or explore_seed is not None:
            if self._temp is None:
                raise ValueError("captured without explore=True: this graph takes the arg-max and holds no temperatures or seeds")
            # (each is checked as recommend_device checks it; the other's place is taken by a valid stand-in)
            ex = _explore.check_explore(0.0 if explore is None else explore, 0 if explore_seed is None else explore_seed, 0,
                                        self.top_k, self.batch_size)
            if explore is not None:
                _explore.temperature_tensor(ex.temperature, self.batch_size, self._temp.device, out=self._temp)
            if explore_seed is not None:
                _explore.seed_tensor(ex.seed, self.batch_size, self._seed.device, out=self._seed)
        if include is not None and (self._in is None or include.dim() != 2 or include.shape[0] != self.batch_size
                                    or include.shape[1] > self.max_include or include.dtype != torch.int64):
            raise ValueError(f"captured with max_include={self.max_include} for batch {self.batch_size}, got an include block "
                             f"of shape {tuple(include.shape)} ({include.dtype})")
        if head_weights is not None:
            if self._head_w is None:
                raise ValueError("captured without head_weights=True: this graph ranks by the CTR head and takes no weights")
            head_weights = _value.check_head_weights(head_weights, self._tasks, self.batch_size, self._auction)
        if self._head_w is not None:
            _value.weights_tensor(self._head_default if head_weights is None else head_weights, self.batch_size,
                                  self._head_w.device, out=self._head_w)
        if stage1_boost is not None:
            if self._boost_w is None:
                raise ValueError("captured without stage1_boost=True: this graph runs the plain search and takes no boost weight")
            if isinstance(stage1_boost, torch.Tensor):
                if stage1_boost.dtype != torch.float32 or stage1_boost.shape != (self.batch_size,):
                    raise ValueError(f"stage1_boost must be float32 [{self.batch_size}], got {stage1_boost.dtype} "
                                     f"{tuple(stage1_boost.shape)}")
            else:
                stage1_boost = _boost.check_weight(stage1_boost)
        if self._boost_w is not None:
            if isinstance(stage1_boost, torch.Tensor):
                self._boost_w.copy_(stage1_boost)
            else:
                self._boost_w.fill_(0.0 if stage1_boost is None else stage1_boost)
        if user_categorical.shape[0] != self.batch_size:
            raise ValueError(f"captured for batch {self.batch_size}, got {user_categorical.shape[0]}")
        if exclude is not None and (self._ex is None or exclude.dim() != 2 or exclude.shape[0] != self.batch_size
                                    or exclude.shape[1] > self.max_exclude):
            raise ValueError(f"captured with max_exclude={self.max_exclude} for batch {self.batch_size}, got an exclusion "
                             f"block of shape {tuple(exclude.shape)}")
        if require_all is not None or require_any is not None:
            if self._masks is None:
                raise ValueError("captured without eligibility=True: this graph runs the plain search and takes no masks")
            for m in (require_all, require_any):
                if m is not None and (m.dtype != torch.int64 or m.shape != (self.batch_size,)):
                    raise ValueError(f"masks must be int64 [{self.batch_size}], got {m.dtype} {tuple(m.shape)}")
        if reserve is not None:
            if self._reserve is None:
                raise ValueError("captured without reserve=True: this graph holds no reserve buffer")
            reserve = _auction.check_reserve(reserve, self.batch_size)
        if self._reserve is not None:
            if isinstance(reserve, torch.Tensor):
                self._reserve.copy_(reserve)
            else:
                self._reserve.fill_(0.0 if reserve is None else reserve)
        if self._masks is not None:
            for row, m in zip(self._masks, (require_all, require_any)):
                row.zero_() if m is None else row.copy_(m)
        if self._ex is not None:
            if exclude is None or exclude.shape[1] < self.max_exclude:
                self._ex.fill_(-1)
            if exclude is not None:
                self._ex[:, :exclude.shape[1]].copy_(exclude)
        if self._in is not None:
            if include is None or include.shape[1] < self.max_include:
                self._in.fill_(-1)
            if include is not None:
                self._in[:, :include.shape[1]].copy_(include)
        self._uc.copy_(user_categorical)
        self._un.copy_(user_numerical)
        self._graph.replay()
        return self._out


def build_faiss_index(model: TwoTowerModel, ad_categorical, device="cuda", save_path: Optional[str] = None,
                      batch_size: int = 1 << 18, index_type: str = "IVF", nlist: int = 100,
                      nprobe: int = 10) -> FAISSIndex:
    """Corpus build (training_pipeline.py:488-546): AdTower over every row in dataset order
    (shuffle=False, :513), ad id = row index (:523), add to the index, optionally save.
    ``ad_categorical`` is the [N, 20] integer table; embeddings never leave the device."""
    model = model.to(device).eval()
    table = ad_categorical if isinstance(ad_categorical, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(ad_categorical))
    idx = FAISSIndex(model.output_dim, index_type=index_type, nlist=nlist, nprobe=nprobe, device=device)
    embs = []
    with torch.no_grad():
        for s in range(0, table.shape[0], batch_size):
            embs.append(model.get_ad_embeddings(table[s:s + batch_size].to(device)))
    emb = torch.cat(embs) if embs else torch.empty((0, model.output_dim), device=device)
    idx.add(emb)                                         # default ids = arange (:523 / faiss_retrieval.py:121)
    if save_path:
        idx.save(save_path)
    return idx
