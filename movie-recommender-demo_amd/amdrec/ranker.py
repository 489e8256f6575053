"""Drop-in for the reference's ``TransformerRanker`` (transformer_ranker.py:207-415): same
constructor, same parameter names/shapes (reference checkpoints load unchanged, including the
dead W_q / W_k and the unused positional rows 1..49), eval-mode ``forward`` on libamdrec.

``forward(user_categorical, ad_categorical, numerical, mask=None)`` keeps the reference's
argument order (ad_categorical is SECOND, unlike TwoTowerModel) and returns the logits dict
``{'ctr','engagement','revenue'}``.  ``mask`` is accepted and ignored: with the sequence
length fixed at 1 (:358) softmax over a single key is 1.0 whatever the mask says.
``score_candidates`` is the pipeline entry: one user row broadcast over its stage-1
candidates, ad features gathered from a resident table by candidate id.

Writes the framework cannot see: the packed weights and the per-ad caches are keyed by tensor identity and ``_version``.
A write through ``.data`` (``p.data.copy_(w)``, ``p.data = t``), a raw pointer or a DLPack alias changes neither and is
outside the keys: call ``invalidate()`` after such a write to a weight, and replace the ad table by a new tensor after
such a write to its rows.  A copy of the module (``copy.deepcopy``, ``pickle``, ``torch.save(model)``) carries no
derived state and packs for itself on first use.
"""
from __future__ import annotations

import weakref
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, weights


class _Attention(nn.Module):
    def __init__(self, d_model, num_heads, dropout):
        super().__init__()
        assert d_model % num_heads == 0
        self.d_model, self.num_heads, self.d_k = d_model, num_heads, d_model // num_heads
        for n in ("W_q", "W_k", "W_v", "W_o"):
            setattr(self, n, nn.Linear(d_model, d_model))
        self.dropout = nn.Dropout(dropout)


class _FFN(nn.Module):
    def __init__(self, d_model, d_ff, dropout):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(d_model, d_ff), nn.Linear(d_ff, d_model)
        self.dropout = nn.Dropout(dropout)


class _EncoderLayer(nn.Module):
    def __init__(self, d_model, num_heads, d_ff, dropout):
        super().__init__()
        self.self_attention = _Attention(d_model, num_heads, dropout)
        self.feed_forward = _FFN(d_model, d_ff, dropout)
        self.norm1, self.norm2 = nn.LayerNorm(d_model), nn.LayerNorm(d_model)
        self.dropout1, self.dropout2 = nn.Dropout(dropout), nn.Dropout(dropout)


class _Cross(nn.Module):
    def __init__(self, dim, num_crosses, dropout):
        super().__init__()
        self.num_crosses = num_crosses
        self.cross_weights = nn.ParameterList([nn.Parameter(torch.randn(dim, dim)) for _ in range(num_crosses)])
        self.cross_biases = nn.ParameterList([nn.Parameter(torch.randn(dim)) for _ in range(num_crosses)])
        self.dropout = nn.Dropout(dropout)


def _head(d_model, dropout):
    return nn.Sequential(nn.Linear(d_model, 256), nn.ReLU(), nn.Dropout(dropout), nn.Linear(256, 64), nn.ReLU(),
                         nn.Dropout(dropout), nn.Linear(64, 1))


class _Packed(NamedTuple):          # TransformerRanker._packed: the weights as packed under ``key`` (``_pack``)
    key: Tuple
    params: weights.RankerParams
    keep: weights.Packed
    tasks: List[str]


class _AdCache(NamedTuple):         # TransformerRanker._ad_cache: one ad table's caches under the pack key they were built with
    key: Tuple
    data_ptr: int                   # data_ptr, shape, version: the table's ``_table_key``
    shape: Tuple
    version: int
    proj: torch.Tensor
    hidden: Optional[torch.Tensor]
    table: "weakref.ref"            # the table itself: address, shape and version all repeat once a table has been freed


def _table_key(table):
    return table.data_ptr(), tuple(table.shape), table._version


def _entry(key, table, proj, hidden) -> _AdCache:
    return _AdCache(key, *_table_key(table), proj, hidden, weakref.ref(table))


class TransformerRanker(nn.Module):
    def __init__(self, user_feature_dims: Dict[str, int], ad_feature_dims: Dict[str, int], numerical_dim: int,
                 embedding_dim: int = 32, d_model: int = 256, num_heads: int = 8, num_layers: int = 3,
                 d_ff: int = 1024, max_seq_len: int = 50, dropout: float = 0.1, num_objectives: int = 3):
        super().__init__()
        self.user_embeddings = nn.ModuleDict({n: nn.Embedding(c, embedding_dim) for n, c in user_feature_dims.items()})
        self.ad_embeddings = nn.ModuleDict({n: nn.Embedding(c, embedding_dim) for n, c in ad_feature_dims.items()})
        total = (len(user_feature_dims) + len(ad_feature_dims)) * embedding_dim + numerical_dim
        self.feature_projection = nn.Linear(total, d_model)
        self.positional_encoding = nn.Parameter(torch.randn(1, max_seq_len, d_model))
        self.transformer_layers = nn.ModuleList([_EncoderLayer(d_model, num_heads, d_ff, dropout)
                                                 for _ in range(num_layers)])
        self.feature_interaction = _Cross(d_model, 3, dropout)
        self.prediction_heads = nn.ModuleDict({t: _head(d_model, dropout) for t in ("ctr", "engagement", "revenue")})
        self.d_model = d_model
        self.dropout = nn.Dropout(dropout)
        self._user_names, self._ad_names, self._n_num = list(user_feature_dims), list(ad_feature_dims), numerical_dim
        self._packed = None
        self._ad_cache = None
        # W_ov = W_o W_v pre-multiplied on the host (exact algebra at seq_len 1; set False to run the two
        # GEMMs in the reference's order)
        self.fuse_attention = True
        # encoder layer 1's attention block folded into the feature projection (exact algebra at seq_len 1: x0 + W_ov x0 +
        # b_ov is linear in the projection's input; weights.folded_projection).  Needs fuse_attention and applies only
        # where every pass runs the row-owner kernel (gemm_engine "f16x3" or "f16" on its architecture, x3_min_rows = 1): one
        # 256 x 256 GEMM less per candidate row.  The fp32 / bf16x6 engines keep the unfolded chain.
        self.fold_first_attention = True
        # stage 1 of layer 1's FFN served from a second per-ad cache (weights.first_ffn_cache: with the fold,
        # W_1 LN1(z) + b_1 = rstd * (P[ad] + Q[user]) + c): passes of more than 16384 rows on the folded 16-row kernel read
        # two rows instead of multiplying with W_1.  ``ensure_ad_cache`` builds P [N, d_ff] fp32 beside the projection
        # cache while both fit ``hidden_cache_max_bytes`` (N * (d_model + d_ff) * 4: 5 KB per ad at the default widths);
        # larger tables, smaller passes and the other engines run the uncached program.
        self.cache_first_ffn = True
        self.hidden_cache_max_bytes = 8 << 30
        # engine of the big passes (> 8192 rows), all fp32 in / fp32 out with fp32-level error:
        #  "f16x3"  (default) the row-owner kernel (csrc/rowowner.hpp): operands split into two fp16 planes, three
        #           fp16-MFMA products per MAC, everything after the projection in ONE kernel, activations in registers
        #  "bf16x6" the round-1 tile GEMMs on three bf16 planes, six products per MAC (also the fallback of "f16x3" for
        #           architectures the row-owner kernel is not written for)
        #  "fp32"   fp32 MFMA everywhere
        # and one opt-in engine of REDUCED precision:
        #  "f16"    the row-owner 16-row kernels with ONE fp16-MFMA product per MAC on the high planes of the streams that
        #           "f16x3" packs (csrc/rowowner16.hpp "SINGLE PRODUCT"): operands carry 11 significant bits, logits differ
        #           from fp32's by about 1e-4 of a row's largest activation (DESIGN.md "Ranker: single-product fp16
        #           engine").  Every pass runs it - fold, hidden cache, CTR-first and graph capture as under "f16x3" - so it
        #           needs x3_variant 16 and x3_min_rows 1 (ValueError at pack time otherwise); on an architecture the
        #           row-owner kernels are not written for it falls back as "f16x3" does, to the fp32-accurate tile GEMMs
        self.gemm_engine = "f16x3"
        # smallest pass that takes the row-owner kernel.  1 = every batch: one launch (~0.35 ms per 128-row round, bound by
        # one CU's weight-stream rate) matches the ~25 small launches of the fp32 path at a single request (0.60 ms end to
        # end either way) and beats it from 2 users up (B = 16: 0.65 vs 0.79 ms; tools/latency_by_engine.py)
        self.x3_min_rows = 1
        self.x3_variant = 16                          # 16: rowowner16.hpp (two waves per SIMD, default: 15 % faster); 32: rowowner.hpp
        # passes of at most this many rows take the column-split kernel (csrc/rowowner16c.hpp: 16 rows per workgroup, the
        # waves split the output features; bit-identical results).  0 = the library's default (4096 rows = 8 requests of
        # 500 candidates), -1 = never
        self.x3_cs_max_rows = 0

    # ENGINES: the engines of fp32-level error - accuracy sweeps iterate this tuple and hold every member to the fp32 engine's
    # error.  REDUCED_ENGINES: the opt-in engines that trade accuracy for speed; ``gemm_engine`` takes a name of either.
    ENGINES = ("f16x3", "bf16x6", "fp32")
    REDUCED_ENGINES = ("f16",)
    ALL_ENGINES = ENGINES + REDUCED_ENGINES
    ROW_OWNER_ENGINES = ("f16x3", "f16")      # the engines of csrc/ranker_x3.hip: three products per MAC, or one
    SMALL_ROWS = 8192       # passes of at most this many rows run the fp32-MFMA small shapes (csrc/layers.hip)

    def x3_fallback_reason(self):
        """Why ``gemm_engine = "f16x3"`` would NOT run the row-owner kernel for these weights (None: it runs): the
        engine is written for the reference's default architecture; anything else takes the generic tile GEMMs
        (bf16x6 above SMALL_ROWS rows, fp32 MFMA below).  The first such pack also logs a warning - the fallback is
        correct (golden-tested on the tutorial's architecture) but several times slower, and must not be silent."""
        return weights.x3_ineligible_reason(self.state_dict(), self.fuse_attention)

    def ctr_first_unsupported_reason(self):
        """Why CTR-first ranking (``score_ctr_first`` + ``winner_scores``; AdRecommenderInference ``heads="ctr_first"``) would
        NOT run for this ranker (None: it runs).  The mode exists on the 16-row kernels of the row-owner engine alone; the
        pipeline then runs the all-heads path, whose results are the same by definition."""
        # (asked once per request by the pipeline: the answer is kept while nothing it depends on can have changed - the
        # switches below, and the architecture, which only a re-registered tensor can change)
        key = (self.gemm_engine, self.fuse_attention, int(self.x3_variant), int(self.x3_min_rows), _lib._REG_EPOCH[0])
        c = self.__dict__.get("_ctr_first_why")
        if c is None or c[0] != key:
            c = self.__dict__["_ctr_first_why"] = (key, self._ctr_first_unsupported_reason())
        return c[1]

    def _ctr_first_unsupported_reason(self):
        if self.gemm_engine not in self.ROW_OWNER_ENGINES:
            return f"gemm_engine {self.gemm_engine!r} (the mode runs on the f16x3 row-owner kernels only)"
        why = self.x3_fallback_reason()
        if why is not None:
            return f"not the row-owner engine's architecture ({why})"
        if int(self.x3_variant) != 16:
            return f"x3_variant {self.x3_variant} (the 32-row kernel has no task window and no gathered input)"
        if int(self.x3_min_rows) != 1:
            return f"x3_min_rows {self.x3_min_rows} (every pass, the winners' included, must run the row-owner kernel)"
        tasks = list(self.prediction_heads.keys())
        if not tasks or tasks[0] != "ctr":
            return "the ranking task (ctr) is not task 0"
        if len(tasks) < 2:
            return "no task besides the ranking task"
        return None

    def gemm_engine_for(self, rows: int) -> str:
        """The engine a pass of ``rows`` rows actually runs on."""
        eng = self.gemm_engine
        if eng in self.ROW_OWNER_ENGINES:
            if weights.x3_eligible(self.state_dict(), self.fuse_attention):
                return eng if rows >= self.x3_min_rows else "fp32"       # ("f16": x3_min_rows is 1, _pack refuses others)
            eng = "bf16x6"                                                # no reduced-precision fallback
        return eng if rows > self.SMALL_ROWS else "fp32"

    # -- packing ----------------------------------------------------------------------
    def invalidate(self):
        """Drop the packed weights and the per-ad caches: the next eval-mode call packs (and caches) again.  Both are keyed
        by what torch shows of a change - the device, the engine switches, every parameter's and buffer's ``_version`` and
        identity; the caches also by the ad table's identity, address, shape and ``_version``.  A write it cannot see
        (``p.data.copy_(w)``, ``p.data = t``, a raw pointer, a DLPack alias) changes none of them, so the HIP path would keep
        serving the old weights while the ATen path (``autograd_forward``, train mode) already shows the new ones: call
        this after such a write to a weight.  After such a write to the ad table, hand the ranker a new tensor (the
        pipeline: assign it to ``rec.ad_features``)."""
        self._packed = None
        self._ad_cache = None
        self.__dict__.pop("_ctr_first_why", None)
        _lib.drop_tensor_list(self)

    def __getstate__(self):                        # deepcopy / pickle / torch.save(module): a copy packs for itself
        return _lib.copyable_state(self)

    def _apply(self, fn, *a, **k):                 # .to() / .cuda() / .float(): tensors may be replaced
        r = super()._apply(fn, *a, **k)
        self.invalidate()
        return r

    def cache_ad_projection(self, ad_table: Optional[torch.Tensor]):
        """Candidate-side cache for ``score_candidates``: the ad half of the feature projection,
        W_proj[:, ad columns] . emb(ad_table[a]), for every row of the resident ad-feature table
        ([N, d_model] fp32, N * 1 KB of HBM at d_model 256).  Like the ad-tower embeddings in the index it depends
        on the ad and the weights only; with it stage 2 replaces the widest-K GEMM of the ranker by a row gather and
        returns bit-identical logits.  ``None`` drops the cache.  Re-packing the weights (load_state_dict, a
        parameter update) drops it too; ``score_candidates`` uses it only for the very table it was built from."""
        self._ad_cache = None
        if ad_table is None:
            return None
        table = _lib.require_gpu(ad_table, "ad_table", torch.int64)
        if not table.is_contiguous() or table.dim() != 2 or table.shape[1] != len(self._ad_names):
            raise ValueError("ad_table must be a contiguous [N, n_ad_feat] int64 tensor")
        dev = table.device
        params, _ = self._pack(dev)
        if not params.w_proj_ad:
            return None                                     # no ad features / no split projection
        lib = _lib.load()
        out = torch.empty((table.shape[0], self.d_model), dtype=torch.float32, device=dev)
        ws = _lib.WORKSPACE.get(4 * self.d_model + 256, dev)
        _lib.check(lib.amdrec_ranker_project_ads(_lib.C.byref(params), _lib.ptr(table), table.shape[0], _lib.ptr(out),
                                                 out.stride(0), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._ad_cache = _entry(self._packed.key, table, out, None)
        return out

    def ensure_ad_cache(self, ad_table):
        """Build the cache for ``ad_table`` unless a valid one exists (weights or table changed -> rebuilt) - and, with
        ``cache_first_ffn`` on weights packed for it, the first-FFN hidden cache P [N, d_ff] beside it while both fit
        ``hidden_cache_max_bytes``.  The cap holds for a hidden cache that exists already: one built under a larger cap is
        dropped here (the projection cache stays), as a fresh ranker under the same cap would have none."""
        params, _ = self._pack(ad_table.device)
        if self._entry_for(ad_table) is None:
            self.cache_ad_projection(ad_table)
        c = self._entry_for(ad_table)
        if c is None or not params.x3.w_hidden_ad:
            return
        n, d_ff = int(ad_table.shape[0]), int(params.d_ff)
        fits = n * (self.d_model + d_ff) * 4 <= int(self.hidden_cache_max_bytes)
        if c.hidden is not None:
            if not fits:                                    # the cap was lowered under a cache built before: the uncached program
                self._ad_cache = c._replace(hidden=None)
            return
        if not fits:
            return
        dev = ad_table.device
        hid = torch.empty((n, d_ff), dtype=torch.float32, device=dev)
        ws = _lib.WORKSPACE.get(4 * d_ff + 256, dev)
        _lib.check(_lib.load().amdrec_ranker_project_ads_hidden(
            _lib.C.byref(params), _lib.ptr(ad_table), n, _lib.ptr(hid), hid.stride(0), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)))
        self._ad_cache = c._replace(hidden=hid)

    def compact_ad_cache(self, old_table, kept, new_table):
        """Rows left the ad table: ``new_table`` = ``old_table[kept]`` (``kept``: device int64, old positions).  If a valid
        cache exists for ``old_table``, its rows are moved along - the projection cache, and the hidden cache when there is
        one, gathered by ``kept`` into NEW tensors, bit for bit (amdrec_rows_gather; the old tensors are left as they are
        for whoever still reads them) - and the cache now belongs to ``new_table``.  Otherwise nothing happens: the cache
        is built lazily, as ever."""
        from .rows_edit import gather_rows
        if not isinstance(old_table, torch.Tensor) or not old_table.is_cuda:
            return
        self._pack(old_table.device)
        c = self._entry_for(old_table)
        if c is None:
            return
        hid = None if c.hidden is None else gather_rows(c.hidden, kept)
        self._ad_cache = _entry(c.key, new_table, gather_rows(c.proj, kept), hid)

    def extend_ad_cache(self, old_table, new_table):
        """Rows were appended to the ad table: ``new_table[:len(old_table)]`` equals ``old_table``.  If a valid cache exists
        for ``old_table``, only the appended rows are projected (amdrec_ranker_project_ads, and _hidden when the hidden
        cache exists and both caches still fit ``hidden_cache_max_bytes`` at the new size - else the hidden cache is
        dropped), into grown copies of the caches, which then belong to ``new_table``.  Otherwise nothing happens."""
        from .rows_edit import grown_copy
        if not isinstance(old_table, torch.Tensor) or not old_table.is_cuda:
            return
        dev = old_table.device
        params, _ = self._pack(dev)
        c = self._entry_for(old_table)
        if c is None:
            return
        n_old, n_new = int(old_table.shape[0]), int(new_table.shape[0])
        if n_new < n_old or not new_table.is_contiguous() or new_table.shape[1:] != old_table.shape[1:]:
            raise ValueError("extend_ad_cache: new_table must be old_table plus appended rows, contiguous")
        lib = _lib.load()
        tail = new_table[n_old:]
        proj = grown_copy(c.proj, n_old, n_new)
        hid = None
        if c.hidden is not None and n_new * (self.d_model + int(params.d_ff)) * 4 <= int(self.hidden_cache_max_bytes):
            hid = grown_copy(c.hidden, n_old, n_new)
        if n_new > n_old:
            ws = _lib.WORKSPACE.get(4 * max(self.d_model, int(params.d_ff)) + 256, dev)
            out = proj[n_old:]
            _lib.check(lib.amdrec_ranker_project_ads(_lib.C.byref(params), _lib.ptr(tail), n_new - n_old, _lib.ptr(out),
                                                     proj.stride(0), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
            if hid is not None:
                out = hid[n_old:]
                _lib.check(lib.amdrec_ranker_project_ads_hidden(
                    _lib.C.byref(params), _lib.ptr(tail), n_new - n_old, _lib.ptr(out), hid.stride(0), _lib.ptr(ws),
                    ws.numel(), _lib.stream_ptr(dev)))
        self._ad_cache = _entry(c.key, new_table, proj, hid)

    def _entry_for(self, table) -> Optional[_AdCache]:
        """The cache entry valid for ``table`` - built under the current pack key for this very tensor OBJECT at its current
        data_ptr, shape and _version - or None.  The object itself is compared (through a weak reference): the caching
        allocator hands a freed table's block to the next table of its shape, and a loader that runs the same code gives
        that one the same _version."""
        c = getattr(self, "_ad_cache", None)
        if c is None or self._packed is None or c.key != self._packed.key or c.table() is not table or \
                c[1:4] != _table_key(table):
            return None
        return c

    def _cache_for(self, table):
        return getattr(self._entry_for(table), "proj", None)

    def _hidden_cache_for(self, table):
        """The first-FFN hidden cache that goes with ``_cache_for(table)`` (None: not built)."""
        return getattr(self._entry_for(table), "hidden", None)

    def _pack(self, device):
        if self.gemm_engine not in self.ALL_ENGINES:
            raise ValueError(f"gemm_engine must be one of {self.ALL_ENGINES}")
        # (the key - and with it the ad-projection cache, which is only served for the key it was built under - covers the
        # fold: an engine switch repacks and rebuilds the cache in the other projection form)
        key = (str(device), self.fuse_attention, bool(self.fold_first_attention), bool(self.cache_first_ffn),
               self.gemm_engine, int(self.x3_min_rows), int(self.x3_variant), int(self.x3_cs_max_rows),
               _lib.tensor_versions(self))
        if self._packed is None or self._packed.key != key:
            sd = self.state_dict()
            row_owner = self.gemm_engine in self.ROW_OWNER_ENGINES
            if self.gemm_engine == "f16" and int(self.x3_variant) != 16:
                raise ValueError(f"gemm_engine 'f16' runs on the 16-row kernels only (x3_variant {self.x3_variant})")
            if self.gemm_engine == "f16" and int(self.x3_min_rows) != 1:
                raise ValueError(f"gemm_engine 'f16' runs every pass or none: x3_min_rows must be 1, not {self.x3_min_rows} "
                                 "(fp16 for some batch sizes and fp32 for others is a trap)")
            why = weights.x3_ineligible_reason(sd, self.fuse_attention) if row_owner else None
            x3 = row_owner and why is None
            if why is not None:
                import warnings
                warnings.warn(f"amdrec TransformerRanker: gemm_engine {self.gemm_engine!r} is not available for these weights ({why}); "
                              f"running the generic tile GEMMs (bf16x6 above {self.SMALL_ROWS} rows, fp32 MFMA below)",
                              RuntimeWarning, stacklevel=3)
            self._packed = _Packed(key, *weights.pack_ranker(
                sd, self._user_names, self._ad_names, self._n_num, device, fuse_attention=self.fuse_attention,
                x6=self.gemm_engine == "bf16x6" or (row_owner and not x3), x3=x3,
                x3_products=1 if self.gemm_engine == "f16" else 3,
                x3_min_rows=self.x3_min_rows, x3_variant=self.x3_variant, x3_cs_max_rows=self.x3_cs_max_rows,
                fold_first_attention=bool(self.fold_first_attention), cache_first_ffn=bool(self.cache_first_ffn)))
        return self._packed.params, self._packed.tasks

    def load_state_dict(self, state_dict, *a, **k):
        r = super().load_state_dict(state_dict, *a, **k)
        self.invalidate()
        return r

    # -- forward ----------------------------------------------------------------------
    def autograd_forward(self, user_categorical, ad_categorical, numerical, mask=None):
        """The reference's op sequence on ATen with autograd (transformer_ranker.py:310-380 with :59-88, :114, :148-153,
        :199-203): used in train mode.  The LITERAL 8-head attention is kept here - with the attention-weight dropout
        (:73) active the seq-len-1 softmax weight is 0 or 1/(1-p) per (row, head), not the constant 1 of eval mode."""
        import math
        F = torch.nn.functional
        ue = torch.cat([e(user_categorical[:, i].long()) for i, e in enumerate(self.user_embeddings.values())], dim=1)
        ae = torch.cat([e(ad_categorical[:, i].long()) for i, e in enumerate(self.ad_embeddings.values())], dim=1)
        x = self.feature_projection(torch.cat([ue, ae, numerical], dim=1)).unsqueeze(1)        # :328, :355-358
        x = self.dropout(x + self.positional_encoding[:, :1, :])                                # :361-362
        for layer in self.transformer_layers:
            at = layer.self_attention
            B = x.size(0)
            q = at.W_q(x).view(B, -1, at.num_heads, at.d_k).transpose(1, 2)
            k = at.W_k(x).view(B, -1, at.num_heads, at.d_k).transpose(1, 2)
            v = at.W_v(x).view(B, -1, at.num_heads, at.d_k).transpose(1, 2)
            scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(at.d_k)
            if mask is not None:
                scores = scores.masked_fill(mask == 0, -1e9)
            w = at.dropout(F.softmax(scores, dim=-1))
            ctx = torch.matmul(w, v).transpose(1, 2).contiguous().view(B, -1, at.d_model)
            x = layer.norm1(x + layer.dropout1(at.W_o(ctx)))                                    # :148-149
            ff = layer.feed_forward
            x = layer.norm2(x + layer.dropout2(ff.fc2(ff.dropout(F.relu(ff.fc1(x))))))           # :114, :152-153
        x = x.squeeze(1)
        fi = self.feature_interaction
        x0, xl = x, x
        for i in range(fi.num_crosses):
            xl = fi.dropout(x0 * (torch.matmul(xl, fi.cross_weights[i]) + fi.cross_biases[i]) + xl)   # :201-202
        return {t: head(xl).squeeze(1) for t, head in self.prediction_heads.items()}            # :375-378

    def _bound_params(self, ad_cat, use_cache):
        """(params, tasks) packed for ``ad_cat``'s device, with the per-ad caches valid for that table (or none) bound."""
        params, tasks = self._pack(ad_cat.device)
        cache = self._cache_for(ad_cat) if use_cache else None
        params.ad_proj_cache = cache.data_ptr() if cache is not None else None
        params.ld_ad_proj_cache = cache.stride(0) if cache is not None else 0
        hidden = self._hidden_cache_for(ad_cat) if cache is not None else None
        params.ad_hidden_cache = hidden.data_ptr() if hidden is not None else None
        params.ld_ad_hidden_cache = hidden.stride(0) if hidden is not None else 0
        return params, tasks

    def _run(self, user_cat, numerical, user_rowdiv, ad_cat, ad_rowmap, rows, check_indices=True, raw=False,
             use_cache=False):
        if self.training:
            raise NotImplementedError("score_candidates / the HIP forward implement eval() semantics only; call .eval()")
        dev = ad_cat.device
        params, tasks = self._bound_params(ad_cat, use_cache)
        lib = _lib.load()
        logits = torch.empty((len(tasks), rows), dtype=torch.float32, device=dev)
        if rows == 0:
            return (tasks, logits) if raw else {t: logits[i] for i, t in enumerate(tasks)}
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if check_indices else None
        nbytes = _lib.C.c_size_t(0)
        _lib.check(lib.amdrec_ranker_workspace(_lib.C.byref(params), rows, _lib.C.byref(nbytes)))
        ws = _lib.WORKSPACE.get(nbytes.value, dev)
        _lib.check(lib.amdrec_ranker_forward(
            _lib.C.byref(params), _lib.ptr(user_cat), _lib.ptr(numerical), user_rowdiv, _lib.ptr(ad_cat),
            _lib.ptr(ad_rowmap), rows, _lib.ptr(logits), logits.stride(0), _lib.ptr(flag),
            user_cat.shape[0], ad_cat.shape[0], _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        if check_indices and int(flag.item()):
            raise IndexError("index out of range in self")
        return (tasks, logits) if raw else {t: logits[i] for i, t in enumerate(tasks)}

    def forward(self, user_categorical, ad_categorical, numerical, mask: Optional[torch.Tensor] = None):
        """transformer_ranker.py:332-380 -> {'ctr','engagement','revenue'}: logits [B].  train() mode: the same network
        in stock PyTorch autograd (``autograd_forward``), for amdrec.training."""
        if self.training:
            return self.autograd_forward(user_categorical, ad_categorical, numerical, mask)
        uc = _lib.require_gpu(user_categorical, "user_categorical").long().contiguous()
        ac = _lib.require_gpu(ad_categorical, "ad_categorical").long().contiguous()
        nm = _lib.require_gpu(numerical, "numerical").to(torch.float32).contiguous()
        B = uc.shape[0]
        if uc.shape != (B, len(self._user_names)) or ac.shape != (B, len(self._ad_names)) or \
                nm.shape != (B, self._n_num):
            raise ValueError("bad feature shapes")
        return self._run(uc, nm, 1, ac, None, B)

    def score_candidates(self, user_categorical, numerical, candidate_rows, ad_table, check_indices=False,
                         raw=False):
        """Pipeline form of inference.py:241-255: user u's features are broadcast over its
        ``k = candidate_rows.shape[1]`` candidates (no .repeat), ad features are gathered from the
        resident ``ad_table [N, n_ad_feat]`` by candidate row.  -> logits dict, each [U*k]
        (``raw=True``: (task names, one [n_tasks, U*k] tensor)).
        A NEGATIVE candidate row means "no candidate" (an unfilled slot of a search result): it never faults (every gather
        clamps it to row 0), its logits are unspecified but finite for finite weights and features, and every other row's
        logits are, bit for bit, what they are with any valid row in its place.  ``check_indices=True``: a user index or an
        ad-table entry outside its embedding table, or a candidate row >= ``ad_table.shape[0]``, raises IndexError (as the
        reference's embedding lookup / ``ad_table[cand]`` would); a negative candidate row does not.  Without the flag a
        row past the table is clamped to its last row, silently."""
        uc = _lib.require_gpu(user_categorical, "user_categorical").long().contiguous()
        nm = _lib.require_gpu(numerical, "numerical").to(torch.float32).contiguous()
        cand = _lib.require_gpu(candidate_rows, "candidate_rows", torch.int64).contiguous()
        table = _lib.require_gpu(ad_table, "ad_table", torch.int64)
        if not table.is_contiguous():
            raise ValueError("ad_table must be contiguous")
        U, k = cand.shape
        if uc.shape[0] != U or nm.shape[0] != U:
            raise ValueError("one user row per candidate list expected")
        return self._run(uc, nm, k, table, cand.view(-1), U * k, check_indices, raw, use_cache=True)

    # -- CTR-first ranking: pass 1 = trunk + CTR head on every candidate, pass 2 = the other heads on the winners ------
    def ctr_first_ready(self, ad_table, rows: int, winner_rows: int) -> bool:
        """Whether ``score_ctr_first`` on ``rows`` candidate rows of ``ad_table`` and ``winner_scores`` on ``winner_rows``
        winners would both run (amdrec_ranker_ctr_first_supported); packs the mode's weight streams on first use
        (weights.pack_ctr_first: the pack key and the existing streams are untouched)."""
        if self.training or rows < 1 or winner_rows < 1 or self.ctr_first_unsupported_reason() is not None:
            return False
        params, _ = self._bound_params(ad_table, True)
        if not weights.pack_ctr_first(params, self._packed.keep):
            return False
        lib = _lib.load()
        return bool(lib.amdrec_ranker_ctr_first_supported(_lib.C.byref(params), rows)) and \
            bool(lib.amdrec_ranker_ctr_first_supported(_lib.C.byref(params), winner_rows))

    def score_ctr_first(self, user_categorical, numerical, candidate_rows, ad_table, check_indices=False, _ready=False):
        """Pass 1 of CTR-first ranking, arguments as ``score_candidates``: the projection, the trunk and the CTR head alone.
        -> (ctr_logits [U*k], trunk [U*k, 256]): bit for bit the CTR row of ``score_candidates`` and, per row, the state its
        heads receive.  ``trunk`` (rows x 1 KB) is a view of the shared workspace (``_lib.WORKSPACE``), meant for the
        ``winner_scores`` call that follows: any other workspace-taking call may overwrite it.  Raises where
        ``ctr_first_ready`` is False: there is no fall-back in here."""
        uc = _lib.require_gpu(user_categorical, "user_categorical").long().contiguous()
        nm = _lib.require_gpu(numerical, "numerical").to(torch.float32).contiguous()
        cand = _lib.require_gpu(candidate_rows, "candidate_rows", torch.int64).contiguous()
        table = _lib.require_gpu(ad_table, "ad_table", torch.int64)
        if not table.is_contiguous():
            raise ValueError("ad_table must be contiguous")
        U, k = cand.shape
        if uc.shape[0] != U or nm.shape[0] != U:
            raise ValueError("one user row per candidate list expected")
        rows, dev = U * k, table.device
        if not _ready and not self.ctr_first_ready(table, max(rows, 1), max(rows, 1)):    # (_ready: the caller has asked)
            raise _lib.AmdrecError("CTR-first ranking is not available for this ranker and shape: " +
                                   (self.ctr_first_unsupported_reason() or "amdrec_ranker_ctr_first_supported says no"))
        params, _ = self._bound_params(table, True)
        lib = _lib.load()
        nbytes = _lib.C.c_size_t(0)
        _lib.check(lib.amdrec_ranker_ctr_first_workspace(_lib.C.byref(params), rows, rows, _lib.C.byref(nbytes)))
        # one block [workspace of both passes | trunk rows]: the winners' pass reads the trunk while it works in the front part
        off_t = (nbytes.value + 255) // 256 * 256
        blk = _lib.WORKSPACE.get(off_t + rows * 1024, dev)
        logits = torch.empty(rows, dtype=torch.float32, device=dev)
        trunk = blk[off_t:off_t + rows * 1024].view(torch.float32).view(rows, 256)
        if rows == 0:
            return logits, trunk
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if check_indices else None
        _lib.check(lib.amdrec_ranker_forward_ctr_first(
            _lib.C.byref(params), _lib.ptr(uc), _lib.ptr(nm), k, _lib.ptr(table), _lib.ptr(cand), rows, _lib.ptr(logits), rows,
            _lib.ptr(flag), uc.shape[0], table.shape[0], _lib.ptr(trunk), 256, _lib.ptr(blk), off_t, _lib.stream_ptr(dev)))
        if check_indices and int(flag.item()):
            raise IndexError("index out of range in self")
        return logits, trunk

    def winner_scores(self, trunk, slots, k_c: int, out_scores):
        """Pass 2: ``slots`` int32 [U, top_k] = the winning slots amdrec_select_topk chose among each user's ``k_c`` rows of
        ``trunk`` ([U * k_c, 256] from ``score_ctr_first``); runs the heads of every task but the first on those rows and
        writes their probabilities into ``out_scores[1:]`` (contiguous float32 [n_tasks, U, top_k]; plane 0 is the
        selection's) - 0.0 where the slot is negative.  -> out_scores."""
        trunk = _lib.require_gpu(trunk, "trunk", torch.float32)
        slots = _lib.require_gpu(slots, "slots", torch.int32)
        out_scores = _lib.require_gpu(out_scores, "out_scores", torch.float32)
        dev = trunk.device
        params, tasks = self._pack(dev)
        U, top_k = slots.shape
        if trunk.dim() != 2 or trunk.shape[1] != 256 or trunk.stride(1) != 1 or not slots.is_contiguous() or \
                not out_scores.is_contiguous() or tuple(out_scores.shape) != (len(tasks), U, top_k):
            raise ValueError("winner_scores: trunk [rows, 256], contiguous slots [U, top_k] and out_scores [n_tasks, U, top_k]")
        if U == 0:
            return out_scores
        if not weights.pack_ctr_first(params, self._packed.keep):
            raise _lib.AmdrecError("CTR-first ranking is not available for this ranker: " +
                                   str(self.ctr_first_unsupported_reason()))
        lib = _lib.load()
        nbytes = _lib.C.c_size_t(0)
        _lib.check(lib.amdrec_ranker_ctr_first_workspace(_lib.C.byref(params), 0, U * top_k, _lib.C.byref(nbytes)))
        ws = _lib.WORKSPACE.get(nbytes.value, dev)
        # the shared workspace may be the very block ``trunk`` lives in (score_ctr_first): work in the part in front of it
        lo, t0 = ws.data_ptr(), trunk.data_ptr()
        if lo <= t0 < lo + ws.numel():
            ws = ws[:t0 - lo] if t0 - lo >= nbytes.value else torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        _lib.check(lib.amdrec_ranker_winner_heads(
            _lib.C.byref(params), _lib.ptr(trunk), trunk.stride(0), trunk.shape[0], _lib.ptr(slots), U, int(k_c), top_k,
            _lib.ptr(out_scores), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return out_scores

    def compute_loss(self, predictions, labels, task_weights=None):
        """transformer_ranker.py:382-415: weighted sum of per-task BCE-with-logits -> (total, dict of floats)."""
        if task_weights is None:
            task_weights = {"ctr": 1.0, "engagement": 0.5, "revenue": 0.3}
        losses, total = {}, 0
        for task in predictions.keys():
            if task in labels:
                tl = torch.nn.functional.binary_cross_entropy_with_logits(predictions[task], labels[task].float())
                losses[f"{task}_loss"] = tl.item()
                total = total + task_weights.get(task, 1.0) * tl
        losses["total_loss"] = total.item()
        return total, losses
