"""Shared machinery of the quantised decoder blocks (LLaMA / OPT): quant-state switches, the fused
smooth-and-quant step, the final fold, parameter selectors and the omni state dict.

Reference: models/int_llama_layer.py:269-368 and models/int_opt_layer.py:348-452 (the two copies are
identical up to module names).
"""
from collections import OrderedDict

import os

import torch
import torch.nn as nn

from . import let as L
from .linear import QuantLinear
from .matmul import QuantMatMul


#: Steps of at least this many query rows over a ragged / paged bfloat16 cache with a past run the MFMA chunked-prefill
#: attention (oq_attn_extend*); shorter ones stay on the decode kernel.  Never below 16 (the measurement).
EXTEND_MIN_TQ = 16


class QuantBlockMixin:
    #: activation / temp-weight dtype of the HIP path: torch.bfloat16 (MFMA bf16) or torch.float32 (exact)
    compute_dtype = torch.bfloat16
    let = False

    # subclasses define: _let_names() -> dict(q,k,v,o,fc1=[...],last, ln1, ln2)

    def set_quant_state(self, weight_quant: bool = False, act_quant: bool = False):
        self.use_weight_quant = weight_quant
        self.use_act_quant = act_quant
        for m in self.modules():
            if isinstance(m, (QuantLinear, QuantMatMul)):
                m.set_quant_state(weight_quant, act_quant)

    def _quant_linears(self):
        return [m for m in self.modules() if isinstance(m, QuantLinear)]

    # ---- block boundary dtype -------------------------------------------------------------------------------------
    # The kernels compute in bfloat16 (MFMA bf16) or float32 (parity mode).  A float16 hidden state -- what the
    # reference's fp16 model hands to the layers it gets back from omniquant() (main.py evaluate) -- is converted to the
    # compute dtype on entry and the result is returned in float16 again, so the returned model keeps its dtype contract.
    def _enter(self, hidden_states):
        from . import ops
        if hidden_states.dtype == torch.float16:
            cd = self.compute_dtype if self.compute_dtype in (torch.bfloat16, torch.float32) else torch.bfloat16
            return ops.cast(hidden_states, cd), torch.float16
        return hidden_states, None

    @staticmethod
    def _leave(hidden_states, back):
        from . import ops
        return hidden_states if back is None else ops.cast(hidden_states, back)

    # ---- packed (real-quant) inference -----------------------------------------------------------------------------
    # realquant.pack_block / load_packed_block mark the block; its forward checks the mark once at entry and runs a plain
    # weight-only inference path on the PackedLinear kernels (no fake quant, no autograd, no graph capture).
    def _packed_check(self, past_key_value=None, use_cache=False, output_attentions=False):
        from ._capi import OQError
        mark = self.__dict__["_oq_packed"]
        bits = mark["act_bits"]
        if bits < 16 and not mark.get("act_quant"):
            raise OQError(f"packed block with {bits}-bit activation quantisers: real quantisation is weight-only (AutoGPTQ's "
                          "QuantLinear has no activation quantiser); evaluate W*A<16 models with the fake-quant block instead")
        if output_attentions:
            raise NotImplementedError("the packed inference path does not return attention weights")

    # ---- incremental decoding (past_key_value / use_cache) on the packed path ----------------------------------------------
    def _kv_cache_in(self, past_key_value, bsz, Tq, nkv, hd, x, head_bits=None):
        """The PackedKVCache this forward appends to: a new one (prefill), the caller's (appended in place) or a copy of a
        reference-layout (k, v) tuple converted to the compute dtype (the caller's tensors are left alone).  head_bits (W4A4
        blocks, whose cache holds head-quantised k / v): the tuple's raw rows are quantised once, on import.
        A block packed with kv_cache_bits=4 creates, and converts tuples into, 4-bit code caches; a caller's PackedKVCache of
        either kind is taken as it is (an empty pre-sized code cache switches an unmarked W4A4 block to codes), except that a
        code cache needs the head quantisers (head_bits 4).  So is a caller's PagedKVCache (paged, ragged storage), which a
        layer view of a model-wide PagedKVPool (pool.layer(l)) is too; a block never creates one by itself.
        A weight-only block (head_bits None) packed with kv_cache_bits=8 creates, and converts tuples into, 8-bit code caches,
        and takes a caller's 8-bit code cache whether marked or not; a W4A4 block refuses one, as a weight-only block refuses
        a 4-bit one."""
        from ._capi import OQError
        from .kvcache import PackedKVCache, PagedKVCache, PagedKVPool
        if hd not in (64, 128):
            raise OQError(f"KV-cache decoding covers head_dim 64 and 128 (oq_attn_decode), not {hd}")
        code_bits = self.__dict__["_oq_packed"].get("kv_cache_bits")
        if past_key_value is None:
            return PackedKVCache(bsz, nkv, hd, x.dtype, x.device, Tq, code_bits=code_bits)
        if isinstance(past_key_value, PagedKVPool):
            raise OQError(f"{past_key_value!r} holds every layer's pages: pass pool.layer(l) to layer l as past_key_value")
        if isinstance(past_key_value, (PackedKVCache, PagedKVCache)):
            c = past_key_value
            if (c.bs, c.nkv, c.hd) != (bsz, nkv, hd) or c.dtype != x.dtype or c.device != x.device:
                raise OQError(f"{c!r} does not fit this block's step: batch {bsz}, {nkv} kv heads of {hd}, {x.dtype} on {x.device}")
            if c.code_bits == 8:
                if head_bits is not None:
                    raise OQError(f"{c!r}: code_bits 8 is the weight-only blocks' cache (this W4A4 block's k / v sit on its "
                                  f"{head_bits}-bit head grid: code_bits 4)")
            elif c.code_bits is not None and head_bits != c.code_bits:
                raise OQError(f"{c!r}: code_bits {c.code_bits} needs a W4A4 block (this block's k / v are not on a 4-bit grid)")
            return c
        if isinstance(past_key_value, (tuple, list)) and len(past_key_value) == 2:
            k = past_key_value[0]
            if not torch.is_tensor(k) or k.dim() != 4 or (k.shape[0], k.shape[1], k.shape[3]) != (bsz, nkv, hd):
                raise OQError(f"past_key_value {tuple(getattr(k, 'shape', ()))}: expected [{bsz}, {nkv}, T, {hd}]")
            return PackedKVCache.from_tuple(past_key_value, dtype=x.dtype, capacity=k.shape[2] + Tq, head_bits=head_bits,
                                            code_bits=code_bits)
        raise OQError(f"past_key_value of type {type(past_key_value).__name__}: expected None, a (k, v) tuple, a PackedKVCache or a "
                      "PagedKVCache")

    @staticmethod
    def _new_tokens_in(new_tokens, past_key_value, bsz, T, device):
        """new_tokens (the valid step rows per sequence of a right-padded ragged step) as (int32 [bs] device tensor or None,
        what the cache's host bound grows by, the counts as Python ints or None).  None: all T rows.  A Python sequence of ints
        is checked (0 <= n <= T) and uploaded, and the bound grows by its maximum; a device tensor is taken as it is -- its
        values are never read -- and the bound grows by T.  Without a ragged cache (PackedKVCache(ragged=True) or a
        PagedKVCache) as past_key_value it is refused."""
        from ._capi import OQError
        if new_tokens is None:
            return None, T, None
        if not getattr(past_key_value, "ragged", False):
            raise OQError("new_tokens needs a ragged PackedKVCache as past_key_value (PackedKVCache(..., ragged=True))")
        if torch.is_tensor(new_tokens):
            if new_tokens.dtype != torch.int32 or tuple(new_tokens.shape) != (bsz,) or new_tokens.device != device:
                raise OQError(f"new_tokens: expected an int32 [{bsz}] tensor on {device}, got {tuple(new_tokens.shape)} "
                              f"{new_tokens.dtype} on {new_tokens.device}")
            return new_tokens, T, None
        try:
            seq = [new_tokens[i].__index__() for i in range(len(new_tokens))]
        except (TypeError, AttributeError):
            raise OQError(f"new_tokens: expected {bsz} ints or an int32 [{bsz}] device tensor, got {new_tokens!r}") from None
        if len(seq) != bsz or min(seq) < 0 or max(seq) > T:
            raise OQError(f"new_tokens {seq}: one count in [0, {T}] for each of the {bsz} sequences")
        return torch.tensor(seq, dtype=torch.int32).to(device, non_blocking=True), max(seq), seq

    @staticmethod
    def _positions(position_ids, past, bsz, T, device):
        """position_ids (None: past .. past + T - 1; [T]; [1 | bs, T]) as the int64 [1 | bs, T] tensor the append gathers at."""
        if position_ids is None:
            return torch.arange(past, past + T, dtype=torch.int64, device=device)[None]
        pos = position_ids.reshape(-1, position_ids.shape[-1]) if position_ids.dim() == 1 else position_ids
        if pos.dim() != 2 or pos.shape[1] != T or pos.shape[0] not in (1, bsz):
            raise ValueError(f"position_ids of shape {tuple(position_ids.shape)} for a batch of {bsz} x {T} tokens")
        return pos.to(device=device, dtype=torch.int64)

    def _step_positions(self, position_ids, cache, bsz, T, device):
        """_positions at the cache's length; None for a ragged cache with a past and no position_ids: the append kernel then
        rotates sequence b's row t at lengths[b] + t, and no position tensor is built."""
        if cache.ragged and cache.length > 0 and position_ids is None:
            return None
        return self._positions(position_ids, cache.length, bsz, T, device)

    @staticmethod
    def _tree_in(tree, cache, attention_mask, position_ids, new_tokens, bsz, T, rope=True):
        """The checks of a speculative TREE step (forward(..., tree=kvcache.TokenTree)), made before the cache changes, and its
        RoPE positions: int64 [bs, T] = lengths[b] + depth(t), one elementwise op on the device with no host read (None
        without rope: OPT).  The step needs a ragged bfloat16 cache with a past, takes no attention_mask, position_ids or
        new_tokens, and its T rows are the tree's nodes."""
        from ._capi import OQError
        from .kvcache import TokenTree
        if not isinstance(tree, TokenTree):
            raise OQError(f"tree: expected a kvcache.TokenTree, got {type(tree).__name__}")
        if attention_mask is not None or position_ids is not None or new_tokens is not None:
            raise OQError("a tree step takes no attention_mask, position_ids or new_tokens: the tree is the mask, a node rotates at "
                          "lengths[b] + its depth, and all Tq nodes are appended")
        if cache is None or not getattr(cache, "ragged", False):
            raise OQError("a tree step needs a ragged cache as past_key_value (PackedKVCache(ragged=True), a PagedKVCache or a "
                          "pool's layer view)")
        if cache.dtype != torch.bfloat16 or cache.length <= 0:
            raise OQError(f"a tree step needs a bfloat16 cache with a past (length > 0), got {cache!r}")
        if tree.Tq != T or tree.bs not in (None, bsz):
            raise OQError(f"{tree!r} does not fit a step of {bsz} x {T} rows (one row per node)")
        if not rope:
            return None
        return cache.lengths[:, None].to(torch.int64) + tree.to(cache.device).depth

    def _cached_attention(self, q, k, v, cache, attention_mask, scale, cos=None, sin=None, positions=None, head_bits=None,
                          new_tokens=(None, None, None), tree=None):
        """Attention of this step's q [bs, Tq, nh, hd] over the cache plus this step's k / v, which are appended to it (rotated
        by cos / sin at `positions` when given: LLaMA).  Without a past (prefill) the attention is exactly the no-cache path's
        (_packed_attention on the rotated q / k); with a past it is oq_attn_decode, with no host synchronisation.
        head_bits (W4A4 blocks): q / k / v (float32 or the cache's dtype) also pass the per-(token, head) quantiser of that
        width in the append's launch, so the cache holds, and the attention reads, the quantised values in the cache's dtype.
        A code cache (cache.code_bits 4) receives the codes instead (oq_kv_append_quant_codes) and steps with a past run
        oq_attn_decode_codes on them; its prefill runs the same attention launches on the same q / k / v values.
        An 8-bit code cache (cache.code_bits 8; weight-only blocks, head_bits None): k / v pass the cache's own 8-bit quantiser
        in the append's launch (oq_kv_append_codes8; q is only rotated) and the prefill attends the DEQUANTISED rows (k_out /
        v_out), which is what every later step reads from the cache (oq_attn_decode_codes8 / oq_attn_extend_codes8).
        A ragged cache (cache.ragged): the append and the attention read the same pre-step cache.lengths on the device
        (lengths= of the ops), `past` and L are host bounds, and the step's rows are right-padded: new_tokens = (counts or None
        for all Tq, growth of the bound, the counts on the host or None) from _new_tokens_in says how many rows of each sequence
        count.  All Tq rows are
        written; rows at or beyond a sequence's new length are scratch that its next step overwrites, and the outputs of pad
        query rows are finite and unspecified.  With cache.length == 0 this is the prefill above (the caller's causal mask
        keeps right padding away from the valid rows; the append goes at lengths = 0).  With a past the mask must be None
        (row t of sequence b attends rows <= lengths[b] + t) and positions None leaves them to the kernel (lengths[b] + t).
        A decode step on a ragged cache performs no device-to-host read and builds no mask or position tensor.
        A step of Tq >= EXTEND_MIN_TQ rows over a ragged bfloat16 cache with a past (a prompt chunk, a forked prefix's suffix, a
        new turn, draft tokens) runs ops.extend_attention / extend_attention_codes instead of the decode kernel (_extend_step):
        the same lengths, L and pad-row contract, the same absence of host reads.
        A paged cache (cache.paged, always ragged; kvcache.PagedKVCache): the same ops calls on its page pools with
        page_table=cache.page_table; reserve() gives every sequence the pages the step's rows need (uploading the table only
        if one was added).  Nothing else about the step changes.
        After the attention a ragged cache books the step itself (cache.book_step): lengths, the bound `length` and, paged, the
        host bounds; a layer view of a PagedKVPool books it with its pool, which applies it once all layers have.
        tree (a kvcache.TokenTree, checked by _tree_in, which also builds `positions` = lengths[b] + depth): the step's Tq rows
        are the nodes of a tree of draft tokens.  They are reserved and appended like any step's rows, attended by
        ops.tree_attention (always, also below EXTEND_MIN_TQ) and booked as a TREE step (cache.book_tree_step): no length
        moves until cache.commit_tree."""
        from . import ops
        from ._capi import OQError
        bsz, Tq = q.shape[0], q.shape[1]
        past = cache.length
        L = past + Tq
        lens = cache.lengths if cache.ragged else None
        paged = {"page_table": cache.page_table} if getattr(cache, "paged", False) else {}
        if lens is not None and past > 0 and attention_mask is not None:
            raise OQError("a ragged cache with a past takes no attention_mask: each sequence attends its own rows "
                          "(pass attention_mask=None)")
        if attention_mask is not None and (attention_mask.dim() != 4 or attention_mask.shape[0] not in (1, bsz)
                                           or tuple(attention_mask.shape[1:]) != (1, Tq, L)):
            raise ValueError(f"Attention mask should be of size {(bsz, 1, Tq, L)}, but is {attention_mask.size()}")
        cache.reserve(Tq)
        rot = cos is not None
        # copies of this step's rows for the prefill's attention, of every tensor the append changes
        if head_bits is None and cache.code_bits == 8:
            qr = torch.empty_like(q) if rot else q
            kr, vr = (torch.empty_like(k), torch.empty_like(v)) if past == 0 else (None, None)
            ops.kv_append_codes(k, v, cache.dtype, cache.k_codes, cache.v_codes, cache.k_meta, cache.v_meta,
                                past=0 if cache.ragged else past, q=q if rot else None, q_out=qr if rot else None, k_out=kr,
                                v_out=vr, cos=cos, sin=sin, positions=positions, lengths=lens, **paged)
        elif head_bits is None:
            qr = torch.empty_like(q) if rot else q
            kr, vr = torch.empty_like(k) if (rot and past == 0) else None, None
            ops.kv_append(k, v, cache.k, cache.v, 0 if cache.ragged else past, q=q if rot else None, q_out=qr if rot else None,
                          k_out=kr, cos=cos, sin=sin, positions=positions, lengths=lens, **paged)
        else:
            qr = torch.empty(q.shape, dtype=cache.dtype, device=q.device)
            kr, vr = (torch.empty(k.shape, dtype=cache.dtype, device=q.device) for _ in range(2)) if past == 0 else (None, None)
            if cache.code_bits is not None:
                ops.kv_append_codes(k, v, cache.dtype, cache.k_codes, cache.v_codes, cache.k_meta, cache.v_meta,
                                    past=0 if cache.ragged else past, q=q, q_out=qr, k_out=kr, v_out=vr, cos=cos, sin=sin,
                                    positions=positions, lengths=lens, **paged)
            else:
                ops.kv_append_quant(k, v, head_bits, cache.dtype, k_cache=cache.k, v_cache=cache.v, past=0 if cache.ragged else past,
                                    q=q, q_out=qr, k_out=kr, v_out=vr, cos=cos, sin=sin, positions=positions, lengths=lens,
                                    **paged)
        if lens is None:
            cache.length = L
        if past == 0:
            mask = attention_mask
            if mask is not None and mask.shape[0] != bsz:
                mask = mask.expand(bsz, 1, Tq, L)
            attn = self._packed_attention(qr, k if kr is None else kr, v if vr is None else vr, mask, scale)
        elif tree is not None:
            attn = ops.tree_attention(qr, cache, L, scale, lens, tree, **paged)
        elif self._extend_step(cache, qr, Tq):
            if cache.code_bits is not None:
                attn = ops.extend_attention_codes(qr, cache, L, scale, lens, **paged)
            else:
                attn = ops.extend_attention(qr, cache.k, cache.v, L, scale, lens, **paged)
        elif cache.code_bits is not None:
            attn = ops.decode_attention_codes(qr, cache, L, scale, attention_mask, lengths=lens, **paged)
        else:
            attn = ops.decode_attention(qr, cache.k, cache.v, L, scale, attention_mask, lengths=lens, **paged)
        if lens is not None:
            # (after the attention, which reads the pre-step lengths; the stream orders the launches)
            if tree is not None:
                cache.book_tree_step(Tq)
            else:
                cache.book_step(Tq, new_tokens)
        return attn

    @staticmethod
    def _extend_step(cache, q, Tq):
        """Whether a step with a past goes to ops.extend_attention*: a ragged (or paged) bfloat16 cache and Tq >= EXTEND_MIN_TQ.
        OQ_NO_EXTEND=1 is the A/B switch: every step with a past then stays on the decode kernel."""
        from . import ops
        if not cache.ragged or Tq < EXTEND_MIN_TQ or os.environ.get("OQ_NO_EXTEND"):
            return False
        return cache.dtype == torch.bfloat16 and ops.extend_attention_supported(q.dtype, Tq, q.shape[3])

    @staticmethod
    def _packed_attention(q, k, v, attention_mask, scale):
        """softmax(scale * q k^T + mask) v on [bs, T, heads, hd] (k / v may have fewer heads: GQA): the fused causal kernel
        where it covers the problem, else scores -> softmax -> PV on the HIP GEMM."""
        from . import ops
        bsz, T = q.shape[0], q.shape[1]
        if attention_mask is not None and attention_mask.size() != (bsz, 1, T, T):
            raise ValueError(f"Attention mask should be of size {(bsz, 1, T, T)}, but is {attention_mask.size()}")
        causal = ops.mask_is_causal(attention_mask)
        if ops.fused_attention_supported(q, causal):
            return ops.FusedCausalAttnFn.apply(q, k, v, scale)
        probs = ops.SoftmaxFn.apply(ops.AttnScoresFn.apply(q, k, causal), attention_mask, scale, causal)
        return ops.AttnPVFn.apply(probs, v, causal)

    def _truncate_scales(self):
        arena = self.__dict__.get("_arena_truncate")
        if arena is not None:
            arena()                      # all LET scales are contiguous in the optimizer's arena: one launch
            return
        with torch.no_grad():
            for name, p in self.named_parameters():
                if "smooth_scale" in name:
                    L.truncate_number(p)

    def _f32c(self, t):
        """float32 copy of a frozen norm weight / bias buffer, cached (they never change during calibration)."""
        if t is None:
            return None
        if t.dtype == torch.float32:
            return t
        cache = self.__dict__.setdefault("_f32_cache", {})
        key = (id(t), t._version)
        hit = cache.get(id(t))
        if hit is None or hit[0] != key:
            cache[id(t)] = (key, t.detach().float().contiguous(), t)     # keep `t` alive so id() stays unique
        return cache[id(t)][1]

    # ---- second HIP stream for the weight path -----------------------------------------------------------------
    # The weight fake-quant kernels (HBM/VALU-bound, no LDS) and their backward depend only on the learnables and on
    # dL/dW, not on the activations, so they can run beside the MFMA-bound GEMMs of the activation path.  When
    # `_fq_stream` is set (StepRunner does it), they are enqueued on that stream; each QuantLinear waits for its
    # own weight's event right before its GEMM.  Autograd runs every backward node on the stream of its forward, so
    # the fake-quant BACKWARD kernels land on the side stream as well and overlap the remaining dgrad/wgrad GEMMs.
    def _weight_stream(self):
        """(stream, forked): the side stream when one is configured, else the current stream."""
        st = self.__dict__.get("_fq_stream")
        if st is None:
            return torch.cuda.current_stream(), False
        return st, True

    def _publish(self, mod, weight, bias, side, forked):
        mod.temp_weight, mod.temp_bias = weight, bias
        mod.use_temporary_parameter = True
        if forked:
            ev = torch.cuda.Event()
            ev.record(side)
            mod._temp_ready = ev
        else:
            mod._temp_ready = None

    def _weight_slabs(self, nm, dtype):
        """{module: destination of its fake-quant weight}: q | k | v (and gate | up) are written back to back into one
        buffer each, so that the sibling projections run as ONE GEMM per direction (ops.stacked_rows).  Per step, from the
        caching allocator (inside the captured graph's pool the addresses are static)."""
        dest = {}
        if os.environ.get("OQ_STACKED_GEMM", "1") == "0":
            return dest
        for group in ([nm["q"], nm["k"], nm["v"]], list(nm["fc1"])):
            # (the reference lists fc1 as [up_proj, gate_proj]; the MLP consumes gate first)
            if group and len(group) > 1 and all(isinstance(m, QuantLinear) for m in group) and \
                    len({(m.in_features, m.weight.device) for m in group}) == 1 and \
                    not any(m.weight_quantizer._identity() for m in group):
                if group[0] is not nm["q"]:
                    group = sorted(group, key=lambda m: 0 if m is getattr(getattr(self, "mlp", None), "gate_proj", None) else 1)
                from . import ops
                dev = group[0].weight.device
                rows_all, cols = sum(m.out_features for m in group), group[0].in_features
                slab = torch.empty((rows_all, cols), dtype=dtype, device=dev)
                # the LET by-product w @ shift of gate / up IS their bias (no vector kernel in between): stacked as well
                ws = torch.empty((rows_all,), dtype=torch.float32, device=dev) if group[0] is not nm["q"] else None
                # integer side channel (ops.IntCodes) of the siblings, stacked the same way: codes + scale | zp | csum vectors
                codes = vec = None
                if all(m.int_fprop_eligible(dtype) for m in group):
                    codes = torch.empty((rows_all, cols), dtype=torch.int8, device=dev)
                    vec = torch.empty((3, rows_all), dtype=torch.float32, device=dev)
                r = 0
                for m in group:
                    n = m.out_features
                    d = ops.WeightDest(slab[r:r + n], None if ws is None else ws[r:r + n])
                    if codes is not None:
                        d.codes, d.scale, d.zp, d.csum = codes[r:r + n], vec[0, r:r + n].view(n, 1), vec[1, r:r + n].view(n, 1), vec[2, r:r + n]
                    dest[m] = d
                    r += n
        return dest

    def _let_temporaries(self, out_dtype, lazy_mlp=False, stack=False):
        """Fused LET path: 6 fused transform+fake-quant kernels (one per smoothed linear) + ONE vector kernel for
        every norm weight/bias and projection bias.  Returns {module: (temp_weight, temp_bias)} and the norm temps.
        lazy_mlp: the MLP weights (no coupling with the vector kernel) are NOT quantised here; instead
        `lazy[mod]` is a closure that does it right before the module's GEMM, so that the 0.27 GB of MLP fake-quant
        weights do not flush the attention projections' weights out of the 256 MB Infinity Cache before they are used
        (same kernels, same values, different issue order)."""
        nm = self._let_names()
        from . import ops
        hidden = self.qkv_smooth_scale.numel()
        for key in ("q", "k", "v"):
            if nm[key].out_features != hidden:
                # smooth_q_k / smooth_fc_fc pair q, k, v and o row by row (models/transformation.py:44-69): the reference
                # dies on a broadcast error for grouped-query attention; fail as loudly instead of reading out of bounds
                raise NotImplementedError(f"LET with {key}_proj.out_features = {nm[key].out_features} != hidden size "
                                          f"{hidden}: grouped-query attention has no LET (use --lwc only)")
        specs = L.block_let_specs(nm, self, None)
        f = self._f32c
        mlp = set(nm["fc1"]) | {nm["last"]} if lazy_mlp else set()
        wq, ws, lazy = {}, {}, {}
        dest = self._weight_slabs(nm, out_dtype) if stack else {}

        def quant(mod, sp):
            # + integer codes for the int8 fprop (ops.IntCodes): of the step's temporaries, and of the FOLDED weights (float32
            # values, same codes) for the propagate pass that follows the fold
            want_int = mod.int_fprop_eligible(out_dtype if stack else self.compute_dtype)
            if sp.shift is not None:
                return mod.weight_quantizer.quantize(mod.weight, out_dtype=out_dtype, col_mul=sp.col_mul,
                                                     row_div=sp.row_div, row_mul=sp.row_mul, shift=sp.shift, out=dest.get(mod),
                                                     want_int=want_int)
            return mod.weight_quantizer.quantize(mod.weight, out_dtype=out_dtype, out=dest.get(mod), want_int=want_int), None

        def mlp_bias(mod, wsh):
            if mod is nm["last"]:
                return mod.bias
            return wsh if mod.bias is None else f(mod.bias) + wsh

        # issue order: the attention projections' weights are quantised LAST-USED-FIRST (o, v, k, q), so that the ones the
        # first GEMMs read are the most recently written and still sit in the 256 MB Infinity Cache (same kernels, same values)
        order = list(specs.items())
        if os.environ.get("OQ_WQ_ORDER", "1") != "0":
            rank = {nm["o"]: 0, nm["v"]: 1, nm["k"]: 2, nm["q"]: 3}
            order.sort(key=lambda it: rank.get(it[0], -1))
        fc1_group = [m for m in nm["fc1"] if m in mlp and m in specs]
        # gate / up in one quantiser launch per direction: both feed ONE stacked GEMM now, so nothing is gained any more by
        # quantising each right before "its" GEMM (+0.3 % same-box; before the stacked launches it cost 0.9 %)
        batch_fc1 = len(fc1_group) > 1 and os.environ.get("OQ_WQ_BATCH_MLP", "1") != "0"
        with ops.WeightQuantBatch():        # the weights quantised here and now (q, k, v, o) share one launch per direction
            for mod, sp in order:
                if mod in mlp:
                    if batch_fc1 and mod in fc1_group:
                        def make(mod=mod):
                            # whichever of gate / up is needed first quantises both in one launch
                            res = {}
                            with ops.WeightQuantBatch():
                                for m2 in fc1_group:
                                    res[m2] = quant(m2, specs[m2])
                            for m2 in fc1_group:
                                m2.temp_weight, m2.temp_bias = res[m2][0], mlp_bias(m2, res[m2][1])
                                if m2 is not mod:
                                    m2.__dict__.pop("_lazy_temp", None)
                    else:
                        def make(mod=mod, sp=sp):
                            w_, ws_ = quant(mod, sp)
                            mod.temp_weight, mod.temp_bias = w_, mlp_bias(mod, ws_)
                    lazy[mod] = make
                else:
                    wq[mod], ws[mod] = quant(mod, sp)
        q, k, v, o, ln1, ln2 = nm["q"], nm["k"], nm["v"], nm["o"], nm["ln1"], nm["ln2"]
        ln1_tw, ln1_tb, ln2_tw, ln2_tb, b_q, b_k, b_v, b_o = ops.LetVectorsFn.apply(
            self.qkv_smooth_scale, self.qkv_smooth_shift, self.out_smooth_scale, self.out_smooth_shift,
            self.fc1_smooth_scale, self.fc1_smooth_shift, self.qkt_smooth_scale,
            ws[q], ws[k], ws[v], ws[o], f(ln1.weight), f(getattr(ln1, "bias", None)), f(ln2.weight),
            f(getattr(ln2, "bias", None)), f(q.bias), f(k.bias), f(v.bias), f(o.bias))
        bias = {q: b_q, k: b_k, v: b_v, o: b_o}
        for mod in list(wq):
            if mod not in bias:
                bias[mod] = mlp_bias(mod, ws[mod])
        self.__dict__["_lazy_let"] = lazy
        return wq, bias, (ln1_tw, ln1_tb), (ln2_tw, ln2_tb)

    def smooth_and_quant_temporary(self):
        """LET re-parameterisation + weight fake-quant of every linear: ONE fused kernel per weight matrix plus one
        vector kernel (reference: ~25 eager passes per matrix, models/int_llama_layer.py:279-307)."""
        nm = self._let_names()
        dt = self.compute_dtype
        main = torch.cuda.current_stream()
        side, forked = self._weight_stream()
        if self.let:
            self._truncate_scales()
            if forked:
                side.wait_stream(main)      # parameters were updated (AdamW / truncate) on the main stream
            lazy_mlp = bool(self.__dict__.get("_lazy_mlp_quant")) and not forked
            with torch.cuda.stream(side):
                wq, bias, t1, t2 = self._let_temporaries(dt, lazy_mlp, stack=True)
                for mod in wq:
                    self._publish(mod, wq[mod], bias[mod], side, forked)
                for mod, fn in self.__dict__.pop("_lazy_let", {}).items():
                    mod.temp_weight, mod.temp_bias = None, None
                    mod.use_temporary_parameter = True
                    mod._temp_ready = None
                    mod.__dict__["_lazy_temp"] = fn
            if forked:
                main.wait_stream(side)      # norm weights/biases are needed at the very start of the block
                # (the per-linear events above are then already satisfied; LWC-only blocks below overlap more)
            for ln, (tw, tb) in ((nm["ln1"], t1), (nm["ln2"], t2)):
                ln.temp_weight, ln.temp_bias = tw, tb
                ln.use_temporary_parameter = True
        else:
            if forked:
                side.wait_stream(main)
            lazy_mlp = bool(self.__dict__.get("_lazy_mlp_quant")) and not forked
            mlp = set(nm["fc1"]) | {nm["last"]} if lazy_mlp else set()
            with torch.cuda.stream(side):
                dest = self._weight_slabs(nm, dt)      # (allocated on the stream that writes them)
                mods = list(self._quant_linears())
                if os.environ.get("OQ_WQ_ORDER", "1") != "0":       # last-used-first, see _let_temporaries
                    rank = {nm["o"]: 0, nm["v"]: 1, nm["k"]: 2, nm["q"]: 3}
                    mods.sort(key=lambda m: rank.get(m, -1))
                for mod in mods:
                    if mod in mlp:
                        def make(mod=mod):
                            mod.temp_weight, mod.temp_bias = mod.weight_quantizer.quantize(
                                mod.weight, out_dtype=dt, out=dest.get(mod), want_int=mod.int_fprop_eligible(dt)), mod.bias
                        mod.temp_weight, mod.temp_bias = None, None
                        mod.use_temporary_parameter = True
                        mod._temp_ready = None
                        mod.__dict__["_lazy_temp"] = make
                    else:
                        self._publish(mod, mod.weight_quantizer.quantize(mod.weight, out_dtype=dt, out=dest.get(mod),
                                                                         want_int=mod.int_fprop_eligible(dt)), mod.bias, side, forked)

    def clear_temp_variable(self):
        nm = self._let_names()
        for mod in self._quant_linears() + [nm["ln1"], nm["ln2"]]:
            mod.__dict__.pop("_lazy_temp", None)
            if hasattr(mod, "temp_weight"):
                del mod.temp_weight
            if hasattr(mod, "temp_bias"):
                del mod.temp_bias

    @torch.no_grad()
    def smooth_and_quant_inplace(self):
        """Final fold (models/int_llama_layer.py:315-332): weights <- fake_quant(LET(W)) in float32, LET biases
        and norm parameters become buffers."""
        nm = self._let_names()
        if self.let:
            self._truncate_scales()
            wq, bias, t1, t2 = self._let_temporaries(torch.float32)
            for ln, (tw, tb) in ((nm["ln1"], t1), (nm["ln2"], t2)):
                ln.use_temporary_parameter = False
                if hasattr(ln, "bias"):
                    del ln.bias
                ln.register_buffer("bias", tb)
                ln.weight = tw
            for mod in wq:
                if bias[mod] is not None and mod is not nm["last"]:
                    if hasattr(mod, "bias"):
                        del mod.bias
                    mod.register_buffer("bias", bias[mod])
                mod.weight = wq[mod]
                mod.use_temporary_parameter = False
        else:
            for mod in self._quant_linears():
                mod.weight = mod.weight_quantizer.quantize(mod.weight, out_dtype=torch.float32,
                                                           want_int=mod.int_fprop_eligible(self.compute_dtype))
                mod.use_temporary_parameter = False
        for ln in (nm["ln1"], nm["ln2"]):
            ln.use_temporary_parameter = False

    def let_parameters(self, use_shift=True):
        template = "smooth" if use_shift else "smooth_scale"
        return iter([m for n, m in self.named_parameters() if n.find(template) > -1])

    def lwc_parameters(self):
        return iter([m for n, m in self.named_parameters() if n.find("bound_factor") > -1])

    def omni_parameters(self, use_shift=True):
        template = "smooth" if use_shift else "smooth_scale"
        return iter([m for n, m in self.named_parameters()
                     if n.find("bound_factor") > -1 or n.find(template) > -1])

    def omni_state_dict(self, destination=None, prefix="", keep_vars=False):
        if destination is None:
            destination = OrderedDict()
        for name, param in self.named_parameters():
            if name.find("smooth") > -1 or name.find("bound_factor") > -1:
                destination[prefix + name] = param if keep_vars else param.detach()
        return destination

    def register_scales_and_zeros(self):
        for mod in self._quant_linears():
            mod.weight_quantizer.register_scales_and_zeros()
