"""Real-quant packing and inference on the HIP path (`--real_quant`, quantize/omniquant.py:255-278; main.py:364 evaluates
the packed model).

The reference hands every folded QuantLinear to AutoGPTQ's `qlinear_cuda.QuantLinear.pack` (third-party, not vendored:
PARITY UNPINNED, see csrc/oq_pack.hip).  `pack_linear` produces the same buffers (`qweight`, `qzeros`, `scales`, `g_idx`,
`bias`, AutoGPTQ names and shapes) with one HIP kernel.  `PackedLinear` runs straight from them (csrc/oq_packed.hip):
`oq_packed_gemv` for skinny inputs (decode), `oq_packed_gemm` above the row threshold (prefill), and for float32
activations `oq_packed_dequant` + the exact-f32 `oq_gemm`.  `dequantize()` (pure torch) is the value contract the kernels
reproduce.  `pack_block` / `load_packed_block` turn a decoder block into its packed form, whose forward then takes the
weight-only inference path of llama_block.py / opt_block.py.

W4A4 (`act_quant=True`, LLaMA, 4-bit per-channel weights, the 4-bit per-token activation quantisers main.py builds for
--abits 4): the same buffers, but every PackedLinear has act_bits = 4 and contracts the activation quantiser's integer codes
with the packed weight codes (csrc/oq_packed_a4.hip): `oq_packed_gemv_a4` up to GEMV_A4_MAX_ROWS rows, else
`oq_packed_codes` + `oq_gemm_i8`.  The value is the exact product of the two grids."""
import os

import torch
import torch.nn as nn

from . import _capi as C

#: rows up to which PackedLinear takes oq_packed_gemv (set by tools/microbench_packed.py)
GEMV_MAX_ROWS = int(os.environ.get("OQ_PACKED_GEMV_ROWS", "16"))
#: bf16 prefill through oq_packed_dequant + oq_gemm instead of oq_packed_gemm (the faster of the two at M = 2048, measured)
PREFILL_BF16_DEQUANT = os.environ.get("OQ_PACKED_PREFILL_DEQUANT", "1") != "0"
#: rows up to which an act_bits = 4 PackedLinear takes oq_packed_gemv_a4, above: oq_packed_codes + oq_gemm_i8 (set by
#: tools/microbench_packed_a4.py)
GEMV_A4_MAX_ROWS = int(os.environ.get("OQ_PACKED_A4_GEMV_ROWS", "16"))


def pack_linear(weight, scales, zeros, bits, group_size=None, bias=None):
    """weight [out,in] = folded fake-quant weight; scales/zeros [out*groups,1] or [out,groups] (the `scales`/`zeros`
    buffers `register_scales_and_zeros` creates).  Returns a dict of AutoGPTQ-style buffers."""
    if not weight.is_cuda:
        raise C.OQError("pack_linear: GPU tensors expected (no CPU fallback)")
    out, inn = weight.shape
    group = group_size or inn
    ng = inn // group
    w = weight.detach().contiguous()
    s = scales.detach().float().reshape(out, ng).contiguous()
    z = zeros.detach().float().reshape(out, ng).contiguous()
    qweight = torch.empty((inn // 32 * bits, out), dtype=torch.int32, device=w.device)
    qzeros = torch.empty((ng, out // 32 * bits), dtype=torch.int32, device=w.device)
    C.call("oq_pack_weights", C.ptr(w), C.dt(w), out, inn, group, bits, C.fptr(s), C.fptr(z), C.ptr(qweight), C.ptr(qzeros),
           C.stream())
    g_idx = (torch.arange(inn, device=w.device, dtype=torch.int32) // group)
    return dict(qweight=qweight, qzeros=qzeros, scales=s.t().contiguous().half(), g_idx=g_idx,
                bias=None if bias is None else bias.detach().half())


def unpack(q, bits, n):
    """Inverse of the AutoGPTQ word packing along dim 0: q [n/32*bits, m] int32 -> codes [n, m] int64."""
    qu = q.to(torch.int64) & 0xFFFFFFFF
    m = qu.shape[1]
    if bits != 3:
        per = 32 // bits
        sh = torch.arange(per, device=q.device, dtype=torch.int64) * bits
        codes = (qu[:, None, :] >> sh[None, :, None]) & ((1 << bits) - 1)
        return codes.reshape(-1, m)[:n]
    w3 = qu.reshape(-1, 3, m)
    a, b, c = w3[:, 0], w3[:, 1], w3[:, 2]
    cols = []
    for j in range(10):
        cols.append((a >> (3 * j)) & 7)
    cols.append(((a >> 30) & 3) | ((b & 1) << 2))
    for j in range(10):
        cols.append((b >> (3 * j + 1)) & 7)
    cols.append(((b >> 31) & 1) | ((c & 3) << 1))
    for j in range(10):
        cols.append((c >> (3 * j + 2)) & 7)
    return torch.stack(cols, dim=1).reshape(-1, m)[:n]


class PackedLinear(nn.Module):
    """AutoGPTQ-layout linear (buffers qweight / qzeros / scales / g_idx / bias, AutoGPTQ's names, shapes and dtypes).

    forward(x, residual=None) = x @ W^T (+ bias) (+ residual), W = dequantize() -- fp16 x: exactly that weight; bf16 x: that
    weight rounded to bf16 (the bf16 MFMA operand); float32 x: the fp16 weight widened exactly, contracted
    in exact f32.  Inference only: the packed weights have no gradient and no gradient is propagated to x either (a call
    that would need one raises OQError; a calibrated block is trained before packing, never after).

    act_bits = 4 (4-bit per-channel weights only): the input is quantised per token on the 4-bit asymmetric grid
    (quantize/quantizer.py:84-147) and the layer returns s_a s_w sum_k (q_a - z_a)(q_w - z_w) + bias (+ residual), the exact
    product of the two grids, contracted in integers (forward_codes); float32 or bfloat16 inputs and outputs."""

    def __init__(self, bits, group_size, in_features, out_features, packed, act_bits=16):
        super().__init__()
        self.bits, self.group_size, self.infeatures, self.outfeatures = bits, group_size or in_features, in_features, out_features
        _check_shape(bits, self.group_size, in_features, out_features)
        self.act_bits = int(act_bits)
        if self.act_bits not in (4, 16):
            raise C.OQError(f"PackedLinear: act_bits {act_bits} (16 = weight-only, or 4)")
        if self.act_bits == 4 and (bits != 4 or self.group_size != in_features):
            raise C.OQError(f"PackedLinear: act_bits 4 needs 4-bit per-channel weights (got {bits} bit, group {self.group_size})")
        for k, v in packed.items():
            if v is not None:
                self.register_buffer(k, v)
            else:
                setattr(self, k, None)
        self._check_g_idx()

    @classmethod
    def empty(cls, bits, group_size, in_features, out_features, bias, device, act_bits=16):
        """Buffers of the right shapes / dtypes (uninitialised, g_idx = the trivial grouping) that a saved state_dict() of a
        PackedLinear loads into.  bias: True / False (or a tensor / None)."""
        group = group_size or in_features
        _check_shape(bits, group, in_features, out_features)
        packed = dict(qweight=torch.zeros((in_features // 32 * bits, out_features), dtype=torch.int32, device=device),
                      qzeros=torch.zeros((in_features // group, out_features // 32 * bits), dtype=torch.int32, device=device),
                      scales=torch.zeros((in_features // group, out_features), dtype=torch.float16, device=device),
                      g_idx=torch.arange(in_features, dtype=torch.int32, device=device) // group,
                      bias=torch.zeros((out_features,), dtype=torch.float16, device=device) if bias is not None and bias is not False
                      else None)
        return cls(bits, group, in_features, out_features, packed, act_bits=act_bits)

    def _check_g_idx(self):
        """Only the trivial grouping g_idx = arange(in) // group: act-order (a permuted g_idx) has no kernel.  Checked when the
        buffers are set (construction, load_state_dict), never per call."""
        g = self.g_idx
        want = torch.arange(self.infeatures, device=g.device, dtype=torch.int64) // self.group_size
        if tuple(g.shape) != (self.infeatures,) or not torch.equal(g.long(), want):
            raise C.OQError("PackedLinear: g_idx is not arange(in) // group_size (act-order / desc_act is not supported)")

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._check_g_idx()

    def dequantize(self):
        """fp16 weight [out, in] = scales * (q - (qzeros + 1))  (AutoGPTQ's dequantisation)."""
        q = unpack(self.qweight, self.bits, self.infeatures)                              # [in, out]
        z = unpack(self.qzeros.t().contiguous(), self.bits, self.outfeatures).t() + 1      # [groups, out]
        g = self.g_idx.long()
        w = self.scales.float()[g] * (q - z[g]).float()
        return w.t().contiguous().half()

    def dequantize_hip(self, dtype=torch.float16):
        """dequantize() on the GPU (oq_packed_dequant), in float16 (bit-exact), bfloat16 or float32."""
        if not self.qweight.is_cuda:
            raise C.OQError("PackedLinear: GPU buffers expected (no CPU fallback)")
        w = torch.empty((self.outfeatures, self.infeatures), dtype=dtype, device=self.qweight.device)
        C.call("oq_packed_dequant", C.ptr(self.qweight), C.ptr(self.qzeros), C.ptr(self.scales), self.infeatures,
               self.outfeatures, self.group_size, self.bits, C.ptr(w), C.dt(w), C.stream())
        return w

    # ---- act_bits = 4: integer path ------------------------------------------------------------------------------------
    def weight_codes(self):
        """ops.IntCodes of the weight (oq_packed_codes): int8 codes [out, in], s_w, z_w = qzeros + 1, Cw [out]."""
        if not self.qweight.is_cuda:
            raise C.OQError("PackedLinear: GPU buffers expected (no CPU fallback)")
        from . import ops
        N, K = self.outfeatures, self.infeatures
        codes = torch.empty((N, K), dtype=torch.int8, device=self.qweight.device)
        vec = torch.empty((3, N), dtype=torch.float32, device=self.qweight.device)
        C.call("oq_packed_codes", C.ptr(self.qweight), C.ptr(self.qzeros), C.ptr(self.scales), K, N, C.ptr(codes), C.fptr(vec[0]),
               C.fptr(vec[1]), C.fptr(vec[2]), C.stream())
        return ops.IntCodes(codes, vec[0], vec[1], vec[2], 4)

    def _check_input(self, x, dtypes, what, allowed):
        """The one input check: a GPU tensor that needs no gradient, with the layer's feature count, in one of `dtypes`
        (`what` and `allowed` word the dtype message)."""
        if not x.is_cuda or not self.qweight.is_cuda:
            raise C.OQError("PackedLinear: the HIP path needs GPU tensors (got a CPU tensor); there is no CPU fallback")
        if torch.is_grad_enabled() and x.requires_grad:
            raise C.OQError("PackedLinear is inference-only: no gradient through a packed weight (run under torch.no_grad())")
        if x.shape[-1] != self.infeatures:
            raise C.OQError(f"PackedLinear: input has {x.shape[-1]} features, the layer {self.infeatures}")
        if x.dtype not in dtypes:
            raise C.OQError(f"PackedLinear{what} {x.dtype} ({allowed})")

    def _check_a4_input(self, x):
        if self.act_bits != 4:
            raise C.OQError("PackedLinear: integer-code inputs need act_bits = 4")
        self._check_input(x, (torch.float32, torch.bfloat16), " (act_bits 4): activation dtype",
                          "float32 or bfloat16; the blocks convert float16 hidden states to their compute dtype on entry")

    def quantize_input(self, x):
        """ops.IntCodes of the per-token 4-bit quantiser applied to x [..., in] (float32 / bfloat16)."""
        self._check_a4_input(x)
        from . import ops
        return ops.act_codes(x.reshape(-1, self.infeatures), self.act_bits)

    def forward_codes(self, xint, residual=None, out_dtype=torch.bfloat16):
        """y [M, out] in out_dtype (float32 / bfloat16) from the activation codes xint (ops.IntCodes, 4-bit, [M, in])."""
        from . import ops
        if self.act_bits != 4 or xint.nbits != 4:
            raise C.OQError(f"PackedLinear.forward_codes: {xint.nbits}-bit codes into an act_bits {self.act_bits} layer")
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise C.OQError(f"PackedLinear (act_bits 4): output dtype {out_dtype} (float32 or bfloat16)")
        codes = xint.codes
        if codes.dim() != 2:
            raise C.OQError(f"PackedLinear.forward_codes: codes {tuple(codes.shape)} (expected [M, {self.infeatures}])")
        self._check_input(codes, (torch.int8,), ".forward_codes: codes dtype", "int8")
        M, K, N = codes.shape[0], self.infeatures, self.outfeatures
        res2 = None
        if residual is not None:
            if residual.dtype not in (torch.float32, torch.bfloat16) or residual.numel() != M * N:
                raise C.OQError("PackedLinear: residual must be float32 / bfloat16 of the output's size")
            res2 = residual.reshape(M, N).contiguous()
        y = torch.empty((M, N), dtype=out_dtype, device=codes.device)
        if M == 0:
            return y
        if M <= GEMV_A4_MAX_ROWS:
            ws_n = C.size_call("oq_packed_gemv_a4_workspace", M, K, N)
            ws = torch.empty(ws_n, dtype=torch.uint8, device=codes.device) if ws_n else None
            C.call("oq_packed_gemv_a4", C.ptr(codes.contiguous()), C.fptr(xint.scale), C.fptr(xint.zp), C.fptr(xint.csum), M, K, N,
                   C.ptr(self.qweight), C.ptr(self.qzeros), C.ptr(self.scales), C.ptr(self.bias), C.ptr(res2),
                   C.dt(res2) if res2 is not None else 0, C.ptr(y), C.dt(y), C.ptr(ws), ws_n, C.stream())
        else:
            # prefill: the weight codes into a transient buffer, then the int8 MFMA GEMM (the W4A16 dequant + oq_gemm route's twin)
            b32 = None if self.bias is None else self.bias.float().contiguous()
            ops.gemm_i8(ops.IntCodes(codes.contiguous(), xint.scale, xint.zp, xint.csum, 4), self.weight_codes(), y, bias=b32,
                        addend=res2)
        return y

    def forward(self, x, residual=None):
        if self.act_bits == 4:
            self._check_a4_input(x)
            y = self.forward_codes(self.quantize_input(x), residual, x.dtype)
            return y.view(*x.shape[:-1], self.outfeatures)
        self._check_input(x, (torch.float16, torch.bfloat16, torch.float32), ": activation dtype", "float16, bfloat16 or float32")
        K, N = self.infeatures, self.outfeatures
        x2 = x.reshape(-1, K).contiguous()
        M = x2.shape[0]
        res2 = None
        if residual is not None:
            if residual.dtype != x.dtype or residual.numel() != M * N:
                raise C.OQError("PackedLinear: residual must have the output's dtype and size")
            res2 = residual.reshape(M, N).contiguous()
        y = torch.empty((M, N), dtype=x.dtype, device=x.device)
        if M == 0:
            return y.view(*x.shape[:-1], N)
        from . import ops
        if x.dtype == torch.float32 or (x.dtype == torch.bfloat16 and M > GEMV_MAX_ROWS and PREFILL_BF16_DEQUANT):
            # dequantise once into a dense temporary, then the resident-weight GEMM (exact f32 MFMA in parity mode)
            w = self.dequantize_hip(x.dtype)
            b32 = None if self.bias is None else self.bias.float().contiguous()
            ops.gemm(x2, w, y, M, N, K, K, K, N, True, True, bias=b32, addend=res2)
        elif M <= GEMV_MAX_ROWS:
            ws_n = C.size_call("oq_packed_gemv_workspace", M, K, N, self.bits)
            ws = torch.empty(ws_n, dtype=torch.uint8, device=x.device) if ws_n else None
            C.call("oq_packed_gemv", C.ptr(x2), C.dt(x2), M, K, N, self.group_size, self.bits, C.ptr(self.qweight),
                   C.ptr(self.qzeros), C.ptr(self.scales), C.ptr(self.bias), C.ptr(res2), C.ptr(y), C.ptr(ws), ws_n, C.stream())
        else:
            C.call("oq_packed_gemm", C.ptr(x2), C.dt(x2), M, K, N, self.group_size, self.bits, C.ptr(self.qweight),
                   C.ptr(self.qzeros), C.ptr(self.scales), C.ptr(self.bias), C.ptr(res2), C.ptr(y), C.stream())
        return y.view(*x.shape[:-1], N)


def _check_shape(bits, group, inn, out):
    if bits not in (2, 3, 4, 8):
        raise C.OQError(f"PackedLinear: bits {bits} (2, 3, 4 or 8)")
    if inn <= 0 or out <= 0 or inn % 32 or out % 32:
        raise C.OQError(f"PackedLinear: in={inn} out={out} (multiples of 32)")
    if group <= 0 or inn % group or (group != inn and group % 32):
        raise C.OQError(f"PackedLinear: group {group} (in={inn}, or a divisor of it that is a multiple of 32)")


def _act_bits(qlayer):
    """Smallest activation bit width the block's quantisers were built with (16 = none acts: weight-only)."""
    from .linear import QuantLinear
    from .matmul import QuantMatMul
    bits = [16]
    for m in qlayer.modules():
        if isinstance(m, QuantLinear) and m.act_quantizer is not None and not m.disable_input_quant:
            bits.append(m.act_quantizer.n_bits)
        elif isinstance(m, QuantMatMul):
            bits += [m.x1_quantizer.n_bits, m.x2_quantizer.n_bits]
    return min(bits)


def _replace_module(root, name, new):
    """Put `new` where root.get_submodule(name) is."""
    parent, _, leaf = name.rpartition(".")
    setattr(root.get_submodule(parent), leaf, new)


def _mark_packed(qlayer, act_bits, act_quant=False, kv_cache_bits=None):
    """The block's forward checks this once at entry and takes the packed inference path (block_common.packed_guard).
    kv_cache_bits (None, 4 or 8): the storage kind of the KV caches the block creates (kvcache.PackedKVCache code_bits)."""
    qlayer._oq_packed = {"act_bits": int(act_bits), "act_quant": bool(act_quant), "kv_cache_bits": kv_cache_bits}


def _check_kv_cache_bits(kv_cache_bits, act_quant):
    if kv_cache_bits is None:
        return
    if kv_cache_bits == 8:
        if act_quant:
            raise C.OQError("kv_cache_bits=8 is the weight-only blocks' code cache; an act_quant=True (W4A4) block's k / v sit on "
                            "its 4-bit head grid (kv_cache_bits=4)")
        return
    if kv_cache_bits != 4:
        raise C.OQError(f"kv_cache_bits {kv_cache_bits} (None: float rows, 4 with act_quant=True, or 8 without)")
    if not act_quant:
        raise C.OQError("kv_cache_bits=4 needs act_quant=True: a weight-only block's k / v are not on a 4-bit grid, and quantising "
                        "them for the cache would change the model")


def _check_a4_quantizer(name, q, bits):
    """The per-token quantiser main.py builds for --abits 4 (main.py:276-299), or a 16-bit identity when bits == 16."""
    if bits == 16:
        if q is not None and q.enable and q.n_bits < 16:
            raise C.OQError(f"act_quant=True: {name} is {q.n_bits}-bit; the attention probabilities must stay 16-bit")
        return
    if q is None:
        raise C.OQError(f"act_quant=True: {name} is missing (the input quantiser is disabled)")
    why = []
    if q.n_bits != 4:
        why.append(f"{q.n_bits}-bit")
    if q.symmetric:
        why.append("symmetric")
    if q.dynamic_method != "per_token":
        why.append(f"dynamic_method {q.dynamic_method}")
    if q.lwc:
        why.append("LWC")
    if q.group_size:
        why.append(f"group {q.group_size}")
    if q.metric == "fix0to1":
        why.append("metric fix0to1")
    if not q.enable:
        why.append("disabled")
    if why:
        raise C.OQError(f"act_quant=True: {name} is {', '.join(why)}; the W4A4 packed path needs the 4-bit asymmetric dynamic "
                        "per-token quantiser (--abits 4)")


def check_act_quant_eligible(qlayer, wbits, group_size=None):
    """Raise OQError naming the offending module unless the block can run the W4A4 packed path: a LLaMA block, 4-bit
    per-channel weights, 4-bit asymmetric dynamic per-token quantisers on every linear's input and on q / k / v
    (qkt_matmul.x1 / x2, pv_matmul.x2), the 16-bit probability quantiser (pv_matmul.x1).  group_size: the packing's group
    (None: each QuantLinear's own weight quantiser's)."""
    from .linear import QuantLinear
    from .llama_block import QuantLlamaDecoderLayer
    from .matmul import QuantMatMul
    if not isinstance(qlayer, QuantLlamaDecoderLayer):
        raise C.OQError(f"act_quant=True: {type(qlayer).__name__} is not a LLaMA block (W4A4 packed inference covers LLaMA only)")
    if wbits != 4:
        raise C.OQError(f"act_quant=True: {wbits}-bit weights (the W4A4 packed path needs wbits 4)")
    for name, m in qlayer.named_modules():
        if isinstance(m, QuantLinear):
            g = group_size if group_size is not None else m.weight_quantizer.group_size
            if g and g != m.in_features:
                raise C.OQError(f"act_quant=True: {name} has grouped weights (group {g}); the W4A4 packed path is per-channel")
            _check_a4_quantizer(name + ".act_quantizer", None if m.disable_input_quant else m.act_quantizer, 4)
        elif isinstance(m, QuantMatMul):
            leaf = name.split(".")[-1]
            if leaf == "qkt_matmul":
                _check_a4_quantizer(name + ".x1_quantizer", m.x1_quantizer, 4)
                _check_a4_quantizer(name + ".x2_quantizer", m.x2_quantizer, 4)
            elif leaf == "pv_matmul":
                _check_a4_quantizer(name + ".x1_quantizer", m.x1_quantizer, 16)
                _check_a4_quantizer(name + ".x2_quantizer", m.x2_quantizer, 4)


def pack_block(qlayer, wbits, act_quant=False, kv_cache_bits=None):
    """Replace every folded QuantLinear of a calibrated block by a PackedLinear (quantize/omniquant.py:255-278) and mark the
    block packed: its forward then runs the weight-only inference path.  act_quant=True (W4A4 LLaMA blocks,
    check_act_quant_eligible): the same buffers -- the state_dict is the weight-only pack's -- with act_bits 4 linears, and
    the forward runs the integer path (llama_block.QuantLlamaDecoderLayer._packed_forward_a4).  kv_cache_bits=4 (with
    act_quant=True): the block's KV caches store the head quantisers' 4-bit codes (kvcache.PackedKVCache code_bits); the values
    the attention reads are the same.  kv_cache_bits=8 (weight-only blocks, LLaMA and OPT): the block's KV caches store 8-bit
    per-(token, head) codes of k / v (PackedKVCache code_bits=8) and every attention, the prefill's included, reads the
    dequantised rows: a lossy cache, 136 instead of 256 / 512 bytes per head row of 128."""
    from .linear import QuantLinear
    _check_kv_cache_bits(kv_cache_bits, act_quant)
    act_bits = _act_bits(qlayer)
    if act_quant:
        check_act_quant_eligible(qlayer, wbits)
    for name, module in list(qlayer.named_modules()):
        if not isinstance(module, QuantLinear):
            continue
        wq = module.weight_quantizer
        packed = pack_linear(module.weight.float(), wq.scales, wq.zeros, wbits, wq.group_size, module.bias)
        _replace_module(qlayer, name, PackedLinear(wbits, wq.group_size, module.in_features, module.out_features, packed,
                                                   act_bits=4 if act_quant else 16))
    _mark_packed(qlayer, act_bits, act_quant, kv_cache_bits)
    return qlayer


def load_packed_block(qlayer, state_dict, wbits, group_size, act_quant=False, kv_cache_bits=None):
    """Turn a fresh Quant*DecoderLayer (built from the model's layer and the run's args, not calibrated) into the packed block
    whose state_dict() this is, without recalibrating: every QuantLinear becomes an empty PackedLinear, the LET-folded norm
    biases get their buffers, then the state dict is loaded (float LET / LWC learnables it still holds are not needed for
    inference and are ignored; any missing tensor is an error)."""
    from .linear import QuantLinear
    from .norm import OmniLayerNorm, OmniLlamaRMSNorm
    _check_kv_cache_bits(kv_cache_bits, act_quant)
    act_bits = _act_bits(qlayer)
    if act_quant:
        check_act_quant_eligible(qlayer, wbits, group_size or 0)
    for name, module in list(qlayer.named_modules()):
        if isinstance(module, QuantLinear):
            _replace_module(qlayer, name, PackedLinear.empty(wbits, group_size, module.in_features, module.out_features,
                                                             (name + ".bias") in state_dict, module.weight.device,
                                                             act_bits=4 if act_quant else 16))
        elif isinstance(module, (OmniLayerNorm, OmniLlamaRMSNorm)) and module.bias is None and (name + ".bias") in state_dict:
            ref = state_dict[name + ".bias"]
            del module.bias
            module.register_buffer("bias", torch.empty(ref.shape, dtype=ref.dtype, device=module.weight.device))
    missing, _ = qlayer.load_state_dict(state_dict, strict=False)
    if missing:
        raise C.OQError(f"load_packed_block: the state dict lacks {missing}")
    _mark_packed(qlayer, act_bits, act_quant, kv_cache_bits)
    return qlayer
