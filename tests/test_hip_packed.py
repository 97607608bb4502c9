"""Real-quant inference on the packed AutoGPTQ buffers (csrc/oq_packed.hip, realquant.PackedLinear, the packed path of the
decoder blocks).  The value contract is PackedLinear.dequantize(): the kernels must reproduce that fp16 weight (rounded once
more to bf16 for bf16 activations) and contract it in fp32."""
import copy
import math

import pytest
import torch

from omniquant_amd import OQError
from omniquant_amd import _capi as C
from omniquant_amd import realquant as RQ
from omniquant_amd.realquant import PackedLinear, load_packed_block, pack_block

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}


def _rand_packed(bits, group, inn, out, bias=True, seed=0, device=DEV):
    """Random int32 words: every code value and every stored zero (including zero - 1 = -1, the wrap to 2^bits) occurs."""
    g = torch.Generator().manual_seed(seed)
    ng = inn // group
    p = dict(qweight=torch.randint(-2 ** 31, 2 ** 31, (inn // 32 * bits, out), generator=g, dtype=torch.int64).to(torch.int32),
             qzeros=torch.randint(-2 ** 31, 2 ** 31, (ng, out // 32 * bits), generator=g, dtype=torch.int64).to(torch.int32),
             scales=((torch.rand(ng, out, generator=g) + 0.5) * (0.5 / (1 << bits))).half(),
             g_idx=torch.arange(inn, dtype=torch.int32) // group,
             bias=torch.randn(out, generator=g).half() if bias else None)
    return PackedLinear(bits, group, inn, out, {k: (None if v is None else v.to(device)) for k, v in p.items()})


@pytest.mark.parametrize("bits", [2, 3, 4, 8])
@pytest.mark.parametrize("group", [None, 32, 64, 128])
def test_dequant_bit_exact_with_dequantize(bits, group):
    inn, out = 256, 96
    pl = _rand_packed(bits, group or inn, inn, out, seed=bits * 10 + (group or 0))
    ref = pl.dequantize()
    w16 = pl.dequantize_hip(torch.float16)
    assert torch.equal(w16.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(pl.dequantize_hip(torch.float32), ref.float())
    assert torch.equal(pl.dequantize_hip(torch.bfloat16), ref.bfloat16())


def _check_forward(pl, x, residual):
    with torch.no_grad():
        y = pl(x, residual=residual)
    w = pl.dequantize()
    w = (w.bfloat16() if x.dtype == torch.bfloat16 else w).double()
    ref = x.double().reshape(-1, pl.infeatures) @ w.T
    if pl.bias is not None:
        ref = ref + pl.bias.double()
    if residual is not None:
        ref = ref + residual.double().reshape(ref.shape)
    mag = x.double().abs().reshape(-1, pl.infeatures) @ w.abs().T
    assert y.dtype == x.dtype and y.shape == (*x.shape[:-1], pl.outfeatures)
    err = (y.double().reshape(ref.shape) - ref).abs()
    bound = UNIT[x.dtype] * ref.abs() + 1e-5 * mag
    assert bool(torch.isfinite(y).all())
    assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("bits,group,inn,out", [(4, 32, 96, 160), (3, 416, 416, 96), (2, 32, 416, 64), (8, 64, 256, 288),
                                                (4, 128, 512, 256)])
def test_forward_matches_dequantized_reference(dtype, bits, group, inn, out):
    """every M on both sides of the gemv / gemm threshold (RQ.GEMV_MAX_ROWS), in values that are not tile multiples."""
    pl = _rand_packed(bits, group, inn, out, bias=(bits != 2), seed=inn + out + bits)
    g = torch.Generator().manual_seed(3)
    ms = sorted({1, 3, 8, 16, 17, 64, 300, RQ.GEMV_MAX_ROWS, RQ.GEMV_MAX_ROWS + 1})
    for M in ms:
        x = torch.randn(M, inn, generator=g).to(dtype).to(DEV)
        res = torch.randn(M, out, generator=g).to(dtype).to(DEV) if M % 2 else None
        _check_forward(pl, x, res)
    x3 = torch.randn(2, 5, inn, generator=g).to(dtype).to(DEV)         # leading dims are flattened and restored
    _check_forward(pl, x3, torch.randn(2, 5, out, generator=g).to(dtype).to(DEV))


@pytest.mark.parametrize("bits,group,inn,out", [(4, 32, 96, 160), (3, 416, 416, 96), (8, 64, 256, 288)])
def test_bf16_packed_gemm_kernel(bits, group, inn, out, monkeypatch):
    """bf16 prefill dispatches to oq_packed_dequant + oq_gemm (faster); oq_packed_gemm's bf16 variant
    must still meet the same contract when chosen."""
    monkeypatch.setattr(RQ, "PREFILL_BF16_DEQUANT", False)
    pl = _rand_packed(bits, group, inn, out, seed=inn * bits)
    g = torch.Generator().manual_seed(4)
    for M in (RQ.GEMV_MAX_ROWS + 1, 64, 300):
        _check_forward(pl, torch.randn(M, inn, generator=g).to(torch.bfloat16).to(DEV),
                       torch.randn(M, out, generator=g).to(torch.bfloat16).to(DEV))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("prefill_dequant", [True, False])
def test_forward_prefill_2048x4096x4096(dtype, prefill_dequant, monkeypatch):
    monkeypatch.setattr(RQ, "PREFILL_BF16_DEQUANT", prefill_dequant)
    pl = _rand_packed(4, 128, 4096, 4096, seed=7)
    x = torch.randn(2048, 4096, generator=torch.Generator().manual_seed(8)).to(dtype).to(DEV)
    _check_forward(pl, x, None)


@pytest.mark.parametrize("M", [4, 256])
def test_two_launches_are_bit_identical(M):
    """gemv (split contraction, partials summed in a fixed order) and gemm: no atomics, the same bits every launch."""
    pl = _rand_packed(3, 128, 4096, 1024, seed=M)
    for dtype in (torch.float16, torch.bfloat16):
        x = torch.randn(M, 4096, generator=torch.Generator().manual_seed(M)).to(dtype).to(DEV)
        with torch.no_grad():
            a, b = pl(x), pl(x)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_kernel_argument_errors_are_loud():
    """out % 32 != 0, an unsupported bit width and a group that does not divide `in` are refused by the C ABI itself
    (OQ_E_ARG -> OQError), before any launch."""
    pl = _rand_packed(4, 64, 256, 64, seed=1)
    x = torch.randn(4, 256, device=DEV, dtype=torch.float16)
    y = torch.empty(4, 64, device=DEV, dtype=torch.float16)
    bufs = (C.ptr(pl.qweight), C.ptr(pl.qzeros), C.ptr(pl.scales))
    for out, bits, group in ((48, 4, 64), (64, 5, 64), (64, 4, 96), (64, 4, 48)):
        with pytest.raises(OQError):
            C.call("oq_packed_gemv", C.ptr(x), C.dt(x), 4, 256, out, group, bits, *bufs, None, None, C.ptr(y), None, 0, C.stream())
        with pytest.raises(OQError):
            C.call("oq_packed_gemm", C.ptr(x), C.dt(x), 4, 256, out, group, bits, *bufs, None, None, C.ptr(y), C.stream())
        with pytest.raises(OQError):
            C.call("oq_packed_dequant", *bufs, 256, out, group, bits, C.ptr(y), C.dt(y), C.stream())
    with pytest.raises(OQError):          # gemv beyond its row limit
        C.call("oq_packed_gemv", C.ptr(x), C.dt(x), 17, 256, 64, 64, 4, *bufs, None, None, C.ptr(y), None, 0, C.stream())
    with pytest.raises(OQError):
        pl(x.float().requires_grad_())     # inference only
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------------------------------
def _calibrated(family, H, T, heads, kv_heads, wbits, group, abits=16, epochs=1, seed=2):
    from omniquant_amd.calibrate import calibrate_layers, default_args
    from omniquant_amd.synthetic import causal_mask, make_calib_inputs, make_config, make_layer
    cfg = make_config(None, family=family, hidden_size=H, inter=2 * H, heads=heads, kv_heads=kv_heads)
    args = default_args(wbits=wbits, abits=abits, group_size=group, lwc=True, let=False, epochs=epochs, nsamples=2, net=family,
                        real_quant=False)
    x = make_calib_inputs(2, T, H, dtype=torch.float16).to(DEV)
    mask = causal_mask(T).to(DEV)
    pos = torch.arange(T, device=DEV)[None] if family == "llama" else None
    # no outlier columns: a group whose minimum sits within half a step of zero gets zero point 0, AutoGPTQ stores it as
    # zero - 1 = -1 and that word's all-ones pattern overwrites its neighbours' zeros -- the packed weight then differs from
    # the fake-quant one by design (the contract the kernels keep, exercised by the random words above)
    layer = make_layer(cfg, seed=seed, device=DEV, outliers=False)
    qlayers, _, _, _ = calibrate_layers([layer], cfg, args, x, mask, pos, use_graph=False)
    return cfg, args, qlayers[0], mask, pos


def _run(block, x, mask, pos):
    kw = dict(attention_mask=mask)
    if pos is not None:
        kw["position_ids"] = pos
    with torch.no_grad():
        return block(x, **kw)[0]


def _oracle(family, cfg, packed, x, mask, pos):
    """oracle.ref_cpu.Block on the packed block's dequantised weights, fp32, under a spec whose quantisers are identities."""
    from oracle import ref_cpu as R
    w = {}
    for name, m in packed.named_modules():
        if isinstance(m, PackedLinear):
            w[name + ".weight"] = m.dequantize().float().cpu()
            if m.bias is not None:
                w[name + ".bias"] = m.bias.float().cpu()
        elif name.endswith("layernorm") or name.endswith("layer_norm"):
            w[name + ".weight"] = m.weight.float().cpu()
            if getattr(m, "bias", None) is not None:
                w[name + ".bias"] = m.bias.float().cpu()
    cd = dict(hidden_size=cfg.hidden_size, num_attention_heads=cfg.num_attention_heads,
              num_key_value_heads=getattr(cfg, "num_key_value_heads", None) or cfg.num_attention_heads)
    if family == "llama":
        cd["rms_norm_eps"] = cfg.rms_norm_eps
    spec = R.QuantSpec(16, 16, None, False, False)
    probe = torch.randn(8, 64)
    assert torch.equal(R.fake_quant(probe, spec.wbits), probe) and torch.equal(R.fake_quant(probe, spec.abits), probe)
    blk = R.Block(family, cd, w, spec, max_pos=x.shape[1])
    with torch.no_grad():
        return blk.forward(x.float().cpu(), mask.cpu(), None if pos is None else pos.cpu(), None, act_quant=False)


def _block_parity(family, H, T, heads, kv_heads, wbits, group):
    from omniquant_amd.synthetic import make_calib_inputs
    cfg, args, fq, mask, pos = _calibrated(family, H, T, heads, kv_heads, wbits, group)
    pk = pack_block(copy.deepcopy(fq), wbits)
    assert sum(isinstance(m, PackedLinear) for m in pk.modules()) == (7 if family == "llama" else 6)
    fq_w = {n: m.weight.float() for n, m in fq.named_modules() if hasattr(m, "weight_quantizer")}
    for n, m in pk.named_modules():
        if isinstance(m, PackedLinear):     # premise of the comparison: the weights differ by the fp16 scales only
            assert float((m.dequantize().float() - fq_w[n]).abs().max()) <= 2e-3 * float(fq_w[n].abs().max()), n
    x = make_calib_inputs(1, T, H, seed=11, dtype=torch.float16).to(DEV)          # fresh inputs, not the calibration set
    a, b = _run(pk, x, mask, pos).float(), _run(fq, x, mask, pos).float()
    assert a.shape == b.shape == x.shape and bool(torch.isfinite(a).all())
    cos = float(torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0))
    # The two blocks' weights differ by the fp16 rounding of the scales and of the dequantised value (<= 2^-10 relative, what
    # test_real_quant_packing bounds); both then round their weight to bf16 and run the same bf16 kernels, and a weight that
    # lands on the other side of a bf16 rounding boundary moves by one bf16 ulp (2^-8).  Every output element is a bf16
    # rounding of a sum over the hidden state: a few bf16 ulps of the output's magnitude, i.e. about 1e-2 of its maximum.
    assert cos >= 0.9999, cos
    assert float((a - b).abs().max()) <= 2e-2 * float(b.abs().max())
    # fp32 parity mode of the packed block vs the oracle on the very same weights
    pk.compute_dtype = torch.float32
    y32 = _run(pk, x.float(), mask, pos).cpu()
    ref = _oracle(family, cfg, pk, x, mask, pos)
    assert float((y32 - ref).abs().max()) <= 1e-3 * float(ref.abs().max())
    return cfg, args, pk, mask, pos, x


LLAMA_SHAPES = {"base": (256, 64, 2, 2), "gqa": (256, 64, 4, 2), "hd128_fused": (256, 256, 2, 2)}


@pytest.mark.parametrize("wbits,group", [(4, 64), (3, 128), (2, 64)])
@pytest.mark.parametrize("shape", list(LLAMA_SHAPES))
def test_llama_block_packed_parity(wbits, group, shape, monkeypatch):
    H, T, nh, nkv = LLAMA_SHAPES[shape]
    cfg, args, pk, mask, pos, x = _block_parity("llama", H, T, nh, nkv, wbits, group)
    if shape == "hd128_fused":
        from omniquant_amd import ops
        calls = []
        orig = ops.FusedCausalAttnFn.apply
        monkeypatch.setattr(ops.FusedCausalAttnFn, "apply", lambda *a: calls.append(1) or orig(*a))
        pk.compute_dtype = torch.bfloat16
        _run(pk, x, mask, pos)
        assert calls, "the hd-128 / T-256 packed block should take the fused causal attention"


@pytest.mark.parametrize("wbits,group", [(4, 64), (3, 128)])
def test_opt_block_packed_parity(wbits, group):
    _block_parity("opt", 256, 64, 4, 4, wbits, group)


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_load_packed_block_is_bit_identical(family):
    from omniquant_amd.calibrate import decoder_layer_class
    from omniquant_amd.synthetic import make_layer
    cfg, args, pk, mask, pos, x = _block_parity(family, 256, 64, 4, 2 if family == "llama" else 4, 4, 64)
    pk.compute_dtype = torch.bfloat16
    sd = {k: v.clone() for k, v in pk.state_dict().items()}
    fresh = decoder_layer_class(family)(cfg, make_layer(cfg, seed=99, device=DEV), args).to(DEV)
    load_packed_block(fresh, sd, 4, 64)
    a, b = _run(fresh, x, mask, pos), _run(pk, x, mask, pos)
    assert a.dtype == b.dtype == torch.float16
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_packed_block_with_activation_quantisers_is_refused():
    from omniquant_amd.synthetic import make_calib_inputs
    cfg, args, fq, mask, pos = _calibrated("llama", 256, 64, 2, 2, 4, None, abits=4, epochs=0)
    pk = pack_block(fq, 4)                      # packing itself is unchanged for W4A4 (as in the reference)
    x = make_calib_inputs(1, 64, 256, dtype=torch.float16).to(DEV)
    with pytest.raises(OQError, match="weight-only"):
        _run(pk, x, mask, pos)


# ---- model level: the three-layer synthetic LM of the PPL parity test (restated, not imported) -----------------------
CFG = dict(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_key_value_heads=4, rms_norm_eps=1e-6)
VOCAB, T_LM, NSAMP, NLAYERS = 256, 64, 8, 3


def _model(seed=0):
    g = torch.Generator().manual_seed(seed)
    H, I = CFG["hidden_size"], CFG["intermediate_size"]
    emb = torch.randn(VOCAB, H, generator=g) * 0.5
    emb[:, 7] *= 6.0
    head = torch.randn(VOCAB, H, generator=g) * 0.02
    fnorm = 1 + 0.1 * torch.randn(H, generator=g)
    layers = []
    for _ in range(NLAYERS):
        w = {}
        for n, shp in (("self_attn.q_proj", (H, H)), ("self_attn.k_proj", (H, H)), ("self_attn.v_proj", (H, H)),
                       ("self_attn.o_proj", (H, H)), ("mlp.gate_proj", (I, H)), ("mlp.up_proj", (I, H)),
                       ("mlp.down_proj", (H, I))):
            w[n + ".weight"] = (torch.randn(shp, generator=g) * 0.08).half().float()
        w["input_layernorm.weight"] = (1 + 0.1 * torch.randn(H, generator=g)).half().float()
        w["post_attention_layernorm.weight"] = (1 + 0.1 * torch.randn(H, generator=g)).half().float()
        layers.append(w)
    tokens = torch.randint(0, VOCAB, (NSAMP, T_LM), generator=g)
    return emb, head, fnorm, layers, tokens


def _ppl(hidden, fnorm, head, tokens):
    T = tokens.shape[1]
    h = fnorm * (hidden * torch.rsqrt(hidden.pow(2).mean(-1, keepdim=True) + 1e-6))
    logits = h @ head.T
    nll = [torch.nn.functional.cross_entropy(logits[i, :-1].float(), tokens[i, 1:]).float() * T for i in range(tokens.shape[0])]
    return float(torch.exp(torch.stack(nll).sum() / (tokens.shape[0] * T)))


def test_packed_model_ppl_matches_fake_quant_chain():
    from omniquant_amd.calibrate import calibrate_layers, default_args
    from omniquant_amd.synthetic import make_config, make_layer
    emb, head, fnorm, layers, tokens = _model()
    inps = emb[tokens]
    mask = torch.triu(torch.full((T_LM, T_LM), torch.finfo(torch.float32).min), 1)[None, None].to(DEV)
    pos = torch.arange(T_LM, device=DEV)[None]
    cfg = make_config(None, family="llama", hidden_size=CFG["hidden_size"], inter=CFG["intermediate_size"], heads=4, kv_heads=4)
    args = default_args(wbits=4, abits=16, group_size=64, lwc=True, let=False, epochs=2, nsamples=NSAMP, net="llama")
    hip_layers = [make_layer(cfg, weights=dict(w), device=DEV) for w in layers]
    qlayers, _, _, (qi, _) = calibrate_layers(hip_layers, cfg, args, inps.to(DEV), mask, pos, use_graph=False,
                                              compute_dtype=torch.float32)
    packed = [pack_block(copy.deepcopy(q), 4) for q in qlayers]
    outs = []
    for i in range(NSAMP):
        h = inps[i:i + 1].to(DEV)
        for blk in packed:
            h = _run(blk, h, mask, pos)
        outs.append(h)
    ppl_packed = _ppl(torch.cat(outs).float().cpu(), fnorm, head, tokens)
    ppl_fq = _ppl(qi.float().cpu(), fnorm, head, tokens)
    print(f"packed-model PPL {ppl_packed:.5f}, fake-quant chain {ppl_fq:.5f}")
    assert math.isfinite(ppl_packed) and abs(ppl_packed - ppl_fq) / ppl_fq < 1e-3
