"""W4A4 real-quant inference (csrc/oq_packed_a4.hip, oq_kv_append_quant, realquant.pack_block(..., act_quant=True), the
integer path of the packed LLaMA block).  The value contract of an act_bits = 4 PackedLinear is the exact product of the two
4-bit grids: y = s_a s_w sum_k (q_a - z_a)(q_w - z_w) + bias (+ residual), the activation codes being the ones the
quantiser kernel wrote (ops.IntCodes), z_w = unpacked qzeros + 1 (AutoGPTQ's decoding, -1 wrap included)."""
import copy
import math
from types import SimpleNamespace

import pytest
import torch

from omniquant_amd import OQError, ops
from omniquant_amd import realquant as RQ
from omniquant_amd.kvcache import PackedKVCache
from omniquant_amd.llama_block import QuantLlamaAttention
from omniquant_amd.realquant import PackedLinear, load_packed_block, pack_block, unpack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rand_packed(inn, out, bias=True, seed=0, device=DEV):
    """Random int32 words of a 4-bit per-channel layer: every code value and every stored zero (including zero - 1 = -1,
    the wrap to 16) occurs."""
    g = torch.Generator().manual_seed(seed)
    p = dict(qweight=torch.randint(-2 ** 31, 2 ** 31, (inn // 8, out), generator=g, dtype=torch.int64).to(torch.int32),
             qzeros=torch.randint(-2 ** 31, 2 ** 31, (1, out // 8), generator=g, dtype=torch.int64).to(torch.int32),
             scales=((torch.rand(1, out, generator=g) + 0.5) * (0.5 / 16)).half(),
             g_idx=torch.zeros(inn, dtype=torch.int32),
             bias=torch.randn(out, generator=g).half() if bias else None)
    return PackedLinear(4, inn, inn, out, {k: (None if v is None else v.to(device)) for k, v in p.items()}, act_bits=4)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _w_grid(pl):
    """(q_w [out, in], z_w [out], s_w [out]) decoded on the host side from the AutoGPTQ buffers."""
    q = unpack(pl.qweight, 4, pl.infeatures).t()
    z = unpack(pl.qzeros.t().contiguous(), 4, pl.outfeatures).t()[0] + 1
    return q, z, pl.scales.float()[0]


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inn,out", [(96, 160), (4096, 11008)])
def test_weight_codes_are_exact(inn, out):
    pl = _rand_packed(inn, out, seed=inn)
    w = pl.weight_codes()
    q, z, s = _w_grid(pl)
    assert w.nbits == 4 and w.codes.dtype == torch.int8 and tuple(w.codes.shape) == (out, inn)
    assert torch.equal(w.codes.long(), q)
    assert bool((z == 16).any()) and bool((q == 15).any()) and bool((q == 0).any())     # the -1 wrap and every code occur
    assert torch.equal(w.zp, z.float()) and torch.equal(w.scale, s)
    assert torch.equal(w.csum.double(), q.sum(1).double())


def _inputs(M, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
    x[0] = torch.rand(K, generator=g) + 0.25               # an all-positive row: its zero-point lies outside the grid
    return x.to(dtype).to(DEV)


def _check_linear(pl, M, dtype, bias, residual, seed):
    K, N = pl.infeatures, pl.outfeatures
    if not bias:
        pl.bias = None
    x = _inputs(M, K, dtype, seed)
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(seed + 1)).to(dtype).to(DEV) if residual else None
    xint = pl.quantize_input(x)
    with torch.no_grad():
        y = pl(x, residual=res)
        y2 = pl.forward_codes(xint, res, dtype)
    assert y.dtype == dtype and y.shape == (M, N) and _same(y, y2)
    qa, za, sa, ca = xint.codes.double(), xint.zp.double(), xint.scale.double(), xint.csum.double()
    assert torch.equal(ca, qa.sum(1))
    q, z, s = _w_grid(pl)
    qw, zw, sw = q.double(), z.double(), s.double()
    acc = qa @ qw.T
    ref = sa[:, None] * sw[None] * ((qa - za[:, None]) @ (qw - zw[:, None]).T)
    mag = sa[:, None] * sw[None] * (acc.abs() + (za[:, None] * qw.sum(1)[None]).abs() + (zw[None] * (ca - K * za)[:, None]).abs())
    if pl.bias is not None:
        ref = ref + pl.bias.double()
        mag = mag + pl.bias.double().abs()
    if res is not None:
        ref = ref + res.double()
        mag = mag + res.double().abs()
    bound = 2.0 ** -20 * mag
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * ref.abs()
    err = (y.double() - ref).abs()
    assert bool(torch.isfinite(y).all())
    assert bool((err <= bound).all()), (M, K, N, float((err - bound).max()))


@pytest.mark.parametrize("inn,out", [(96, 160), (4096, 4096), (4096, 11008), (11008, 4096)])
def test_linear_matches_float64_contract(inn, out):
    pl = _rand_packed(inn, out, seed=inn + out)
    bias0 = pl.bias
    for i, M in enumerate((1, 5, 16, 17, 64, 2048)):
        pl.bias = bias0
        dtype = (torch.float32, torch.bfloat16)[i % 2]
        _check_linear(pl, M, dtype, bias=i % 3 != 2, residual=i % 2 == 0, seed=100 * i + inn)
    pl.bias = bias0
    if inn == 96:
        for M in (1, 17):                        # every dtype / epilogue combination on the small shape
            for dtype in (torch.float32, torch.bfloat16):
                for b in (False, True):
                    for r in (False, True):
                        pl.bias = bias0
                        _check_linear(pl, M, dtype, b, r, seed=M + 7)


def test_degenerate_row_poisons_its_own_row():
    pl = _rand_packed(256, 64, seed=5)
    for M in (4, 40):
        x = _inputs(M, 256, torch.float32, 9)
        x[1] = 0.5                                # constant row: scale 0 (quirk Q1)
        with torch.no_grad():
            y = pl(x)
        assert bool(torch.isnan(y[1]).all()) and bool(torch.isfinite(y[torch.arange(M) != 1]).all())


def test_batch_invariance_gemv_vs_prefill():
    pl = _rand_packed(4096, 4096, seed=3)
    for dtype in (torch.bfloat16, torch.float32):
        x = _inputs(2048, 4096, dtype, 11)
        res = torch.randn(2048, 4096, generator=torch.Generator().manual_seed(12)).to(dtype).to(DEV)
        xint = pl.quantize_input(x)
        full = pl.forward_codes(xint, res, dtype)
        again = pl.forward_codes(xint, res, dtype)
        assert _same(full, again)
        for lo, hi in ((0, 1), (0, 5), (100, 116), (2040, 2048)):
            assert hi - lo <= RQ.GEMV_A4_MAX_ROWS
            part = pl.forward_codes(xint.rows(lo, hi), res[lo:hi], dtype)
            assert _same(part, full[lo:hi]), (dtype, lo, hi)
            assert _same(part, pl.forward_codes(xint.rows(lo, hi), res[lo:hi], dtype))


def _ref_headq(x, nbits=4):
    """quantize/quantizer.py:122-147 per (token, head) over the last dim, in the reference's float32 arithmetic."""
    Q = 2 ** nbits - 1
    xmin, xmax = x.amin(-1, keepdim=True), x.amax(-1, keepdim=True)
    scale = (xmax - xmin) / Q
    zp = (-xmin / scale).clamp(min=-1e4, max=1e4).round()
    return ((x / scale).round() + zp).clamp(0, Q).sub(zp).mul(scale)


def _ref_rot(x, c, s):
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat((x1 * c[..., :h] + (-x2) * s[..., :h], x2 * c[..., h:] + x1 * s[..., h:]), dim=-1)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dts", [(torch.float32, torch.bfloat16), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)])
def test_kv_append_quant_matches_reference(hd, dts):
    din, dout = dts
    bs, Tq, nh, nkv, past, cap = 3, 5, 8, 2, 11, 24
    g = torch.Generator(device=DEV).manual_seed(hd)
    q = (torch.randn(bs, Tq, nh, hd, generator=g, device=DEV) * 3).to(din)
    k = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV).to(din)
    v = (torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV) + 2).to(din)
    attn = SimpleNamespace(rope_theta=10000.0, head_dim=hd, max_position_embeddings=64)
    cos, sin = QuantLlamaAttention._rope_table(attn, past + Tq, DEV)
    per_sample = torch.stack([torch.arange(past, past + Tq) - 3, torch.arange(past, past + Tq), torch.arange(Tq) * 7 + 2]).to(DEV)
    P = cos.shape[0]
    cpos = per_sample.clamp(0, P - 1).cpu()
    c, s = cos.cpu()[cpos][:, :, None], sin.cpu()[cpos][:, :, None]          # [bs, Tq, 1, hd]
    rq = _ref_headq(_ref_rot(q.float().cpu(), c, s)).to(dout)
    rk = _ref_headq(_ref_rot(k.float().cpu(), c, s)).to(dout)
    rv = _ref_headq(v.float().cpu()).to(dout)
    kc = torch.full((bs, nkv, cap, hd), 12345.0, dtype=dout, device=DEV)
    vc = torch.full_like(kc, -777.0)
    kc0, vc0 = kc.clone(), vc.clone()
    qo, ko, vo = torch.empty(q.shape, dtype=dout, device=DEV), torch.empty(k.shape, dtype=dout, device=DEV), torch.empty(k.shape, dtype=dout, device=DEV)
    ops.kv_append_quant(k, v, 4, dout, k_cache=kc, v_cache=vc, past=past, q=q, q_out=qo, k_out=ko, v_out=vo, cos=cos, sin=sin,
                        positions=per_sample)
    assert _same(qo.cpu(), rq) and _same(ko.cpu(), rk) and _same(vo.cpu(), rv)
    assert _same(kc[:, :, past:past + Tq].cpu(), rk.transpose(1, 2)) and _same(vc[:, :, past:past + Tq].cpu(), rv.transpose(1, 2))
    for t, t0 in ((kc, kc0), (vc, vc0)):
        assert _same(t[:, :, :past], t0[:, :, :past]) and _same(t[:, :, past + Tq:], t0[:, :, past + Tq:])
    # no cache (the no-cache forward), shared positions = past + t by default
    qo2, ko2, vo2 = torch.empty_like(qo), torch.empty_like(ko), torch.empty_like(vo)
    ops.kv_append_quant(k, v, 4, dout, past=past, q=q, q_out=qo2, k_out=ko2, v_out=vo2, cos=cos, sin=sin)
    c2, s2 = cos.cpu()[past:past + Tq][None, :, None], sin.cpu()[past:past + Tq][None, :, None]
    assert _same(qo2.cpu(), _ref_headq(_ref_rot(q.float().cpu(), c2, s2)).to(dout)) and _same(vo2, vo)


# ---------------------------------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------------------------------
LLAMA_SHAPES = {"base": (256, 64, 2, 2), "gqa": (256, 64, 4, 2), "hd128_fused": (256, 256, 2, 2)}
_BUILT = {}


def _calibrated(shape, let=False, seed=2):
    key = (shape, let)
    if key not in _BUILT:
        from omniquant_amd.calibrate import calibrate_layers, default_args
        from omniquant_amd.synthetic import causal_mask, make_calib_inputs, make_config, make_layer
        H, T, nh, nkv = LLAMA_SHAPES[shape]
        cfg = make_config(None, family="llama", hidden_size=H, inter=2 * H, heads=nh, kv_heads=nkv)
        args = default_args(wbits=4, abits=4, group_size=None, lwc=True, let=let, epochs=1, nsamples=2, net="llama", real_quant=False)
        x = make_calib_inputs(2, T, H, dtype=torch.float16).to(DEV)
        mask = causal_mask(T).to(DEV)
        pos = torch.arange(T, device=DEV)[None]
        layer = make_layer(cfg, seed=seed, device=DEV, outliers=False)
        qlayers, _, _, _ = calibrate_layers([layer], cfg, args, x, mask, pos, use_graph=False)
        pk = pack_block(copy.deepcopy(qlayers[0]), 4, act_quant=True)
        _BUILT[key] = (cfg, args, qlayers[0], pk, mask, pos)
    return _BUILT[key]


def _fwd(blk, x, mask=None, pos=None, past=None, use_cache=False):
    kw = dict(attention_mask=mask, past_key_value=past, use_cache=use_cache)
    if pos is not None:
        kw["position_ids"] = pos
    with torch.no_grad():
        return blk(x, **kw)


def _oracle(cfg, pk, x, mask, pos):
    """oracle.ref_cpu.Block, fp32, 4-bit activation quantisers on, weights = the exact grid values s_w (q_w - z_w)."""
    from oracle import ref_cpu as R
    w = {}
    for name, m in pk.named_modules():
        if isinstance(m, PackedLinear):
            wc = m.weight_codes()
            w[name + ".weight"] = (wc.scale[:, None] * (wc.codes.float() - wc.zp[:, None])).cpu()
            if m.bias is not None:
                w[name + ".bias"] = m.bias.float().cpu()
        elif name.endswith("layernorm"):
            w[name + ".weight"] = m.weight.float().cpu()
            if getattr(m, "bias", None) is not None:
                w[name + ".bias"] = m.bias.float().cpu()
    cd = dict(hidden_size=cfg.hidden_size, num_attention_heads=cfg.num_attention_heads,
              num_key_value_heads=cfg.num_key_value_heads, rms_norm_eps=cfg.rms_norm_eps)
    blk = R.Block("llama", cd, w, R.QuantSpec(16, 4, None, False, False), max_pos=x.shape[1])
    with torch.no_grad():
        return blk.forward(x.float().cpu(), mask.cpu(), pos.cpu(), None, act_quant=True)


def _cos_delta(out, ref, x):
    a, b = (out.float() - x.float()).flatten(), (ref.float() - x.float()).flatten()
    return float(torch.nn.functional.cosine_similarity(a, b, dim=0))


# (LET has no grouped-query attention: block_common._let_temporaries refuses it, so GQA runs with LWC only)
@pytest.mark.parametrize("shape,let", [("base", False), ("gqa", False), ("hd128_fused", False), ("base", True),
                                       ("hd128_fused", True)])
def test_llama_w4a4_block_matches_oracle(shape, let, monkeypatch):
    from omniquant_amd.synthetic import make_calib_inputs
    cfg, args, fq, pk, mask, pos = _calibrated(shape, let)
    H, T = LLAMA_SHAPES[shape][:2]
    assert all(m.act_bits == 4 for m in pk.modules() if isinstance(m, PackedLinear))
    x = make_calib_inputs(1, T, H, seed=11, dtype=torch.float16).to(DEV)
    ref = _oracle(cfg, pk, x, mask, pos)
    pk.compute_dtype = torch.float32
    y32 = _fwd(pk, x.float(), mask, pos)[0].cpu()
    err = float((y32 - ref).abs().max())
    print(f"W4A4 {shape} let={let}: fp32 max err {err:.3e} of max|ref| {float(ref.abs().max()):.3e}")
    assert err <= 1e-3 * float(ref.abs().max())
    pk.compute_dtype = torch.bfloat16
    calls = []
    orig = ops.FusedCausalAttnFn.apply
    monkeypatch.setattr(ops.FusedCausalAttnFn, "apply", lambda *a: calls.append(1) or orig(*a))
    y16 = _fwd(pk, x, mask, pos)[0]
    assert y16.dtype == torch.float16 and bool(torch.isfinite(y16).all())
    cosd = _cos_delta(y16.cpu(), ref, x.cpu())
    print(f"W4A4 {shape} let={let}: bf16 cosine of the deltas {cosd:.5f}")
    assert cosd >= 0.99
    assert bool(calls) == (shape == "hd128_fused")


def test_state_dict_is_the_weight_only_pack_and_reloads_bit_identically():
    from omniquant_amd.calibrate import decoder_layer_class
    from omniquant_amd.synthetic import make_calib_inputs, make_layer
    cfg, args, fq, pk, mask, pos = _calibrated("gqa")
    wo = pack_block(copy.deepcopy(fq), 4)
    sd, sd_wo = pk.state_dict(), wo.state_dict()
    assert sd.keys() == sd_wo.keys() and all(_same(sd[k], sd_wo[k]) for k in sd)
    fresh = decoder_layer_class("llama")(cfg, make_layer(cfg, seed=99, device=DEV), args).to(DEV)
    load_packed_block(fresh, {k: v.clone() for k, v in sd.items()}, 4, None, act_quant=True)
    x = make_calib_inputs(2, 64, 256, seed=4, dtype=torch.float16).to(DEV)
    mask = mask.expand(2, 1, 64, 64)
    for cd in (torch.bfloat16, torch.float32):
        pk.compute_dtype = fresh.compute_dtype = cd
        assert _same(_fwd(fresh, x, mask, pos)[0], _fwd(pk, x, mask, pos)[0])
    pk.compute_dtype = torch.bfloat16


# ---- KV cache ------------------------------------------------------------------------------------------------------------
def _causal(T, past=0, dtype=torch.float32):
    j = torch.arange(past + T)[None, :]
    t = torch.arange(T)[:, None]
    return torch.where(j > past + t, torch.finfo(dtype).min, 0.0).to(dtype)[None, None].to(DEV)


def _x(bs, T, seed, H=256):
    from omniquant_amd.synthetic import make_calib_inputs
    return make_calib_inputs(bs, T, H, seed=seed, dtype=torch.float16).to(DEV)


def _agree(inc, ref, x, cd):
    inc, ref = inc.float(), ref.float()
    assert inc.shape == ref.shape and bool(torch.isfinite(inc).all())
    err, top = float((inc - ref).abs().max()), float(ref.abs().max())
    cosd = _cos_delta(inc, ref, x)
    print(f"{cd}: max err {err:.3e} of max {top:.3e}, cosine of the deltas {cosd:.5f}")
    if cd == torch.float32:
        assert err <= 1e-3 * top, (err, top)
    else:
        assert cosd >= 0.99, cosd


@pytest.mark.parametrize("shape", list(LLAMA_SHAPES))
def test_prefill_with_cache_is_bit_identical_and_decode_matches_full(shape):
    cfg, args, fq, pk, mask, pos = _calibrated(shape)
    H, T, nh, nkv = LLAMA_SHAPES[shape]
    hd = H // nh
    T0 = 200 if shape == "hd128_fused" else 40
    chunks = [1, 1, 1, 1, 3, 1]
    N = T0 + sum(chunks)
    for cd in (torch.bfloat16, torch.float32):
        pk.compute_dtype = cd
        xb = _x(2, T, 11)
        mb = _causal(T).expand(2, 1, T, T)
        a = _fwd(pk, xb, mb, pos)
        out = _fwd(pk, xb, mb, pos, use_cache=True)
        assert len(a) == 1 and len(out) == 2 and isinstance(out[1], PackedKVCache) and _same(a[0], out[0])
        present = out[1]
        assert present.length == T and present[0].shape == (2, nkv, T, hd) and present[0].dtype == cd
        # the cache holds head-quantised rows: at most 16 distinct values per (token, head)
        assert int(torch.unique(present[1][0, 0, 3]).numel()) <= 16
        x = _x(1, N, 5)
        p_ = torch.arange(N, device=DEV)[None]
        ref = _fwd(pk, x, _causal(N), p_)[0]
        o, cache = _fwd(pk, x[:, :T0], _causal(T0), p_[:, :T0], use_cache=True)
        outs, p = [o], T0
        for i, n in enumerate(chunks):
            m = _causal(n, p) if (n > 1 or i % 2) else None
            o, c2 = _fwd(pk, x[:, p:p + n], m, None if i == 2 else p_[:, p:p + n], past=cache, use_cache=True)
            assert c2 is cache and cache.length == p + n
            outs.append(o)
            p += n
        _agree(torch.cat(outs, dim=1), ref, x, cd)
    pk.compute_dtype = torch.bfloat16


def test_tuple_past_equals_packed_cache_and_is_left_alone():
    cfg, args, fq, pk, mask, pos = _calibrated("gqa")
    a = pk.self_attn
    T0, n, nkv, hd = 32, 3, 2, 64
    for cd in (torch.bfloat16, torch.float32):
        pk.compute_dtype = cd
        x = _x(2, T0 + n, 7)
        p_ = torch.arange(T0 + n, device=DEV)[None]
        _, cache = _fwd(pk, x[:, :T0], _causal(T0).expand(2, 1, T0, T0), p_[:, :T0], use_cache=True)
        # the reference layer's present: RAW rotated k and v (fp32 here), [bs, nkv, T, hd]
        with torch.no_grad():
            xe = ops.cast(x[:, :T0], torch.float32).reshape(-1, 256)
            hint = pk._norm_codes(pk.input_layernorm, xe)
            k = a.k_proj.forward_codes(hint, out_dtype=torch.float32).view(2, T0, nkv, hd)
            v = a.v_proj.forward_codes(hint, out_dtype=torch.float32).view(2, T0, nkv, hd)
            cos, sin = a._rope_tables(p_[:, :T0], T0, DEV)
            k = ops.RopeFn.apply(k, cos, sin)
        tup = (k.transpose(1, 2).contiguous(), v.transpose(1, 2).contiguous())
        snap = [t.clone() for t in tup]
        m = _causal(n, T0)
        ra, pa = _fwd(pk, x[:, T0:], m, p_[:, T0:], past=tup, use_cache=True)
        rb, pb = _fwd(pk, x[:, T0:], m, p_[:, T0:], past=cache, use_cache=True)
        assert isinstance(pa, PackedKVCache) and pa.length == pb.length == T0 + n
        assert all(_same(t, s) for t, s in zip(tup, snap))
        _agree(ra, rb, x[:, T0:], cd)
    pk.compute_dtype = torch.bfloat16


@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float32])
def test_left_padded_batch_matches_each_sample_alone(cd):
    cfg, args, fq, pk, mask, pos = _calibrated("gqa")
    pk.compute_dtype = cd
    lens, steps = [24, 16, 8], 8
    Tp = max(lens)
    seqs = [_x(1, n + steps, 30 + i) for i, n in enumerate(lens)]
    X = _x(3, Tp, 29)                         # the pad positions hold some token's hidden state (a zero row has scale 0: NaN)
    am = torch.zeros(3, Tp, dtype=torch.int64, device=DEV)
    for i, n in enumerate(lens):
        X[i, Tp - n:] = seqs[i][0, :n]
        am[i, Tp - n:] = 1

    def hf_mask(am, Tq):
        mn = torch.finfo(torch.float16).min
        return _causal(Tq, am.shape[1] - Tq, torch.float16) + (1 - am[:, None, None, :].to(torch.float16)) * mn

    def pos_of(am):
        return (am.cumsum(-1) - 1).masked_fill(am == 0, 1)

    out, cache = _fwd(pk, X, hf_mask(am, Tp), pos_of(am), use_cache=True)
    step_outs = []
    for s in range(steps):
        xs = torch.stack([seqs[i][0, n + s] for i, n in enumerate(lens)])[:, None]
        am = torch.cat([am, torch.ones(3, 1, dtype=torch.int64, device=DEV)], dim=1)
        o, cache = _fwd(pk, xs, hf_mask(am, 1), pos_of(am)[:, -1:], past=cache, use_cache=True)
        step_outs.append(o)
    for i, n in enumerate(lens):
        ref = _fwd(pk, seqs[i], _causal(n + steps), torch.arange(n + steps, device=DEV)[None])[0]
        got = torch.cat([out[i:i + 1, Tp - n:]] + [o[i:i + 1] for o in step_outs], dim=1)
        _agree(got, ref, seqs[i], cd)
    pk.compute_dtype = torch.bfloat16


# ---- greedy generation on the three-layer synthetic LM (restated from test_hip_kv_decode.py), W4A4 ---------------------
CFG = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_key_value_heads=2, rms_norm_eps=1e-6)
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


def test_greedy_generation_with_cache_matches_recompute():
    from omniquant_amd.calibrate import calibrate_layers, default_args
    from omniquant_amd.synthetic import make_config, make_layer
    emb, head, fnorm, layers, tokens = _model()
    mask = torch.triu(torch.full((T_LM, T_LM), torch.finfo(torch.float32).min), 1)[None, None].to(DEV)
    pos = torch.arange(T_LM, device=DEV)[None]
    cfg = make_config(None, family="llama", hidden_size=CFG["hidden_size"], inter=CFG["intermediate_size"], heads=2, kv_heads=2)
    args = default_args(wbits=4, abits=4, group_size=None, lwc=True, let=False, epochs=1, nsamples=NSAMP, net="llama")
    hip_layers = [make_layer(cfg, weights=dict(w), device=DEV) for w in layers]
    qlayers, _, _, _ = calibrate_layers(hip_layers, cfg, args, emb[tokens].to(DEV), mask, pos, use_graph=False,
                                        compute_dtype=torch.float32)
    packed = [pack_block(copy.deepcopy(q), 4, act_quant=True) for q in qlayers]
    for blk in packed:
        blk.compute_dtype = torch.float32
    emb_d, head_d, fnorm_d = emb.to(DEV), head.to(DEV), fnorm.to(DEV)

    def logits(h):
        h = h.float()
        return (fnorm_d * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + 1e-6))) @ head_d.T

    seq = tokens[0, :16].tolist()
    P = len(seq)
    h = emb_d[torch.tensor(seq, device=DEV)][None]
    caches = []
    for blk in packed:
        h, c = _fwd(blk, h, _causal(P), torch.arange(P, device=DEV)[None], use_cache=True)
        caches.append(c)
    lc = logits(h[0, -1])
    for step in range(16):
        T = len(seq)
        Tp = -(-T // 8) * 8                 # right-padded to the no-cache GEMMs' multiple of 8: causal rows < T never see it
        hf = emb_d[torch.tensor(seq + [0] * (Tp - T), device=DEV)][None]
        for blk in packed:
            hf = _fwd(blk, hf, _causal(Tp), torch.arange(Tp, device=DEV)[None])[0]
        lf = logits(hf[0, T - 1])
        assert int(lc.argmax()) == int(lf.argmax()), (step, float((lc - lf).abs().max()))
        seq.append(int(lf.argmax()))
        hs = emb_d[seq[-1]][None, None]
        for i, blk in enumerate(packed):
            hs, caches[i] = _fwd(blk, hs, None, torch.tensor([[T]], device=DEV), past=caches[i], use_cache=True)
        lc = logits(hs[0, -1])
    assert len(seq) == 32


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_errors_stay_loud():
    pl = _rand_packed(256, 64, seed=1)
    x = torch.randn(4, 256, device=DEV)
    with pytest.raises(OQError, match="float16"):
        pl(x.half())
    with pytest.raises(OQError):
        pl(x.cpu())
    with pytest.raises(OQError):
        pl(x.requires_grad_())
    with pytest.raises(OQError):                         # W4A16 forward of an act_bits 4 layer's codes path
        _rand_packed(256, 64).forward_codes(ops.IntCodes(torch.zeros(4, 256, dtype=torch.int8, device=DEV),
                                                         *(torch.zeros(4, device=DEV) for _ in range(3)), 8))
    cfg, args, fq, pk, mask, pos = _calibrated("gqa")
    with pytest.raises(OQError, match="3-bit weights"):
        pack_block(copy.deepcopy(fq), 3, act_quant=True)
    with pytest.raises(NotImplementedError):
        with torch.no_grad():
            pk(_x(1, 8, 3), attention_mask=_causal(8), position_ids=torch.arange(8, device=DEV)[None], output_attentions=True)
    torch.cuda.synchronize()
