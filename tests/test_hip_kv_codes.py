"""The KV cache stored as 4-bit codes (PackedKVCache(code_bits=4)): the appending kernel's codes against the float32 cache of
the same inputs (oq_kv_append_quant_codes vs oq_kv_append_quant, bit for bit), decode attention on the codes
(oq_attn_decode_codes) against a float64 reference and against oq_attn_decode, and the cache object's Python surface."""
import copy
from types import SimpleNamespace

import pytest
import torch

from omniquant_amd import OQError, ops
from omniquant_amd.kvcache import PackedKVCache, unpack_codes
from omniquant_amd.llama_block import QuantLlamaAttention
from omniquant_amd.realquant import pack_block

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else (t.view(torch.int32) if t.element_size() == 4 else t)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _same_nan(a, b):
    """Bit for bit, a NaN counting as equal to a NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(na, nb) and \
        torch.equal(_bits(a.contiguous())[~na], _bits(b.contiguous())[~nb])


def _code_buffers(bs, nkv, cap, hd, fill=None):
    kc = torch.empty(bs, nkv, cap, hd // 2, dtype=torch.uint8, device=DEV)
    km = torch.empty(bs, nkv, cap, 2, dtype=F32, device=DEV)
    if fill is not None:
        kc.fill_(fill[0])
        km.fill_(fill[1])
    return kc, kc.clone(), km, km.clone()


# ---------------------------------------------------------------------------------------------------------------------
# append
# ---------------------------------------------------------------------------------------------------------------------
def _append_both(q, k, v, dout, past, cap, cos, sin, positions):
    """The float32-cache append and the code append of the same inputs."""
    bs, Tq, nkv, hd = k.shape
    kc = torch.full((bs, nkv, cap, hd), 12345.0, dtype=F32, device=DEV)
    vc = torch.full_like(kc, -777.0)
    # (bf16 inputs are widened exactly, as the kernel widens them before it rotates and quantises)
    ops.kv_append_quant(k.float(), v.float(), 4, F32, k_cache=kc, v_cache=vc, past=past, q=q.float(),
                        q_out=torch.empty(q.shape, dtype=F32, device=DEV), cos=cos, sin=sin, positions=positions)
    ref = [torch.empty(t.shape, dtype=dout, device=DEV) for t in (q, k, v)]
    ops.kv_append_quant(k, v, 4, dout, past=past, q=q, q_out=ref[0], k_out=ref[1], v_out=ref[2], cos=cos, sin=sin,
                        positions=positions)
    bufs = _code_buffers(bs, nkv, cap, hd, fill=(0xA5, 12345.0))
    out = [torch.empty(t.shape, dtype=dout, device=DEV) for t in (q, k, v)]
    ops.kv_append_codes(k, v, dout, *bufs, past=past, q=q, q_out=out[0], k_out=out[1], v_out=out[2], cos=cos, sin=sin,
                        positions=positions)
    return kc, vc, ref, bufs, out


def _check_append(kc, vc, ref, bufs, out, past, Tq):
    k_codes, v_codes, k_meta, v_meta = bufs
    rows = slice(past, past + Tq)
    for codes, meta, cache in ((k_codes, k_meta, kc), (v_codes, v_meta, vc)):
        # (dequantised on the CPU: the contract in plain float32 arithmetic with subnormals kept)
        assert _same_nan(unpack_codes(codes[:, :, rows].cpu(), meta[:, :, rows].cpu()), cache[:, :, rows].cpu())
        for lo, hi in ((0, past), (past + Tq, codes.shape[2])):
            assert bool((codes[:, :, lo:hi] == 0xA5).all()) and bool((meta[:, :, lo:hi] == 12345.0).all())
    assert all(_same_nan(a, b) for a, b in zip(out, ref))


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dts", [(F32, F32), (F32, BF16), (BF16, BF16)])
def test_append_codes_match_the_float32_cache_bit_for_bit(hd, dts):
    din, dout = dts
    bs, Tq, nh, nkv, past, cap = 3, 5, 8, 2, 11, 24
    g = torch.Generator(device=DEV).manual_seed(hd)
    q = (torch.randn(bs, Tq, nh, hd, generator=g, device=DEV) * 3).to(din)
    k = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV).to(din)
    v = (torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV) + 2).to(din)
    attn = SimpleNamespace(rope_theta=10000.0, head_dim=hd, max_position_embeddings=64)
    cos, sin = QuantLlamaAttention._rope_table(attn, past + Tq, DEV)
    per_sample = torch.stack([torch.arange(past, past + Tq) - 3, torch.arange(past, past + Tq), torch.arange(Tq) * 7 + 2]).to(DEV)
    kc, vc, ref, bufs, out = _append_both(q, k, v, dout, past, cap, cos, sin, per_sample)
    assert not bool(torch.isnan(kc[:, :, past:past + Tq]).any())
    _check_append(kc, vc, ref, bufs, out, past, Tq)
    # the zero-points are the quantiser's rounded ones; v = randn + 2 has rows above 0, whose zero-point is negative
    assert bool((bufs[3][:, :, past:past + Tq, 1] == bufs[3][:, :, past:past + Tq, 1].round()).all())


def test_append_codes_degenerate_rows():
    """A constant non-zero head row and an all-zero head row (scale 0: the reference quantiser's 0 / 0) come out of the float32
    append as NaN throughout; the code cache must hold the same."""
    bs, Tq, nh, nkv, hd, past, cap = 2, 4, 4, 2, 64, 3, 9
    g = torch.Generator(device=DEV).manual_seed(5)
    q = torch.randn(bs, Tq, nh, hd, generator=g, device=DEV)
    k = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV)
    v = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV)
    k[0, 1, 0] = 1.75
    k[1, 2, 1] = 0.0
    v[1, 0, 0] = -3.0
    kc, vc, ref, bufs, out = _append_both(q, k, v, F32, past, cap, None, None, None)     # (no rotation: the rows stay constant)
    assert bool(torch.isnan(kc[0, 0, past + 1]).all()) and bool(torch.isnan(kc[1, 1, past + 2]).all())
    assert int(torch.isnan(kc[:, :, past:past + Tq]).sum()) == 2 * hd
    _check_append(kc, vc, ref, bufs, out, past, Tq)


def test_append_codes_subnormal_scale_row():
    """A head row whose scale is subnormal (its reciprocal overflows): the quantiser divides exactly there, a zero element
    stays a number, and the code cache holds what the float32 cache holds."""
    bs, Tq, nh, nkv, hd, past, cap = 1, 2, 2, 2, 64, 0, 2
    g = torch.Generator(device=DEV).manual_seed(9)
    q = torch.randn(bs, Tq, nh, hd, generator=g, device=DEV)
    k = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV)
    v = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV)
    steps = torch.randint(0, 16, (hd,), generator=g, device=DEV, dtype=torch.int32)
    steps[0], steps[1] = 0, 15
    k[0, 1, 0] = (steps * 71362).view(F32)                 # multiples of ~1e-40 (bit patterns: no arithmetic that could flush)
    kc, vc, ref, bufs, out = _append_both(q, k, v, F32, past, cap, None, None, None)
    assert not bool(torch.isnan(kc).any())
    _check_append(kc, vc, ref, bufs, out, past, Tq)
    codes = torch.stack((bufs[0][0, 0, 1] & 0xF, bufs[0][0, 0, 1] >> 4), dim=-1).reshape(hd)
    assert torch.equal(codes.int(), steps) and float(bufs[2][0, 0, 1, 1]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------------------------------------------------
HEADS = [(2, 2, 1), (4, 2, 1), (3, 1, 1), (8, 1, 1), (4, 1, 3)]       # (nh, nkv, Tq): R = rep * Tq = 1, 2, 3, 8, 12
LENGTHS = [1, 127, 128, 129, 1000]
_CACHES = {}


def _filled(hd, bs, nkv, cap):
    """Code buffers of `cap` random rows (through the append kernel, no rotation), computed once per shape and left alone."""
    key = (hd, bs, nkv, cap)
    if key not in _CACHES:
        g = torch.Generator(device=DEV).manual_seed(hd + 7 * bs + 13 * nkv + cap)
        k = torch.randn(bs, cap, nkv, hd, generator=g, device=DEV) * 1.5
        v = torch.randn(bs, cap, nkv, hd, generator=g, device=DEV) + 0.5
        bufs = _code_buffers(bs, nkv, cap, hd)
        ops.kv_append_codes(k, v, F32, *bufs, past=0)
        _CACHES[key] = bufs
    return _CACHES[key]


def _ref64(q, kf, vf, L, scale, mask):
    """float64 softmax(scale q k^T + mask) v on the CPU from the dequantised float32 buffers [bs, nkv, cap, hd]."""
    bs, Tq, nh, hd = q.shape
    rep = nh // kf.shape[1]
    k = kf[:, :, :L].double().cpu().repeat_interleave(rep, dim=1)
    v = vf[:, :, :L].double().cpu().repeat_interleave(rep, dim=1)
    s = torch.einsum("bthd,bhjd->bhtj", q.double().cpu(), k) * scale
    if mask is not None:
        s = torch.maximum(s + mask.double().cpu(), torch.tensor(float(torch.finfo(F32).min), dtype=torch.float64))
    return torch.einsum("bhtj,bhjd->bthd", torch.softmax(s, dim=-1), v)


def _bound(cd, top):
    """fp32: the project's bound for summation-order differences; bf16: plus one rounding of the output (2^-9 relative)
    with a factor 2 of margin."""
    return (1e-4 + (2.0 ** -8 if cd == BF16 else 0.0)) * top


def _masks(bs, Tq, L, kind):
    if kind is None:
        return None
    past = L - Tq
    j, t = torch.arange(L)[None, :], torch.arange(Tq)[:, None]
    if kind == "causal":                                   # float32 [1, 1, Tq, L], broadcast over the batch
        return torch.where(j > past + t, torch.finfo(F32).min, 0.0).to(F32)[None, None].to(DEV)
    mn = torch.finfo(torch.float16).min                    # fp16 per sample, the second sample left-padded
    m = torch.where(j > past + t, mn, 0.0).to(torch.float16)[None, None].repeat(bs, 1, 1, 1)
    m[1, 0, :, :min(2, past)] += torch.tensor(mn, dtype=torch.float16)
    return m.to(DEV)


def _run_case(cd, hd, nh, nkv, Tq, L, bs, kind, worst):
    scale = hd ** -0.5
    bufs = tuple(t[:, :, :L].contiguous() for t in _filled(hd, bs, nkv, 1000))
    kf, vf = unpack_codes(bufs[0], bufs[2]), unpack_codes(bufs[1], bufs[3])
    g = torch.Generator(device=DEV).manual_seed(L + nh)
    q = torch.randn(bs, Tq, nh, hd, generator=g, device=DEV).to(cd)
    mask = _masks(bs, Tq, L, kind)
    o = ops.decode_attention_codes(q, bufs, L, scale, mask)
    assert o.dtype == cd and o.shape == q.shape and bool(torch.isfinite(o).all())
    ref = _ref64(q, kf, vf, L, scale, mask)
    err, top = float((o.double().cpu() - ref).abs().max()), float(ref.abs().max())
    worst[0] = max(worst[0], err / top)
    assert err <= _bound(cd, top), (hd, nh, nkv, Tq, L, kind, err, top)
    # a second launch, and a larger capacity whose rows >= L hold NaN scales and 0xFF codes: the same bits
    assert _same(ops.decode_attention_codes(q, bufs, L, scale, mask), o)
    big = _code_buffers(bs, nkv, L + 37, hd, fill=(0xFF, float("nan")))
    for t, s in zip(big, bufs):
        t[:, :, :L].copy_(s)
    assert _same(ops.decode_attention_codes(q, big, L, scale, mask), o)
    # today's kernel on a float32 / bf16 cache of the dequantised values: within the summation-order bound (NOT bit-identical:
    # the code kernel applies a row's scale once per row and, for one or two query rows, holds 16 dims per lane)
    if cd == F32:
        o2 = ops.decode_attention(q, kf, vf, L, scale, mask)
        e2 = float((o2 - o).abs().max())
        worst[1] = max(worst[1], e2 / top)
        assert e2 <= 1e-4 * top, (hd, nh, nkv, Tq, L, kind, e2, top)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("cd", [F32, BF16])
def test_decode_attention_codes_matches_float64(cd, hd):
    worst = [0.0, 0.0]
    for nh, nkv, Tq in HEADS:
        for L in LENGTHS:
            if L < Tq:          # (oq_attn_decode's contract: the Tq query rows are among the L cached ones)
                continue
            _run_case(cd, hd, nh, nkv, Tq, L, 1, None, worst)
            if Tq == 3:
                _run_case(cd, hd, nh, nkv, Tq, L, 1, "causal", worst)
            if (nh, nkv) == (4, 2):
                _run_case(cd, hd, nh, nkv, Tq, L, 2, "hf", worst)
    print(f"decode_attention_codes {cd} hd {hd}: max err / max|ref| vs float64 {worst[0]:.3e}, vs oq_attn_decode {worst[1]:.3e}")


def test_decode_attention_codes_takes_a_cache_and_a_batch_of_long_rows():
    """The PackedKVCache form of the argument, at a batch whose split count is limited by the workgroup target."""
    bs, nkv, nh, hd, L = 5, 8, 16, 128, 300
    c = PackedKVCache(bs, nkv, hd, BF16, DEV, 320, code_bits=4)
    g = torch.Generator(device=DEV).manual_seed(3)
    k, v = (torch.randn(bs, L, nkv, hd, generator=g, device=DEV) for _ in range(2))
    ops.kv_append_codes(k, v, BF16, c.k_codes, c.v_codes, c.k_meta, c.v_meta, past=0)
    c.length = L
    q = torch.randn(bs, 1, nh, hd, generator=g, device=DEV).to(BF16)
    o = ops.decode_attention_codes(q, c, L, hd ** -0.5)
    ref = _ref64(q, unpack_codes(c.k_codes, c.k_meta), unpack_codes(c.v_codes, c.v_meta), L, hd ** -0.5, None)
    err, top = float((o.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"decode_attention_codes bs 5, 16 / 8 heads of 128, L 300, bf16: max err {err:.3e} of max|ref| {top:.3e}")
    assert err <= _bound(BF16, top)


# ---------------------------------------------------------------------------------------------------------------------
# the cache object
# ---------------------------------------------------------------------------------------------------------------------
def test_code_cache_python_surface():
    bs, nkv, hd, cap, T = 2, 3, 128, 10, 7
    c = PackedKVCache(bs, nkv, hd, F32, DEV, cap, code_bits=4)
    assert c.nbytes() == 2 * bs * nkv * cap * (64 + 8) and c.capacity == cap and "code_bits=4" in repr(c)
    assert PackedKVCache(bs, nkv, hd, BF16, DEV, cap).nbytes() == 2 * bs * nkv * cap * hd * 2
    g = torch.Generator(device=DEV).manual_seed(1)
    raw = tuple(torch.randn(bs, nkv, T, hd, generator=g, device=DEV) for _ in range(2))
    snap = [t.clone() for t in raw]
    c = PackedKVCache.from_tuple(raw, head_bits=4, code_bits=4)
    f = PackedKVCache.from_tuple(raw, head_bits=4)
    assert all(_same(t, s) for t, s in zip(raw, snap))
    assert c.code_bits == 4 and f.code_bits is None and c.length == f.length == T and len(c) == 2
    k, v = c.dequantize()
    assert _same(k, f.k[:, :, :T]) and _same(v, f.v[:, :, :T])
    assert c[0].shape == (bs, nkv, T, hd) and _same(c[0], k) and _same(c[-1], v) and _same(c.to_tuple()[1], v)
    assert all(_same(a, b) for a, b in zip(c, (k, v)))
    c[0].zero_()                                            # a copy, not a view
    assert _same(c[0], k)
    # clone is independent; reserve keeps the valid rows
    d = c.clone()
    d.k_codes.fill_(0)
    d.v_meta.fill_(0)
    assert _same(c.dequantize()[0], k) and _same(c.dequantize()[1], v)
    old = c.capacity
    c.reserve(old + 5)
    assert c.capacity >= T + old + 5 and c.length == T
    assert _same(c.dequantize()[0], k) and _same(c.dequantize()[1], v)
    h = PackedKVCache.from_tuple(raw, dtype=BF16, head_bits=4, code_bits=4)
    assert h[0].dtype == BF16 and _same(h[0], k.to(BF16))


def test_code_cache_errors():
    from test_hip_packed_a4 import _calibrated, _causal, _fwd, _x
    with pytest.raises(OQError, match="code_bits"):
        PackedKVCache(1, 2, 64, F32, DEV, 4, code_bits=3)
    with pytest.raises(OQError, match="head_dim"):
        PackedKVCache(1, 2, 96, F32, DEV, 4, code_bits=4)
    with pytest.raises(OQError, match="GPU"):
        PackedKVCache(1, 2, 64, F32, "cpu", 4, code_bits=4)
    raw = tuple(torch.randn(1, 2, 4, 64, device=DEV) for _ in range(2))
    with pytest.raises(OQError):
        PackedKVCache.from_tuple(raw, code_bits=4)          # raw rows are not on a 4-bit grid
    cfg, args, fq, pk, mask, pos = _calibrated("gqa")
    with pytest.raises(OQError, match="act_quant"):
        pack_block(copy.deepcopy(fq), 4, kv_cache_bits=4)
    with pytest.raises(OQError, match="kv_cache_bits"):
        pack_block(copy.deepcopy(fq), 4, act_quant=True, kv_cache_bits=8)
    p_ = torch.arange(8, device=DEV)[None]
    for bs, nkv in ((3, 2), (2, 4)):                        # the block's step: batch 2, 2 kv heads of 64
        wrong = PackedKVCache(bs, nkv, 64, torch.bfloat16, DEV, 16, code_bits=4)
        with pytest.raises(OQError, match="does not fit"):
            _fwd(pk, _x(2, 8, 3), _causal(8).expand(2, 1, 8, 8), p_, past=wrong, use_cache=True)
    torch.cuda.synchronize()
