"""The 8-bit code KV cache of the weight-only packed blocks (PackedKVCache / PagedKVCache(code_bits=8)): the appending kernel
against the quantiser's torch restatement (oq_kv_append_codes8 and its ragged / paged forms), decode and chunked-prefill
attention on the codes against float64 (oq_attn_decode_codes8*, oq_attn_extend_codes8*), the cache objects, and the
weight-only LLaMA-GQA and OPT blocks packed with kv_cache_bits=8 against the same blocks on a float cache."""
import copy
import math
from types import SimpleNamespace

import pytest
import torch

import test_hip_kv_decode as KD
import test_hip_kv_ragged as RG
from omniquant_amd import OQError, block_common, ops
from omniquant_amd.kvcache import PackedKVCache, PagedKVCache, unpack_codes
from omniquant_amd.llama_block import QuantLlamaAttention
from omniquant_amd.realquant import load_packed_block, pack_block
from test_hip_kv_codes import HEADS, LENGTHS, _bound, _masks, _ref64, _same, _same_nan
from test_hip_kv_extend import LENS as EXT_LENS
from test_hip_kv_paged import UNIT, _perm, _pool_of, _slab
from test_hip_kv_ragged import _i32, _ragged_ref64, _x

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")


def quant8(x):
    """The 8-bit code cache's quantiser in plain float32 torch, over the last dim (tests/test_kvcodes8_cpu.py checks this
    restatement against oracle.ref_cpu.fake_quant): 255 levels, the row range widened to contain zero.  Returns (codes uint8,
    meta float32 [..., 2]).  Scale 0: codes 0, meta (0, 0); scale not finite: codes 0 under a NaN scale (zero-point
    unspecified, returned as 0)."""
    x = x.to(F32)
    lo = x.amin(dim=-1, keepdim=True).clamp(max=0.0)
    hi = x.amax(dim=-1, keepdim=True).clamp(min=0.0)
    scale = (hi - lo) / 255.0
    zp = (-lo / scale).clamp(min=-1e4, max=1e4).round()
    q = (torch.round(x / scale) + zp).clamp(0, 255)
    zero, bad = scale == 0, ~torch.isfinite(scale)
    codes = torch.where(zero | bad, torch.zeros_like(q), q).to(torch.uint8)
    scale = torch.where(bad, torch.full_like(scale, NAN), scale)
    zp = torch.where(zero | bad, torch.zeros_like(zp), zp)
    return codes, torch.cat((scale, zp), dim=-1)


def _buffers8(n, nkv, cap, hd, fill=(0xFF, NAN)):
    """Poisoned 8-bit code buffers [n, nkv, cap, hd | 2]."""
    kc = torch.full((n, nkv, cap, hd), fill[0], dtype=torch.uint8, device=DEV)
    km = torch.full((n, nkv, cap, 2), fill[1], dtype=F32, device=DEV)
    return [kc, kc.clone(), km, km.clone()]


def _poisoned(bufs, sl):
    return all(bool((bufs[i][sl] == 0xFF).all()) and bool(torch.isnan(bufs[2 + i][sl]).all()) for i in range(2))


def _rope(hd, P=64):
    attn = SimpleNamespace(rope_theta=10000.0, head_dim=hd, max_position_embeddings=P)
    return QuantLlamaAttention._rope_table(attn, P, DEV)


def _meta_equal(got, want):
    """(scale, zero-point) pairs bit for bit; a NaN scale equals a NaN scale and leaves the zero-point open."""
    bad = torch.isnan(want[..., 0])
    return torch.equal(torch.isnan(got[..., 0]), bad) and torch.equal(got[~bad].view(torch.int32), want[~bad].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# append
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tq", [3, 1])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dts", [(F32, F32), (BF16, BF16), (F32, BF16)])
def test_append_codes8_matches_the_restatement_bit_for_bit(dts, hd, Tq):
    din, dout = dts
    bs, nh, nkv, past, cap = 2, 4, 2, 2, 8
    g = torch.Generator(device=DEV).manual_seed(hd + Tq)
    q = (torch.randn(bs, Tq, nh, hd, generator=g, device=DEV) * 3).to(din)
    k = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV).to(din)
    v = (torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV) * 0.7).to(din)
    cos, sin = _rope(hd)
    pos = torch.stack([torch.arange(Tq) * 7 + 2, torch.arange(Tq) + 40]).to(DEV)
    bufs = _buffers8(bs, nkv, cap, hd)
    qo, ko, vo = (torch.empty(t.shape, dtype=dout, device=DEV) for t in (q, k, v))
    ops.kv_append_codes(k, v, dout, *bufs, past=past, q=q, q_out=qo, k_out=ko, v_out=vo, cos=cos, sin=sin, positions=pos)
    rows = slice(past, past + Tq)
    # the fp32 post-RoPE k (the plain append of the widened inputs into a float32 cache) and v
    kc = torch.zeros(bs, nkv, cap, hd, dtype=F32, device=DEV)
    vc = torch.zeros_like(kc)
    q32 = ops.kv_append(k.float(), v.float(), kc, vc, past, q=q.float(), q_out=torch.empty(q.shape, dtype=F32, device=DEV), cos=cos,
                        sin=sin, positions=pos)
    for codes, meta, rot, out in ((bufs[0], bufs[2], kc, ko), (bufs[1], bufs[3], vc, vo)):
        want_c, want_m = quant8(rot[:, :, rows].cpu())
        assert torch.equal(codes[:, :, rows].cpu(), want_c) and _meta_equal(meta[:, :, rows].cpu(), want_m)
        val = unpack_codes(codes[:, :, rows].cpu(), meta[:, :, rows].cpu(), bits=8)
        assert _same(out.cpu(), val.to(dout).transpose(1, 2).contiguous())
    assert _poisoned(bufs, (slice(None), slice(None), slice(0, past))) and \
        _poisoned(bufs, (slice(None), slice(None), slice(past + Tq, cap)))
    # q is rotated, not quantised: ops.kv_append's bits (float32 inputs into a bfloat16 cache: rounded once)
    if din == dout:
        c2 = torch.zeros(bs, nkv, cap, hd, dtype=dout, device=DEV)
        want_q = ops.kv_append(k, v, c2, c2.clone(), past, q=q, q_out=torch.empty_like(q), cos=cos, sin=sin, positions=pos)
    else:
        want_q = q32.to(dout)
    assert _same(qo, want_q)
    # rows that straddle zero: the float32 cache of today's 8-bit head quantiser
    k8 = torch.zeros(bs, nkv, cap, hd, dtype=F32, device=DEV)
    v8 = torch.zeros_like(k8)
    ops.kv_append_quant(k.float(), v.float(), 8, F32, k_cache=k8, v_cache=v8, past=past, q=q.float(),
                        q_out=torch.empty(q.shape, dtype=F32, device=DEV), cos=cos, sin=sin, positions=pos)
    for codes, meta, rot, ref in ((bufs[0], bufs[2], kc, k8), (bufs[1], bufs[3], vc, v8)):
        r = rot[:, :, rows]
        straddle = ((r.amin(-1) < 0) & (r.amax(-1) > 0)).cpu()
        assert int(straddle.sum()) >= straddle.numel() - 1
        val = unpack_codes(codes[:, :, rows].cpu(), meta[:, :, rows].cpu(), bits=8)
        assert _same(val[straddle], ref[:, :, rows].cpu()[straddle])


def test_append_codes8_special_rows():
    """All-positive, all-negative, constant, all-zero, NaN, +inf and subnormal-scale rows in one batch (no rotation)."""
    bs, Tq, nh, nkv, hd, cap = 1, 7, 2, 2, 64, 8
    g = torch.Generator(device=DEV).manual_seed(5)
    k = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV)
    v = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV)
    k[0, 0, 0] = k[0, 0, 0].abs() + 6.0
    k[0, 1, 0] = -k[0, 1, 0].abs() - 6.0
    k[0, 2, 0] = 1.75
    k[0, 3, 0] = 0.0
    v[0, 3, 1] = 0.0
    k[0, 4, 0, 5] = NAN
    v[0, 5, 1, 7] = float("inf")
    steps = torch.randint(0, 256, (hd,), generator=g, device=DEV, dtype=torch.int32)
    steps[0], steps[1] = 0, 255
    k[0, 6, 0] = (steps * 32771).view(F32)                 # bit patterns below 2^23: multiples of ~4.6e-41, a subnormal scale
                                                           # whose reciprocal overflows
    bufs = _buffers8(bs, nkv, cap, hd)
    ko, vo = torch.empty_like(k), torch.empty_like(v)
    ops.kv_append_codes(k, v, F32, *bufs, past=0, k_out=ko, v_out=vo)
    for codes, meta, src, out in ((bufs[0], bufs[2], k, ko), (bufs[1], bufs[3], v, vo)):
        want_c, want_m = quant8(src.transpose(1, 2).cpu())
        assert torch.equal(codes[:, :, :Tq].cpu(), want_c) and _meta_equal(meta[:, :, :Tq].cpu(), want_m)
        assert _same_nan(out.cpu(), unpack_codes(codes[:, :, :Tq].cpu(), meta[:, :, :Tq].cpu(), bits=8).transpose(1, 2).contiguous())
    kcod, kmet = bufs[0][0, 0].cpu(), bufs[2][0, 0].cpu()
    assert kmet[0, 1] == 0 and kmet[1, 1] == 255 and kmet[2, 1] == 0 and bool((kcod[2] == 255).all())
    assert bool((kcod[3] == 0).all()) and kmet[3].tolist() == [0.0, 0.0] and bool((ko[0, 3, 0] == 0).all())
    assert bool((bufs[1][0, 1, 3] == 0).all()) and bufs[3][0, 1, 3].tolist() == [0.0, 0.0] and bool((vo[0, 3, 1] == 0).all())
    assert bool((kcod[4] == 0).all()) and bool(torch.isnan(kmet[4, 0])) and bool(torch.isnan(ko[0, 4, 0]).all())
    assert bool((bufs[1][0, 1, 5] == 0).all()) and bool(torch.isnan(bufs[3][0, 1, 5, 0])) and bool(torch.isnan(vo[0, 5, 1]).all())
    assert torch.equal(kcod[6].int(), steps.cpu()) and float(kmet[6, 1]) == 0.0 and float(kmet[6, 0]) > 0.0
    assert int(torch.isnan(ko).sum()) == hd and int(torch.isnan(vo).sum()) == hd
    assert _poisoned(bufs, (slice(None), slice(None), slice(Tq, cap)))


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dts", [(F32, F32), (BF16, BF16), (F32, BF16)])
def test_ragged_and_paged_append_codes8_store_the_slab_rows(dts, hd):
    din, dout = dts
    bs, Tq, nh, nkv, cap = 5, 3, 4, 2, 16
    lens = [0, 5, 3, 70, 2]                                 # sequence 3: beyond every capacity used here
    g = torch.Generator(device=DEV).manual_seed(hd)
    q = (torch.randn(bs, Tq, nh, hd, generator=g, device=DEV) * 3).to(din)
    k = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV).to(din)
    v = (torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV) + 0.5).to(din)
    cos, sin = _rope(hd, 128)

    def outs():
        return [torch.empty(t.shape, dtype=dout, device=DEV) for t in (q, k, v)]

    slab = _buffers8(bs, nkv, cap, hd)
    so = outs()
    ops.kv_append_codes(k, v, dout, *slab, q=q, q_out=so[0], k_out=so[1], v_out=so[2], cos=cos, sin=sin, lengths=_i32(lens))
    for b, n in enumerate(lens):
        one = slice(b, b + 1)
        if n + Tq > cap:
            assert _poisoned(slab, (one,))
            continue
        ref = _buffers8(1, nkv, cap, hd)
        ro = [torch.empty(t[one].shape, dtype=dout, device=DEV) for t in (q, k, v)]
        ops.kv_append_codes(k[one], v[one], dout, *ref, past=n, q=q[one], q_out=ro[0], k_out=ro[1], v_out=ro[2], cos=cos, sin=sin)
        assert all(_same_nan(t[one], r) for t, r in zip(slab, ref)), b
        assert all(_same(o[one], r) for o, r in zip(so, ro)), b
        assert not _poisoned(slab, (one, slice(None), slice(n, n + Tq)))
    for ps in (16, 64):
        num_pages = 6
        perm = _perm(num_pages, hd + ps)
        table = [[perm[0]], [perm[1]], [perm[2]], [perm[3]], [-1]]      # sequence 4: no page
        pools = _buffers8(num_pages, nkv, ps, hd)
        po = outs()
        ops.kv_append_codes(k, v, dout, *pools, q=q, q_out=po[0], k_out=po[1], v_out=po[2], cos=cos, sin=sin, lengths=_i32(lens),
                            page_table=torch.tensor(table, dtype=torch.int32, device=DEV))
        assert all(_same(a, b_) for a, b_ in zip(po, so))
        for b in range(3):
            for t, s in zip(pools, slab):
                assert _same_nan(t[perm[b], :, :cap], s[b]), (ps, b)
            assert _poisoned(pools, (perm[b], slice(None), slice(cap, ps)))
        for page in perm[3:]:                                # beyond the capacity (ps 16) or past the first page; unused pages
            assert _poisoned(pools, (page,)), (ps, page)


# ---------------------------------------------------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------------------------------------------------
_CACHES = {}


def _filled8(hd, bs, nkv, cap):
    """8-bit code buffers of `cap` random rows (through the append kernel, no rotation), computed once per shape."""
    key = (hd, bs, nkv, cap)
    if key not in _CACHES:
        g = torch.Generator(device=DEV).manual_seed(hd + 7 * bs + 13 * nkv + cap)
        k = torch.randn(bs, cap, nkv, hd, generator=g, device=DEV) * 1.5
        v = torch.randn(bs, cap, nkv, hd, generator=g, device=DEV) + 0.5
        v[:, ::5] = v[:, ::5].abs() + 0.1                   # all-positive rows: zero-point 0
        bufs = _buffers8(bs, nkv, cap, hd)
        ops.kv_append_codes(k, v, F32, *bufs, past=0)
        assert bool((bufs[3][:, :, ::5, 1] == 0).all()) and bool((bufs[3][:, :, 1::5, 1] > 0).any())
        _CACHES[key] = bufs
    return _CACHES[key]


def _values8(bufs):
    return unpack_codes(bufs[0], bufs[2], bits=8), unpack_codes(bufs[1], bufs[3], bits=8)


def _run_case(cd, hd, nh, nkv, Tq, L, bs, kind, worst):
    scale = hd ** -0.5
    bufs = tuple(t[:, :, :L].contiguous() for t in _filled8(hd, bs, nkv, 1000))
    kf, vf = _values8(bufs)
    g = torch.Generator(device=DEV).manual_seed(L + nh)
    q = torch.randn(bs, Tq, nh, hd, generator=g, device=DEV).to(cd)
    mask = _masks(bs, Tq, L, kind)
    o = ops.decode_attention_codes(q, bufs, L, scale, mask)
    assert o.dtype == cd and o.shape == q.shape and bool(torch.isfinite(o).all())
    ref = _ref64(q, kf, vf, L, scale, mask)
    err, top = float((o.double().cpu() - ref).abs().max()), float(ref.abs().max())
    worst[0] = max(worst[0], err / top)
    assert err <= _bound(cd, top), (hd, nh, nkv, Tq, L, kind, err, top)
    # a second launch, and a larger capacity whose rows >= L hold NaN meta and 0xFF codes: the same bits
    assert _same(ops.decode_attention_codes(q, bufs, L, scale, mask), o)
    big = _buffers8(bs, nkv, L + 37, hd)
    for t, s in zip(big, bufs):
        t[:, :, :L].copy_(s)
    assert _same(ops.decode_attention_codes(q, big, L, scale, mask), o)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("cd", [F32, BF16])
def test_decode_attention_codes8_matches_float64(cd, hd):
    """The bound of test_hip_kv_codes: (1e-4 + 2^-8 [bf16]) max|ref| against float64 of the dequantised buffers."""
    worst = [0.0]
    for nh, nkv, Tq in HEADS:
        for L in LENGTHS:
            if L < Tq:
                continue
            _run_case(cd, hd, nh, nkv, Tq, L, 1, None, worst)
            if Tq == 3:
                _run_case(cd, hd, nh, nkv, Tq, L, 1, "causal", worst)
            if (nh, nkv) == (4, 2):
                _run_case(cd, hd, nh, nkv, Tq, L, 2, "hf", worst)
    print(f"decode_attention_codes (8-bit) {cd} hd {hd}: max err / max|ref| vs float64 {worst[0]:.3e}")


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("cd", [F32, BF16])
def test_ragged_and_paged_decode_attention_codes8(cd, hd):
    """lens [0, 5, 130] against a per-sequence float64 softmax, rows no query sees poisoned; paged == ragged bit for bit."""
    bs, lens, scale = 3, [0, 5, 130], hd ** -0.5
    for nh, nkv, Tq in ((4, 2, 1), (8, 2, 3), (8, 1, 1)):
        L = max(lens) + Tq
        src = [t[:, :, :L] for t in _filled8(hd, bs, nkv, 1000)]
        g = torch.Generator(device=DEV).manual_seed(nh + Tq)
        q = torch.randn(bs, Tq, nh, hd, generator=g, device=DEV).to(cd)
        bufs = _buffers8(bs, nkv, L + 9, hd)
        for t, s in zip(bufs, src):
            for b, n in enumerate(lens):
                t[b, :, :n + Tq] = s[b, :, :n + Tq]
        o = ops.decode_attention_codes(q, bufs, L, scale, lengths=_i32(lens))
        kf, vf = _values8([s.contiguous() for s in src])
        ref, _ = _ragged_ref64(q, kf, vf, lens, scale)
        err, top = float((o.double() - ref).abs().max()), float(ref.abs().max())
        print(f"ragged 8-bit codes {cd} hd {hd} heads ({nh}, {nkv}) Tq {Tq}: max err {err:.3e} of max|ref| {top:.3e}")
        assert o.dtype == cd and bool(torch.isfinite(o).all()) and err <= _bound(cd, top), (err, top)
        assert _same(o, ops.decode_attention_codes(q, bufs, L, scale, lengths=_i32(lens)))
        clean = [s.contiguous() for s in src]
        assert _same(o, ops.decode_attention_codes(q, clean, L, scale, lengths=_i32(lens)))
        for ps in (16, 128):
            mp = -(-L // ps)
            num_pages = 3 * mp + 1
            perm = _perm(num_pages, ps + Tq)
            table = [perm[b * mp:(b + 1) * mp] for b in range(bs)]
            pools = _pool_of([_slab(t, mp * ps) for t in clean], table, num_pages, ps)
            op = ops.decode_attention_codes(q, tuple(pools), L, scale, lengths=_i32(lens),
                                            page_table=torch.tensor(table, dtype=torch.int32, device=DEV))
            assert _same(op, o), (nh, nkv, Tq, ps)


# ---------------------------------------------------------------------------------------------------------------------
# chunked prefill
# ---------------------------------------------------------------------------------------------------------------------
NROWS = 1152


def _extend8(q, bufs, L, scale, lens, table=None, **kw):
    if table is not None:
        kw["page_table"] = torch.tensor(table, dtype=torch.int32, device=DEV)
    return ops.extend_attention_codes(q, tuple(bufs), L, scale, _i32(lens), **kw)


def _query(hd, nh, Tq):
    g = torch.Generator(device=DEV).manual_seed(3 * nh + Tq)
    return torch.randn(3, Tq, nh, hd, generator=g, device=DEV).to(BF16)


@pytest.mark.parametrize("Tq", [16, 17, 40, 130])
@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (6, 1)])
@pytest.mark.parametrize("hd", [64, 128])
def test_extend_attention_codes8_matches_float64(hd, heads, Tq):
    """test_hip_kv_extend's bound: |o - ref| <= UNIT[bf16] |ref| + (2^-8 + 2e-5) mag, mag = sum_j p_j |v_j|."""
    nh, nkv = heads
    scale = 1.0 / math.sqrt(hd)
    q = _query(hd, nh, Tq)
    bufs = _filled8(hd, 3, nkv, NROWS)
    kf, vf = _values8(bufs)
    for lens, extra in EXT_LENS:
        L = max(lens) + Tq + extra
        o = _extend8(q, [_slab(t, L) for t in bufs], L, scale, lens)
        ref, mag = _ragged_ref64(q, kf, vf, lens, scale)
        err = (o.double() - ref).abs()
        bound = UNIT[BF16] * ref.abs() + (2.0 ** -8 + 2e-5) * mag
        print(f"extend 8-bit codes hd {hd} heads {heads} Tq {Tq} lens {lens}: max err {float(err.max()):.3e}, "
              f"max (err - bound) {float((err - bound).max()):.3e}")
        assert o.dtype == BF16 and bool(torch.isfinite(o).all())
        assert bool((err <= bound).all()), (lens, float((err - bound).max()))


@pytest.mark.parametrize("Tq", [17, 40])
@pytest.mark.parametrize("hd", [64, 128])
def test_extend_attention_codes8_paged_poisoned_and_reproducible(hd, Tq):
    nh, nkv = 8, 2
    lens, extra = EXT_LENS[2]
    L, scale = max(lens) + Tq + extra, 1.0 / math.sqrt(hd)
    q = _query(hd, nh, Tq)
    bufs = _filled8(hd, 3, nkv, NROWS)
    ref = _extend8(q, [_slab(t, L) for t in bufs], L, scale, lens)
    assert bool(torch.isfinite(ref).all())
    # bitwise reproducible, into a caller's output and a dirty workspace
    ws = torch.full((64 << 20,), 0xFF, dtype=torch.uint8, device=DEV)
    o = torch.empty_like(q)
    assert _extend8(q, [_slab(t, L) for t in bufs], L, scale, lens, out=o, workspace=ws) is o and _same(o, ref)
    # rows no query row sees, and rows beyond L, hold 0xFF codes under NaN meta
    dirty = []
    for t, fill in zip(bufs, (0xFF, 0xFF, NAN, NAN)):
        s = _slab(t, L + 9, fill)
        for b, n in enumerate(lens):
            s[b, :, n + Tq:] = fill
        dirty.append(s)
    assert _same(_extend8(q, dirty, L, scale, lens), ref)
    for ps in (16, 128):
        mp = -(-L // ps)
        vals = [_slab(t, mp * ps) for t in bufs]
        num_pages = 3 * mp + 1
        perm = _perm(num_pages, ps + Tq)
        table = [perm[b * mp:(b + 1) * mp] for b in range(3)]
        assert _same(_extend8(q, _pool_of(vals, table, num_pages, ps), L, scale, lens, table), ref), (hd, Tq, ps)
        # the pages a sequence does not need: -1 in the table, NaN in the pool
        held = [-(-(n + Tq) // ps) for n in lens]
        cut = [table[b][:held[b]] + [-1] * (mp - held[b]) for b in range(3)]
        pools = []
        for t, fill in zip(vals, (0xFF, 0xFF, NAN, NAN)):
            s = t.clone()
            for b, n in enumerate(lens):
                s[b, :, n + Tq:] = fill
            pool = torch.full((num_pages, nkv, ps, t.shape[3]), fill, dtype=t.dtype, device=DEV)
            for b in range(3):
                for i in range(held[b]):
                    pool[cut[b][i]] = s[b, :, i * ps:(i + 1) * ps]
            pools.append(pool)
        assert _same(_extend8(q, pools, L, scale, lens, cut), ref), (hd, Tq, ps)


# ---------------------------------------------------------------------------------------------------------------------
# the cache objects
# ---------------------------------------------------------------------------------------------------------------------
def test_code8_cache_python_surface():
    bs, nkv, hd, cap, T = 2, 3, 128, 10, 7
    c = PackedKVCache(bs, nkv, hd, F32, DEV, cap, code_bits=8)
    assert c.nbytes() == 2 * bs * nkv * cap * (hd + 8) and c.capacity == cap and "code_bits=8" in repr(c)
    assert c.k_codes.shape == (bs, nkv, cap, hd) and c.k_meta.shape == (bs, nkv, cap, 2)
    assert PackedKVCache(1, 2, 64, BF16, DEV, 4, code_bits=8).nbytes() == 2 * 2 * 4 * 72
    g = torch.Generator(device=DEV).manual_seed(1)
    raw = tuple(torch.randn(bs, nkv, T, hd, generator=g, device=DEV) for _ in range(2))
    snap = [t.clone() for t in raw]
    c = PackedKVCache.from_tuple(raw, code_bits=8)
    assert all(_same(t, s) for t, s in zip(raw, snap))
    assert c.code_bits == 8 and c.length == T and len(c) == 2
    for codes, meta, src in ((c.k_codes, c.k_meta, raw[0]), (c.v_codes, c.v_meta, raw[1])):
        want_c, want_m = quant8(src.cpu())
        assert torch.equal(codes[:, :, :T].cpu(), want_c) and _meta_equal(meta[:, :, :T].cpu(), want_m)
    k, v = c.dequantize()
    assert _same(k.cpu(), unpack_codes(c.k_codes[:, :, :T].cpu(), c.k_meta[:, :, :T].cpu(), bits=8))
    assert c[0].shape == (bs, nkv, T, hd) and _same(c[0], k) and _same(c[-1], v) and _same(c.to_tuple()[1], v)
    c[0].zero_()                                            # a copy, not a view
    assert _same(c[0], k)
    d = c.clone()
    assert d.code_bits == 8 and _same(d.dequantize()[0], k)
    d.k_codes.fill_(0)
    d.v_meta.fill_(0)
    assert _same(c.dequantize()[0], k) and _same(c.dequantize()[1], v)
    old = c.capacity
    c.reserve(old + 5)
    assert c.capacity >= T + old + 5 and c.length == T and c.k_codes.shape[3] == hd
    assert _same(c.dequantize()[0], k) and _same(c.dequantize()[1], v)
    h = PackedKVCache.from_tuple(raw, dtype=BF16, code_bits=8)
    assert h[0].dtype == BF16 and _same(h[0], k.to(BF16))
    with pytest.raises(OQError, match="code_bits"):
        PackedKVCache(1, 2, 64, F32, DEV, 4, code_bits=3)
    with pytest.raises(OQError, match="head_dim"):
        PackedKVCache(1, 2, 96, F32, DEV, 4, code_bits=8)
    with pytest.raises(OQError):
        PackedKVCache.from_tuple(raw, head_bits=4, code_bits=8)     # a W4A4 block's rows belong in a 4-bit code cache
    with pytest.raises(OQError, match="code_bits"):
        PagedKVCache(1, 2, 64, F32, DEV, 4, code_bits=3)


def test_paged_code8_cache_fork_and_set_lengths_keep_the_codes():
    nkv, hd, ps, n = 2, 64, 16, 40
    c = PagedKVCache(2, nkv, hd, BF16, DEV, 8, page_size=ps, code_bits=8)
    assert c.k_codes.shape == (8, nkv, ps, hd) and "code_bits=8" in repr(c)
    assert c.nbytes() == 2 * 8 * nkv * ps * (hd + 8) + c.page_table.numel() * 4
    g = torch.Generator(device=DEV).manual_seed(2)
    k, v = (torch.randn(2, n, nkv, hd, generator=g, device=DEV).to(BF16) for _ in range(2))
    c.reserve(n)
    ops.kv_append_codes(k, v, BF16, c.k_codes, c.v_codes, c.k_meta, c.v_meta, lengths=c.lengths, page_table=c.page_table)
    c.advance(n, [n, 0])
    c.set_lengths([n, 0])
    want = tuple(unpack_codes(*quant8(t[0].float().transpose(0, 1).cpu()), bits=8).to(BF16) for t in (k, v))
    assert all(_same(a.cpu(), w) for a, w in zip(c.sequence(0), want))
    c.fork(0, 1)
    p0, p1 = c.pages(0), c.pages(1)
    assert p0[:2] == p1[:2] and p0[2] != p1[2]              # two full pages shared, the partial one copied
    assert all(_same(a.cpu(), w) for a, w in zip(c.sequence(1), want))
    c.set_lengths([n, 20])                                  # into a shared page: a private copy of it first
    assert c.pages(1)[0] == p0[0] and c.pages(1)[1] != p0[1]
    assert all(_same(a.cpu(), w[:, :20]) for a, w in zip(c.sequence(1), want))
    assert all(_same(a.cpu(), w) for a, w in zip(c.sequence(0), want))
    d = c.clone()
    assert d.code_bits == 8 and all(_same(a.cpu(), w) for a, w in zip(d.sequence(0), want))


# ---------------------------------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------------------------------
BLOCKS8 = {"llama_gqa": ("llama", 4, 2), "opt": ("opt", 4, 4)}
_PACKED8 = {}
H, PROMPT, ONES, CHUNK = 256, 24, 4, 20
TOTAL = PROMPT + ONES + CHUNK


def _blocks(name):
    """(the weight-only block on a float cache, the same calibrated block packed with kv_cache_bits=8)."""
    if name not in _PACKED8:
        _, fq, pk = KD._block(name)
        _PACKED8[name] = (pk, pack_block(copy.deepcopy(fq), 4, kv_cache_bits=8))
    return _PACKED8[name]


def _new_cache(name, cd, kind, code_bits, bs=2):
    fam, nh, nkv = BLOCKS8[name]
    if kind == "paged":
        return PagedKVCache(bs, nkv, H // nh, cd, DEV, 8, page_size=16, code_bits=code_bits)
    return PackedKVCache(bs, nkv, H // nh, cd, DEV, capacity=TOTAL, code_bits=code_bits, ragged=True)


def _drive(blk, name, cache, x, after=None):
    """Prefill PROMPT rows, ONES single-token steps and one CHUNK-row step of the hidden inputs x [2, TOTAL, H] on a ragged
    cache; after(cache) runs behind every step.  Returns the outputs of all rows."""
    fam = BLOCKS8[name][0]
    outs = [RG._step(blk, fam, x[:, :PROMPT], cache, KD._causal(PROMPT).expand(2, 1, PROMPT, PROMPT),
                     torch.arange(PROMPT, device=DEV)[None])]
    at = PROMPT
    for n in [1] * ONES + [CHUNK]:
        if after is not None:
            after(cache, at)
        outs.append(RG._step(blk, fam, x[:, at:at + n], cache))
        at += n
    if after is not None:
        after(cache, at)
    return torch.cat(outs, dim=1)


def _lossy_agree(got, ref, what):
    """The criterion of a bfloat16 block against its float32 self (test_hip_kv_decode._agree, bf16 branch), printed first."""
    got, ref = got.float(), ref.float()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    err, top = float((got - ref).abs().max()), float(ref.abs().max())
    cos = float(torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0))
    print(f"8-bit code cache vs float cache, {what}: max err / max|ref| {err / top:.3e}, 1 - cos {1 - cos:.3e}")
    assert cos >= 0.9999 and err <= 2e-2 * top, (what, cos, err, top)


@pytest.mark.parametrize("cd", [F32, BF16])
@pytest.mark.parametrize("name", list(BLOCKS8))
def test_blocks_on_the_8bit_code_cache(name, cd, monkeypatch):
    pk, p8 = _blocks(name)
    calls = []
    real = ops.extend_attention_codes
    monkeypatch.setattr(ops, "extend_attention_codes", lambda *a, **kw: (calls.append(a[0].shape[1]), real(*a, **kw))[1])
    try:
        pk.compute_dtype = p8.compute_dtype = cd
        x = _x(2, TOTAL, 41)
        fcache = _new_cache(name, cd, "slab", None)
        ref = _drive(pk, name, fcache, x)
        assert not calls
        snaps = []

        def rows_match(cache, at):
            """float32 compute: the code cache's dequantised rows are the restatement of the float cache's rows, bit for bit
            (the float-cache block ran first: its rows [0, at) are final)."""
            if cd != F32:
                return
            for b in range(2):
                got = cache.sequence(b)
                for g_, f in zip(got, (fcache.k[b, :, :at], fcache.v[b, :, :at])):
                    assert _same(g_.cpu(), unpack_codes(*quant8(f.cpu()), bits=8)), (name, at, b)
            snaps.append(at)

        c8 = _new_cache(name, cd, "slab", 8)
        out = _drive(p8, name, c8, x, rows_match)
        assert c8.code_bits == 8 and c8.lengths.tolist() == [TOTAL, TOTAL]
        assert cd != F32 or snaps == [PROMPT + i for i in range(ONES + 1)] + [TOTAL]
        # the 20-row chunk on a bfloat16 ragged cache takes the MFMA kernel, once; float32 stays on the decode kernel
        assert calls == ([CHUNK] if cd == BF16 else [])
        _lossy_agree(out, ref, f"{name} {cd} (prefill {PROMPT}, {ONES} x 1, chunk {CHUNK})")
        calls.clear()
        paged = _new_cache(name, cd, "paged", 8)
        assert _same(_drive(p8, name, paged, x), out)
        assert calls == ([CHUNK] if cd == BF16 else [])
        # the block creates its own cache of that kind, and converts a (k, v) tuple into one
        fam = BLOCKS8[name][0]
        mask, pos = KD._causal(PROMPT).expand(2, 1, PROMPT, PROMPT), torch.arange(PROMPT, device=DEV)[None]
        o1, own = KD._fwd(p8, x[:, :PROMPT], mask, pos, use_cache=True)
        assert isinstance(own, PackedKVCache) and own.code_bits == 8 and own.length == PROMPT
        assert _same(o1, out[:, :PROMPT])
        raw = tuple(t[:, :, :PROMPT].clone() for t in (fcache.k, fcache.v))
        step = x[:, PROMPT:PROMPT + 1]
        o2, c2 = KD._fwd(p8, step, None, torch.full((1, 1), PROMPT, device=DEV), past=raw, use_cache=True)
        assert c2.code_bits == 8 and c2.length == PROMPT + 1
        o3, _ = KD._fwd(p8, step, None, torch.full((1, 1), PROMPT, device=DEV), past=own, use_cache=True)
        if cd == F32:                                       # (bfloat16: the tuple's rows were rounded before they were quantised)
            assert _same(o2, o3) and _same(o3, out[:, PROMPT:PROMPT + 1])
        assert fam in ("llama", "opt")
    finally:
        pk.compute_dtype = p8.compute_dtype = BF16


@pytest.mark.parametrize("name", list(BLOCKS8))
def test_zero_pad_rows_are_harmless_on_the_8bit_code_cache(name):
    """A right-padded ragged prefill whose pad rows are all-zero hidden states, then a padded chunk: finite valid rows that
    agree with the float-cache block (on which such rows are legal today)."""
    pk, p8 = _blocks(name)
    fam = BLOCKS8[name][0]
    tokens, chunk = [PROMPT, 16], [CHUNK, 9]
    x = _x(2, PROMPT + CHUNK, 43)
    x[1, 16:PROMPT] = 0
    xc = x[:, PROMPT:].clone()
    xc[1, 9:] = 0
    outs = []
    for blk, bits in ((pk, None), (p8, 8)):
        cache = _new_cache(name, BF16, "slab", bits)
        a = RG._step(blk, fam, x[:, :PROMPT], cache, KD._causal(PROMPT).expand(2, 1, PROMPT, PROMPT),
                     torch.arange(PROMPT, device=DEV)[None], new_tokens=tokens)
        if bits == 8 and fam == "llama":                    # RMSNorm of a zero row is zero, and so is its k: codes 0, meta (0, 0)
            assert bool((cache.k_codes[1, :, 16:PROMPT] == 0).all()) and bool((cache.k_meta[1, :, 16:PROMPT] == 0).all())
        b = RG._step(blk, fam, xc, cache, new_tokens=chunk)
        valid = torch.cat([a[0], b[0], a[1, :16], b[1, :9]])
        assert bool(torch.isfinite(valid).all()), (name, bits)
        outs.append(valid)
    _lossy_agree(outs[1], outs[0], f"{name} bf16 with zero pad rows")


def test_load_packed_block_with_kv_cache_bits_8_and_the_refusals():
    from omniquant_amd.calibrate import decoder_layer_class, default_args
    from omniquant_amd.synthetic import make_layer
    import test_hip_packed_a4 as A4
    name = "llama_gqa"
    cfg, fq, pk = KD._block(name)
    _, p8 = _blocks(name)
    args = default_args(wbits=4, abits=16, group_size=64, lwc=True, let=False, epochs=1, nsamples=2, net="llama", real_quant=False)
    fresh = decoder_layer_class("llama")(cfg, make_layer(cfg, seed=99, device=DEV), args).to(DEV)
    load_packed_block(fresh, {k: v.clone() for k, v in p8.state_dict().items()}, 4, 64, kv_cache_bits=8)
    x = _x(2, TOTAL, 44)
    try:
        for cd in (BF16, F32):
            p8.compute_dtype = fresh.compute_dtype = cd
            ca, cb = _new_cache(name, cd, "slab", 8), _new_cache(name, cd, "slab", 8)
            assert _same(_drive(p8, name, ca, x), _drive(fresh, name, cb, x))
            assert all(_same(s, t) for b in range(2) for s, t in zip(ca.sequence(b), cb.sequence(b)))
    finally:
        p8.compute_dtype = BF16
    # the three refusals
    with pytest.raises(OQError, match="act_quant"):
        pack_block(copy.deepcopy(fq), 4, kv_cache_bits=4)
    a4 = A4._calibrated("gqa")
    with pytest.raises(OQError, match="kv_cache_bits"):
        pack_block(copy.deepcopy(a4[2]), 4, act_quant=True, kv_cache_bits=8)
    with pytest.raises(OQError, match="code_bits"):
        PackedKVCache(1, 2, 64, F32, DEV, 4, code_bits=3)
    # a caller's cache of the wrong kind: 8-bit on a W4A4 block, 4-bit on a weight-only block
    mask, pos = KD._causal(8).expand(2, 1, 8, 8), torch.arange(8, device=DEV)[None]
    with pytest.raises(OQError, match="code_bits"):
        A4._fwd(a4[3], A4._x(2, 8, 3), mask, pos, past=PackedKVCache(2, 2, 64, BF16, DEV, 16, code_bits=8), use_cache=True)
    with pytest.raises(OQError, match="code_bits"):
        KD._fwd(pk, _x(2, 8, 3), mask, pos, past=PackedKVCache(2, 2, 64, BF16, DEV, 16, code_bits=4), use_cache=True)
    # an unmarked weight-only block takes a caller's 8-bit cache
    out, present = KD._fwd(pk, _x(2, 8, 3), mask, pos, past=PackedKVCache(2, 2, 64, BF16, DEV, 16, code_bits=8), use_cache=True)
    assert present.code_bits == 8 and present.length == 8 and bool(torch.isfinite(out).all())
    torch.cuda.synchronize()
    assert block_common.EXTEND_MIN_TQ <= CHUNK
