"""Ragged batches on the packed blocks' KV cache: one length per sequence, held on the device.  The ragged appends and
decode attentions of csrc/oq_decode.hip (lens in the place of past / L and the mask), PackedKVCache(ragged=True) and the block
forwards' new_tokens: right-padded prefill, mask-free decode steps, slot reuse and mixed chunk sizes.  The uniform entry points
are the references of the kernels (bit for bit where the issue says so), float64 softmax of the attention, and each sequence
run alone of the blocks."""
import math
from types import SimpleNamespace

import pytest
import torch

import test_hip_kv_decode as KD
import test_hip_packed_a4 as A4
from omniquant_amd import OQError, ops
from omniquant_amd.kvcache import PackedKVCache, unpack_codes
from omniquant_amd.llama_block import QuantLlamaAttention
from test_hip_kv_codes import _bound as _code_bound
from test_hip_kv_codes import _same_nan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
UNIT = KD.UNIT
NAN = float("nan")


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else (t.view(torch.int32) if t.element_size() == 4 else t)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _i32(seq):
    return torch.tensor(list(seq), dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# append: (kind, input dtype, cache / output dtype)
# ---------------------------------------------------------------------------------------------------------------------
APPENDS = [("plain", BF16, BF16), ("plain", F32, F32), ("quant", F32, BF16), ("quant", F32, F32), ("codes", F32, BF16),
           ("codes", F32, F32)]
SENT = {"k": 12345.0, "v": -777.0, "codes": 0xA5, "meta": 12345.0}


def _buffers(kind, bs, nkv, cap, hd, dout, lead=0):
    """Sentinel-filled cache buffers of a kind, [lead + bs + lead, nkv, cap, ...] (the caller slices the middle)."""
    n = bs + 2 * lead
    if kind == "codes":
        kc = torch.full((n, nkv, cap, hd // 2), SENT["codes"], dtype=torch.uint8, device=DEV)
        km = torch.full((n, nkv, cap, 2), SENT["meta"], dtype=F32, device=DEV)
        return [kc, kc.clone(), km, km.clone()]
    return [torch.full((n, nkv, cap, hd), SENT["k"], dtype=dout, device=DEV),
            torch.full((n, nkv, cap, hd), SENT["v"], dtype=dout, device=DEV)]


def _append(kind, q, k, v, bufs, dout, cos, sin, positions, past=0, lengths=None):
    """One append of a kind; returns (q_out, k_out, v_out) (v_out None for the plain append, which has none)."""
    qo = torch.empty(q.shape, dtype=dout, device=DEV)
    ko = torch.empty(k.shape, dtype=dout, device=DEV)
    vo = None if kind == "plain" else torch.empty(v.shape, dtype=dout, device=DEV)
    kw = dict(q=q, q_out=qo, k_out=ko, cos=cos, sin=sin, positions=positions, lengths=lengths)
    if kind == "plain":
        ops.kv_append(k, v, bufs[0], bufs[1], past, **kw)
    elif kind == "quant":
        ops.kv_append_quant(k, v, 4, dout, k_cache=bufs[0], v_cache=bufs[1], past=past, v_out=vo, **kw)
    else:
        ops.kv_append_codes(k, v, dout, *bufs, past=past, v_out=vo, **kw)
    return qo, ko, vo


def _step_inputs(hd, din, bs=3, Tq=4, nh=4, nkv=2):
    g = torch.Generator(device=DEV).manual_seed(hd)
    q = (torch.randn(bs, Tq, nh, hd, generator=g, device=DEV) * 3).to(din)
    k = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV).to(din)
    v = (torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV) + 2).to(din)
    attn = SimpleNamespace(rope_theta=10000.0, head_dim=hd, max_position_embeddings=64)
    cos, sin = QuantLlamaAttention._rope_table(attn, 64, DEV)
    return q, k, v, cos, sin


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kind,din,dout", APPENDS)
def test_ragged_append_equals_the_uniform_append_per_sequence(kind, din, dout, hd):
    bs, Tq, cap, nkv, lens = 3, 4, 24, 2, [0, 5, 17]
    q, k, v, cos, sin = _step_inputs(hd, din)
    explicit = torch.stack([torch.arange(Tq) + 3, torch.arange(Tq) * 7 + 2, torch.arange(Tq) + 40]).to(DEV)
    for pos in (None, explicit):
        bufs = _buffers(kind, bs, nkv, cap, hd, dout)
        outs = _append(kind, q, k, v, bufs, dout, cos, sin, pos, lengths=_i32(lens))
        for b, n in enumerate(lens):
            one = slice(b, b + 1)
            ref_bufs = _buffers(kind, 1, nkv, cap, hd, dout)
            ref_outs = _append(kind, q[one], k[one], v[one], ref_bufs, dout, cos, sin, None if pos is None else pos[one], past=n)
            # the whole [nkv, cap, ...] slab of the sequence: its rows [n, n + Tq) and every sentinel around them
            assert all(_same_nan(t[one], r) for t, r in zip(bufs, ref_bufs)), (kind, b)
            assert all(_same_nan(o[one], r) for o, r in zip(outs, ref_outs) if o is not None), (kind, b)
            for t, fresh in zip(bufs, _buffers(kind, 1, nkv, cap, hd, dout)):
                assert _same(t[one, :, :n], fresh[:, :, :n]) and _same(t[one, :, n + Tq:], fresh[:, :, n + Tq:])
                assert not _same(t[one, :, n:n + Tq], fresh[:, :, n:n + Tq])


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kind,din,dout", APPENDS)
def test_ragged_append_guards_the_rows_the_host_cannot_see(kind, din, dout, hd):
    bs, Tq, cap, nkv, lens, P = 3, 4, 24, 2, [22, 30, -3], 64
    q, k, v, cos, sin = _step_inputs(hd, din)
    big = _buffers(kind, bs, nkv, cap, hd, dout, lead=1)
    expect = [t.clone() for t in big]
    outs = _append(kind, q, k, v, [t[1:1 + bs] for t in big], dout, cos, sin, None, lengths=_i32(lens))
    # The rows that fit: 22 and 23 of sequence 0 (its step rows 0 and 1), and row 0 of sequence 2, whose step row 3 lands at
    # lens + t = -3 + 3 = 0 -- the guard is per row (lens[b] + t in [0, cap)), so that row is stored like any other.  Each
    # equals the uniform append of those step rows alone; sequence 1 (30 >= cap) stores nothing.
    for b, rows, past in ((0, slice(0, 2), 22), (2, slice(3, 4), 0)):
        ref_bufs = _buffers(kind, 1, nkv, cap, hd, dout)
        n = rows.stop - rows.start
        _append(kind, q[b:b + 1, rows], k[b:b + 1, rows], v[b:b + 1, rows], ref_bufs, dout, cos, sin, None, past=past)
        for e, r in zip(expect, ref_bufs):
            e[1 + b, :, past:past + n] = r[0, :, past:past + n]
    assert all(_same_nan(t, e) for t, e in zip(big, expect)), kind          # nothing else, inside or outside the slice
    # the *_out tensors are complete: the uniform append at the same (clamped) positions into a scratch cache
    pos = torch.stack([(torch.arange(Tq) + n).clamp(0, P - 1) for n in lens]).to(DEV)
    ref_outs = _append(kind, q, k, v, _buffers(kind, bs, nkv, cap, hd, dout), dout, cos, sin, pos, past=0)
    assert all(_same_nan(o, r) for o, r in zip(outs, ref_outs) if o is not None), kind


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
_ROWS = {}


def _rows(hd, bs, nkv, n):
    """Random K / V rows [bs, n, nkv, hd] float32 and their 4-bit code buffers (through the append kernel), computed once
    per shape and left alone."""
    key = (hd, bs, nkv, n)
    if key not in _ROWS:
        g = torch.Generator(device=DEV).manual_seed(hd + 7 * bs + 13 * nkv + n)
        k = torch.randn(bs, n, nkv, hd, generator=g, device=DEV) * 1.5
        v = torch.randn(bs, n, nkv, hd, generator=g, device=DEV) + 0.5
        kc = torch.empty(bs, nkv, n, hd // 2, dtype=torch.uint8, device=DEV)
        km = torch.empty(bs, nkv, n, 2, dtype=F32, device=DEV)
        codes = (kc, kc.clone(), km, km.clone())
        ops.kv_append_codes(k, v, F32, *codes, past=0)
        _ROWS[key] = (k.transpose(1, 2).contiguous(), v.transpose(1, 2).contiguous(), codes)
    return _ROWS[key]


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("cache", ["bf16", "f32", "codes"])
def test_ragged_attention_uniform_lengths_is_the_uniform_kernel_bit_for_bit(cache, hd):
    nh, nkv, scale = 8, 2, 1.0 / math.sqrt(hd)
    cd = F32 if cache == "f32" else BF16
    for bs in (1, 3):
        kf, vf, codes = _rows(hd, bs, nkv, 2049)
        g = torch.Generator(device=DEV).manual_seed(bs)
        q = torch.randn(bs, 1, nh, hd, generator=g, device=DEV).to(cd)
        for L in (1, 128, 129, 257, 2049):
            lens = _i32([L - 1] * bs)
            if cache == "codes":
                bufs = tuple(t[:, :, :L].contiguous() for t in codes)
                ref = ops.decode_attention_codes(q, bufs, L, scale)
                a, b = (ops.decode_attention_codes(q, bufs, L, scale, lengths=lens) for _ in range(2))
            else:
                kc, vc = kf[:, :, :L].to(cd).contiguous(), vf[:, :, :L].to(cd).contiguous()
                ref = ops.decode_attention(q, kc, vc, L, scale)
                a, b = (ops.decode_attention(q, kc, vc, L, scale, lengths=lens) for _ in range(2))
            assert bool(torch.isfinite(ref).all()) and _same(a, ref) and _same(a, b), (cache, hd, bs, L)


def _ragged_ref64(q, kf, vf, lens, scale):
    """Per sequence and per query row: float64 softmax over rows [0, lens[b] + t] of the float32 values kf / vf
    [bs, nkv, cap, hd].  Returns (o, sum_j p_j |v_j|), each [bs, Tq, nh, hd] float64."""
    bs, Tq, nh, hd = q.shape
    rep = nh // kf.shape[1]
    o = torch.empty(q.shape, dtype=torch.float64, device=q.device)
    mag = torch.empty_like(o)
    for b, n in enumerate(lens):
        for t in range(Tq):
            k = kf[b, :, :n + t + 1].double().repeat_interleave(rep, dim=0)          # [nh, n + t + 1, hd]
            v = vf[b, :, :n + t + 1].double().repeat_interleave(rep, dim=0)
            p = torch.softmax(torch.einsum("hd,hjd->hj", q[b, t].double(), k) * scale, dim=-1)
            o[b, t] = torch.einsum("hj,hjd->hd", p, v)
            mag[b, t] = torch.einsum("hj,hjd->hd", p, v.abs())
    return o, mag


@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (64, 8)])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("Tq", [1, 4])
def test_ragged_attention_matches_float64_and_never_reads_invisible_rows(Tq, hd, heads):
    nh, nkv = heads
    bs, lens, scale = 3, [0, 130, 2047], 1.0 / math.sqrt(hd)
    Lb = 2047 + Tq
    cap = 2 * Lb
    kf, vf, codes = _rows(hd, bs, nkv, Lb)
    lens_t = _i32(lens)
    g = torch.Generator(device=DEV).manual_seed(nh + Tq)
    q32 = torch.randn(bs, Tq, nh, hd, generator=g, device=DEV)

    def poisoned(src, cap, fill):
        """src's rows [0, lens[b] + Tq) of each sequence in a buffer of `cap` rows whose every other row holds `fill`."""
        t = torch.full((bs, nkv, cap) + tuple(src.shape[3:]), fill, dtype=src.dtype, device=DEV)
        for b, n in enumerate(lens):
            t[b, :, :n + Tq] = src[b, :, :n + Tq]
        return t

    for cd in (BF16, F32):
        q = q32.to(cd)
        # float cache: rows no query of the sequence may see are NaN
        kc, vc = kf.to(cd), vf.to(cd)
        o = ops.decode_attention(q, poisoned(kc, cap, NAN), poisoned(vc, cap, NAN), Lb, scale, lengths=lens_t)
        ref, mag = _ragged_ref64(q, kc.float(), vc.float(), lens, scale)
        err = (o.double() - ref).abs()
        bound = UNIT[cd] * ref.abs() + 2e-5 * mag                       # the bound of test_hip_kv_decode._check
        print(f"ragged float {cd} hd {hd} heads {heads} Tq {Tq}: max (err - bound) {float((err - bound).max()):.3e}")
        assert o.dtype == cd and bool(torch.isfinite(o).all())
        assert bool((err <= bound).all()), (cd, float((err - bound).max()))
        o2 = ops.decode_attention(q, poisoned(kc, 2 * cap, NAN), poisoned(vc, 2 * cap, NAN), Lb, scale, lengths=lens_t)
        assert _same(o, o2)
        # code cache: codes 0xFF under NaN (scale, zero-point) in the invisible rows
        bufs = [poisoned(codes[0], cap, 0xFF), poisoned(codes[1], cap, 0xFF), poisoned(codes[2], cap, NAN),
                poisoned(codes[3], cap, NAN)]
        oc = ops.decode_attention_codes(q, bufs, Lb, scale, lengths=lens_t)
        refc, _ = _ragged_ref64(q, unpack_codes(codes[0], codes[2]), unpack_codes(codes[1], codes[3]), lens, scale)
        errc, top = float((oc.double() - refc).abs().max()), float(refc.abs().max())
        print(f"ragged codes {cd} hd {hd} heads {heads} Tq {Tq}: max err {errc:.3e} of max|ref| {top:.3e}")
        assert oc.dtype == cd and bool(torch.isfinite(oc).all())
        assert errc <= _code_bound(cd, top), (cd, errc, top)             # the bound test_hip_kv_codes asserts
        big = [poisoned(codes[0], 2 * cap, 0xFF), poisoned(codes[1], 2 * cap, 0xFF), poisoned(codes[2], 2 * cap, NAN),
               poisoned(codes[3], 2 * cap, NAN)]
        assert _same(oc, ops.decode_attention_codes(q, big, Lb, scale, lengths=lens_t))


@pytest.mark.parametrize("cache", ["f32", "codes"])
def test_ragged_attention_clamps_the_lengths_the_host_cannot_see(cache):
    """A negative length counts as 0 and a length above L_bound - Tq as L_bound - Tq: no query row is left without a key and
    nothing beyond row L_bound is read (NaN there).  The reference is the float64 softmax at the clamped lengths."""
    bs, Tq, nh, nkv, hd, Lb = 3, 2, 8, 2, 64, 140
    scale = 1.0 / math.sqrt(hd)
    lens, clamped = [-5, Lb + 7, 60], [0, Lb - Tq, 60]
    kf, vf, codes = _rows(hd, bs, nkv, Lb)
    g = torch.Generator(device=DEV).manual_seed(3)
    q = torch.randn(bs, Tq, nh, hd, generator=g, device=DEV)

    def padded(src, fill):
        t = torch.full((bs, nkv, Lb + 9) + tuple(src.shape[3:]), fill, dtype=src.dtype, device=DEV)
        t[:, :, :Lb] = src
        return t

    if cache == "codes":
        bufs = [padded(codes[0], 0xFF), padded(codes[1], 0xFF), padded(codes[2], NAN), padded(codes[3], NAN)]
        o = ops.decode_attention_codes(q, bufs, Lb, scale, lengths=_i32(lens))
        o2 = ops.decode_attention_codes(q, bufs, Lb, scale, lengths=_i32(clamped))
        ref, _ = _ragged_ref64(q, unpack_codes(codes[0], codes[2]), unpack_codes(codes[1], codes[3]), clamped, scale)
        err, top = float((o.double() - ref).abs().max()), float(ref.abs().max())
        assert bool(torch.isfinite(o).all()) and err <= _code_bound(F32, top), (err, top)
    else:
        o = ops.decode_attention(q, padded(kf, NAN), padded(vf, NAN), Lb, scale, lengths=_i32(lens))
        o2 = ops.decode_attention(q, padded(kf, NAN), padded(vf, NAN), Lb, scale, lengths=_i32(clamped))
        ref, mag = _ragged_ref64(q, kf, vf, clamped, scale)
        err = (o.double() - ref).abs()
        assert bool(torch.isfinite(o).all()) and bool((err <= UNIT[F32] * ref.abs() + 2e-5 * mag).all())
    assert _same(o, o2)


# ---------------------------------------------------------------------------------------------------------------------
# blocks: name -> (builder of the packed block, family, nh, nkv, cache code_bits, W4A4)
# ---------------------------------------------------------------------------------------------------------------------
H = 256
RAGGED_BLOCKS = {
    "wo_llama_gqa": (lambda: KD._block("llama_gqa")[2], "llama", 4, 2, None, False),
    "wo_opt": (lambda: KD._block("opt")[2], "opt", 4, 4, None, False),
    "a4_gqa": (lambda: A4._calibrated("gqa")[3], "llama", 4, 2, None, True),
    "a4_gqa_codes": (lambda: A4._calibrated("gqa")[3], "llama", 4, 2, 4, True),
    "a4_hd128_fused": (lambda: A4._calibrated("hd128_fused")[3], "llama", 2, 2, None, True),
    "a4_hd128_fused_codes": (lambda: A4._calibrated("hd128_fused")[3], "llama", 2, 2, 4, True),
}
PROMPTS, STEPS = [24, 16, 8], 8


def _x(bs, T, seed):
    from omniquant_amd.synthetic import make_calib_inputs
    return make_calib_inputs(bs, T, H, seed=seed, dtype=torch.float16).to(DEV)


def _step(blk, fam, x, cache, mask=None, pos=None, new_tokens=None):
    kw = dict(attention_mask=mask, past_key_value=cache, use_cache=True)
    if new_tokens is not None:
        kw["new_tokens"] = new_tokens
    if pos is not None and fam == "llama":
        kw["position_ids"] = pos
    with torch.no_grad():
        out, present = blk(x, **kw)
    assert present is cache
    return out


def _alone(blk, fam, x, use_cache=False):
    """One full, unpadded forward of one sequence (right-padded to the no-cache GEMMs' multiple of 8 under the causal mask,
    which keeps the pad rows away from the valid ones)."""
    n = x.shape[1]
    Tp = -(-n // 8) * 8
    if Tp != n:
        x = torch.cat([x, _x(1, Tp - n, 77)], dim=1)
    kw = dict(attention_mask=KD._causal(Tp), use_cache=use_cache)
    if fam == "llama":
        kw["position_ids"] = torch.arange(Tp, device=DEV)[None]
    with torch.no_grad():
        out = blk(x, **kw)
    return (out[0][:, :n],) + tuple(out[1:])


def _agree(got, ref, x, cd, a4):
    """The bounds the two block test files assert: test_hip_kv_decode._agree (weight-only), test_hip_packed_a4._agree (W4A4)."""
    if a4:
        A4._agree(got, ref, x, cd)
    else:
        KD._agree(got, ref, cd)


def _prefill_and_decode(name, cd):
    """Right-padded prefill of PROMPTS with new_tokens and the causal mask, then STEPS single-token steps without mask or
    positions.  Returns (block, family, cache, the sequences' inputs, each sequence's output rows so far)."""
    build, fam, nh, nkv, code_bits, a4 = RAGGED_BLOCKS[name]
    blk = build()
    blk.compute_dtype = cd
    Tp = max(PROMPTS)
    seqs = [_x(1, n + STEPS + 8, 30 + i) for i, n in enumerate(PROMPTS)]
    X = _x(3, Tp, 29)                  # the pad rows hold some token's hidden state (a zero row has scale 0 on W4A4: NaN)
    for i, n in enumerate(PROMPTS):
        X[i, :n] = seqs[i][0, :n]
    cache = PackedKVCache(3, nkv, H // nh, cd, DEV, capacity=Tp, code_bits=code_bits, ragged=True)
    out = _step(blk, fam, X, cache, KD._causal(Tp).expand(3, 1, Tp, Tp), torch.arange(Tp, device=DEV)[None], new_tokens=PROMPTS)
    assert cache.length == Tp
    rows = [[out[i:i + 1, :n]] for i, n in enumerate(PROMPTS)]
    for s in range(STEPS):
        xs = torch.stack([seqs[i][0, n + s] for i, n in enumerate(PROMPTS)])[:, None]
        o = _step(blk, fam, xs, cache)
        assert cache.length == Tp + s + 1
        for i in range(3):
            rows[i].append(o[i:i + 1])
    return blk, fam, cache, seqs, rows


@pytest.mark.parametrize("cd", [BF16, F32])
@pytest.mark.parametrize("name", list(RAGGED_BLOCKS))
def test_right_padded_prefill_then_maskless_decode_matches_each_sequence_alone(name, cd):
    a4 = RAGGED_BLOCKS[name][5]
    blk, fam, cache, seqs, rows = _prefill_and_decode(name, cd)
    try:
        assert "ragged" in repr(cache)
        for i, n in enumerate(PROMPTS):
            x = seqs[i][:, :n + STEPS]
            ref = _alone(blk, fam, x, use_cache=True)
            _agree(torch.cat(rows[i], dim=1), ref[0], x, cd, a4)
            k, v = cache.sequence(i)
            assert k.shape == v.shape == (cache.nkv, n + STEPS, cache.hd) and k.dtype == cd
            if not a4 and cd == F32:
                # fp32 weight-only blocks (LLaMA: rotation at the same positions; OPT: none): the same projections of the same
                # rows, so the rows a ragged run caches are the alone run's
                rk, rv = ref[1][0][0], ref[1][1][0]
                print(f"sequence {i}: cache rows vs alone run, max |dk| {float((k - rk).abs().max()):.3e}, "
                      f"max |dv| {float((v - rv).abs().max()):.3e}")
                assert _same(k, rk) and _same(v, rv)
    finally:
        blk.compute_dtype = BF16


def test_slot_reuse_and_mixed_chunk_sizes():
    name, cd = "wo_llama_gqa", F32
    blk, fam, cache, seqs, rows = _prefill_and_decode(name, cd)
    try:
        n0, n2 = PROMPTS[0] + STEPS, PROMPTS[2] + STEPS
        cache.set_lengths([n0, 0, n2])                  # slot 1 is recycled: a fresh 5-token prompt starts there
        assert cache.length == n0
        fresh = _x(1, 8, 55)
        seqs[1], rows[1] = fresh, []
        at = [n0, 0, n2]                                # rows consumed so far of each sequence's inputs
        X = _x(3, 5, 56)
        X[0, 0], X[1, :5], X[2, 0] = seqs[0][0, at[0]], fresh[0, :5], seqs[2][0, at[2]]
        o = _step(blk, fam, X, cache, new_tokens=[1, 5, 1])
        assert cache.length == n0 + 5
        for i, n in enumerate([1, 5, 1]):
            rows[i].append(o[i:i + 1, :n])
            at[i] += n
        for _ in range(2):
            xs = torch.stack([seqs[i][0, at[i]] for i in range(3)])[:, None]
            o = _step(blk, fam, xs, cache)
            for i in range(3):
                rows[i].append(o[i:i + 1])
                at[i] += 1
        assert at == [n0 + 3, 7, n2 + 3]
        for i in range(3):
            x = seqs[i][:, :at[i]]
            KD._agree(torch.cat(rows[i], dim=1), _alone(blk, fam, x)[0], cd)
        assert cache.lengths.tolist() == at             # read once, at the end
        assert [cache.sequence(i)[0].shape[1] for i in range(3)] == at
        # the device-tensor forms: set_lengths(tensor, bound=) and new_tokens as an int32 tensor, whose values the host never
        # reads (the bound grows by Tq).  Rewind every sequence by its last two tokens and replay them as one 2-row step.
        back = [n - 2 for n in at]
        cache.set_lengths(_i32(back), bound=max(back))
        assert cache.length == max(back)
        X2 = torch.cat([seqs[i][:, back[i]:at[i]] for i in range(3)])
        o = _step(blk, fam, X2, cache, new_tokens=_i32([2, 2, 2]))
        assert cache.length == max(back) + 2 and cache.lengths.tolist() == at
        for i in range(3):
            KD._agree(torch.cat(rows[i][:-2] + [o[i:i + 1]], dim=1), _alone(blk, fam, seqs[i][:, :at[i]])[0], cd)
    finally:
        blk.compute_dtype = BF16


def test_errors_stay_loud():
    blk = KD._block("llama_gqa")[2]
    opt = KD._block("opt")[2]
    _, fq, _ = KD._block("llama_gqa")
    T, nkv, hd = 8, 2, 64
    x = _x(3, T, 3)
    pos = torch.arange(T, device=DEV)[None]
    cache = PackedKVCache(3, nkv, hd, BF16, DEV, capacity=32, ragged=True)
    _step(blk, "llama", x, cache, KD._causal(T).expand(3, 1, T, T), pos, new_tokens=[8, 4, 2])
    before = (cache.length, cache.lengths.tolist())
    assert before == (8, [8, 4, 2])
    one = x[:, :1]
    with pytest.raises(OQError, match="takes no attention_mask"):          # a mask with a ragged cache that has a past
        _step(blk, "llama", one, cache, KD._causal(1, T))
    uniform = PackedKVCache(3, nkv, hd, BF16, DEV, capacity=32)
    for past in (None, uniform):                                            # new_tokens without a ragged cache
        with pytest.raises(OQError, match="new_tokens needs a ragged"):
            with torch.no_grad():
                blk(one, past_key_value=past, use_cache=True, new_tokens=[1, 1, 1])
    with pytest.raises(OQError, match="new_tokens needs"):
        with torch.no_grad():
            opt(one, use_cache=True, new_tokens=[1, 1, 1])
    with pytest.raises(OQError, match="new_tokens needs"):                 # the fake-quant calibration block
        with torch.no_grad():
            fq(x, attention_mask=KD._causal(T), position_ids=pos, new_tokens=[1, 1, 1])
    for bad in ([1, 1], [1, 1, 2], [1, -1, 1], [1.0, 1.0, 1.0], _i32([1, 1]), _i32([1, 1, 1]).long(), _i32([1, 1, 1]).cpu(), 1):
        with pytest.raises(OQError, match="new_tokens"):                    # wrong length, range, dtype or device
            _step(blk, "llama", one, cache, new_tokens=bad)
    for surface in (lambda: cache[0], lambda: cache[:], lambda: list(cache), lambda: cache.to_tuple(), lambda: cache.dequantize(),
                    lambda: tuple(t for t in cache)):
        with pytest.raises(OQError, match="ragged"):                        # the (k, v) tuple surface
            surface()
    with pytest.raises(OQError, match="ragged"):
        PackedKVCache.from_tuple((cache.k, cache.v), ragged=True)
    with pytest.raises(OQError):
        uniform.set_lengths([1, 1, 1])
    with pytest.raises(OQError):
        uniform.sequence(0)
    with pytest.raises(OQError, match="bound="):
        cache.set_lengths(_i32([1, 1, 1]))                                  # a device tensor needs an explicit bound
    with pytest.raises(OQError):
        cache.set_lengths([1, 1, 33])                                       # beyond the capacity
    q = torch.randn(3, 1, 4, hd, device=DEV).bfloat16()
    lens = _i32([1, 2, 3])
    for bad in (lens.cpu(), lens.long(), _i32([1, 2])):                     # lengths on the wrong device, dtype or shape
        with pytest.raises(OQError, match="lengths"):
            ops.decode_attention(q, cache.k, cache.v, 8, 0.125, lengths=bad)
        with pytest.raises(OQError, match="lengths"):
            ops.kv_append(q[:, :, :2], q[:, :, :2], cache.k, cache.v, 0, lengths=bad)
    with pytest.raises(OQError, match="bound L = 33"):                      # L_bound > cap
        ops.decode_attention(q, cache.k, cache.v, 33, 0.125, lengths=lens)
    with pytest.raises(OQError, match="excludes a mask"):
        ops.decode_attention(q, cache.k, cache.v, 8, 0.125, torch.zeros(1, 1, 1, 8, device=DEV), lengths=lens)
    # every refused step and call left the cache as it was; a clone carries the lengths
    assert (cache.length, cache.lengths.tolist()) == before
    c2 = cache.clone()
    assert c2.ragged and (c2.length, c2.lengths.tolist()) == before and _same(c2.sequence(1)[0], cache.sequence(1)[0])
    _step(blk, "llama", one, cache)
    assert (cache.length, cache.lengths.tolist()) == (9, [9, 5, 3]) and c2.lengths.tolist() == before[1]
    torch.cuda.synchronize()
