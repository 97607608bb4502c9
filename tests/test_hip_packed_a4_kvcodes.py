"""W4A4 packed LLaMA blocks on a KV cache stored as 4-bit codes (realquant.pack_block(..., act_quant=True, kv_cache_bits=4)):
the prefill is the no-cache forward bit for bit, decoding matches the full-sequence forward and the float-cache decoding, and
the code cache dequantises to the float cache's rows bit for bit.  Blocks, inputs and bounds are those of test_hip_packed_a4.py."""
import copy

import pytest
import torch

from omniquant_amd import OQError
from omniquant_amd.kvcache import PackedKVCache
from omniquant_amd.realquant import load_packed_block, pack_block
from test_hip_packed_a4 import LLAMA_SHAPES, _agree, _calibrated, _causal, _fwd, _same, _x

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNKS = [1, 1, 1, 1, 3, 1]
_CODED = {}


def _coded(shape):
    """(the block packed with kv_cache_bits=4, the same block packed without) of test_hip_packed_a4._calibrated(shape)."""
    if shape not in _CODED:
        cfg, args, fq, pk, mask, pos = _calibrated(shape)
        _CODED[shape] = (pack_block(copy.deepcopy(fq), 4, act_quant=True, kv_cache_bits=4), pk)
    return _CODED[shape]


def _decode(blk, x, T0, past=None):
    """Prefill of x[:, :T0] then the CHUNKS steps (masks and positions varied as in test_hip_packed_a4); returns the
    concatenated outputs and the cache."""
    N = x.shape[1]
    p_ = torch.arange(N, device=DEV)[None]
    o, cache = _fwd(blk, x[:, :T0], _causal(T0), p_[:, :T0], past=past, use_cache=True)
    outs, p = [o], T0
    for i, n in enumerate(CHUNKS):
        m = _causal(n, p) if (n > 1 or i % 2) else None
        o, c2 = _fwd(blk, x[:, p:p + n], m, None if i == 2 else p_[:, p:p + n], past=cache, use_cache=True)
        assert c2 is cache and cache.length == p + n
        outs.append(o)
        p += n
    return torch.cat(outs, dim=1), cache


@pytest.mark.parametrize("shape", list(LLAMA_SHAPES))
def test_prefill_is_bit_identical_and_decode_on_codes_matches_full(shape):
    ck, pk = _coded(shape)
    H, T, nh, nkv = LLAMA_SHAPES[shape]
    hd = H // nh
    T0 = 200 if shape == "hd128_fused" else 40
    N = T0 + sum(CHUNKS)
    for cd in (torch.bfloat16, torch.float32):
        ck.compute_dtype = pk.compute_dtype = cd
        xb = _x(2, T, 11)
        mb = _causal(T).expand(2, 1, T, T)
        pos = torch.arange(T, device=DEV)[None]
        a = _fwd(ck, xb, mb, pos)
        out = _fwd(ck, xb, mb, pos, use_cache=True)
        assert len(a) == 1 and len(out) == 2 and _same(a[0], out[0]) and _same(a[0], _fwd(pk, xb, mb, pos)[0])
        present = out[1]
        assert isinstance(present, PackedKVCache) and present.code_bits == 4 and present.length == T
        assert present.k_codes.shape == (2, nkv, present.capacity, hd // 2) and present.k_codes.dtype == torch.uint8
        assert present[0].shape == (2, nkv, T, hd) and present[0].dtype == cd
        # a block packed without the option still returns today's cache kind
        assert _fwd(pk, xb, mb, pos, use_cache=True)[1].code_bits is None
        x = _x(1, N, 5)
        ref = _fwd(ck, x, _causal(N), torch.arange(N, device=DEV)[None])[0]
        got, cache = _decode(ck, x, T0)
        assert cache.code_bits == 4
        print(f"code cache, {shape}:", end=" ")
        _agree(got, ref, x, cd)
    ck.compute_dtype = pk.compute_dtype = torch.bfloat16


@pytest.mark.parametrize("shape", list(LLAMA_SHAPES))
def test_code_cache_decoding_equals_float_cache_decoding_fp32(shape):
    ck, pk = _coded(shape)
    T0 = 200 if shape == "hd128_fused" else 40
    ck.compute_dtype = pk.compute_dtype = torch.float32
    x = _x(1, T0 + sum(CHUNKS), 5)
    a, ca = _decode(pk, x, T0)
    b, cb = _decode(ck, x, T0)
    err, top = float((a.float() - b.float()).abs().max()), float(a.float().abs().max())
    print(f"code cache vs float cache, {shape}, fp32: max err {err:.3e} of max {top:.3e}")
    assert err <= 1e-4 * top
    assert ca.code_bits is None and cb.code_bits == 4 and ca.length == cb.length
    k, v = cb.dequantize()
    assert _same(k, ca[0]) and _same(v, ca[1])
    # an empty pre-sized code cache makes the unmarked block decode on codes; a raw tuple is converted to the block's kind
    c, cc = _decode(pk, x, T0, past=PackedKVCache(1, ca.nkv, ca.hd, torch.float32, DEV, x.shape[1], code_bits=4))
    assert cc.code_bits == 4 and _same(c, b)
    n = x.shape[1] - 1
    raw = tuple(t[:, :, :n].clone() for t in ca.to_tuple())
    o, ct = _fwd(ck, x[:, n:], None, torch.tensor([[n]], device=DEV), past=raw, use_cache=True)
    assert ct.code_bits == 4 and ct.length == n + 1          # (the rows were quantised again on import: close, not bit-equal)
    _agree(o, b[:, n:], x[:, n:], torch.float32)
    ck.compute_dtype = pk.compute_dtype = torch.bfloat16


@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float32])
def test_left_padded_batch_on_codes_matches_each_sample_alone(cd):
    ck, _ = _coded("gqa")
    ck.compute_dtype = cd
    lens, steps = [24, 16], 8
    Tp = max(lens)
    seqs = [_x(1, n + steps, 30 + i) for i, n in enumerate(lens)]
    X = _x(2, Tp, 29)                         # the pad positions hold some token's hidden state (a zero row has scale 0: NaN)
    am = torch.zeros(2, Tp, dtype=torch.int64, device=DEV)
    for i, n in enumerate(lens):
        X[i, Tp - n:] = seqs[i][0, :n]
        am[i, Tp - n:] = 1

    def hf_mask(am, Tq):
        mn = torch.finfo(torch.float16).min
        return _causal(Tq, am.shape[1] - Tq, torch.float16) + (1 - am[:, None, None, :].to(torch.float16)) * mn

    def pos_of(am):
        return (am.cumsum(-1) - 1).masked_fill(am == 0, 1)

    out, cache = _fwd(ck, X, hf_mask(am, Tp), pos_of(am), use_cache=True)
    assert cache.code_bits == 4
    step_outs = []
    for s in range(steps):
        xs = torch.stack([seqs[i][0, n + s] for i, n in enumerate(lens)])[:, None]
        am = torch.cat([am, torch.ones(2, 1, dtype=torch.int64, device=DEV)], dim=1)
        o, cache = _fwd(ck, xs, hf_mask(am, 1), pos_of(am)[:, -1:], past=cache, use_cache=True)
        step_outs.append(o)
    for i, n in enumerate(lens):
        ref = _fwd(ck, seqs[i], _causal(n + steps), torch.arange(n + steps, device=DEV)[None])[0]
        got = torch.cat([out[i:i + 1, Tp - n:]] + [o[i:i + 1] for o in step_outs], dim=1)
        _agree(got, ref, seqs[i], cd)
    ck.compute_dtype = torch.bfloat16


def test_load_packed_block_with_kv_cache_bits_reproduces_pack_block():
    from omniquant_amd.calibrate import decoder_layer_class
    from omniquant_amd.synthetic import make_layer
    cfg, args, fq, pk, mask, pos = _calibrated("gqa")
    ck, _ = _coded("gqa")
    fresh = decoder_layer_class("llama")(cfg, make_layer(cfg, seed=99, device=DEV), args).to(DEV)
    load_packed_block(fresh, {k: v.clone() for k, v in ck.state_dict().items()}, 4, None, act_quant=True, kv_cache_bits=4)
    with pytest.raises(OQError, match="act_quant"):
        load_packed_block(decoder_layer_class("llama")(cfg, make_layer(cfg, seed=99, device=DEV), args).to(DEV),
                          {k: v.clone() for k, v in ck.state_dict().items()}, 4, None, kv_cache_bits=4)
    x = _x(1, 40 + sum(CHUNKS), 4)
    for cd in (torch.bfloat16, torch.float32):
        ck.compute_dtype = fresh.compute_dtype = cd
        a, ca = _decode(ck, x, 40)
        b, cb = _decode(fresh, x, 40)
        assert cb.code_bits == 4 and _same(a, b) and all(_same(s, t) for s, t in zip(ca.dequantize(), cb.dequantize()))
    ck.compute_dtype = torch.bfloat16
