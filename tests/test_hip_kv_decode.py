"""Incremental decoding of the packed (real-quant) blocks: csrc/oq_decode.hip (oq_kv_append, oq_attn_decode), the
PackedKVCache and the blocks' past_key_value / use_cache contract (models/int_llama_layer.py:121-135,177,264-265,
models/int_opt_layer.py:110-121,343-344)."""
import copy
import math
from types import SimpleNamespace

import pytest
import torch

from omniquant_amd import OQError, ops
from omniquant_amd.kvcache import PackedKVCache
from omniquant_amd.llama_block import QuantLlamaAttention
from omniquant_amd.realquant import pack_block

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
LOWEST = torch.finfo(torch.float32).min
BIG_L = 64 * 128 + 109          # above the largest split threshold (64 splits of >= 128 rows)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def _hf_mask(bs, Tq, L, pads, dtype=torch.float16):
    """transformers-4.31-style additive mask [bs, 1, Tq, L]: causal over the last Tq positions plus left padding (the sum of
    the two finfo.min terms is -inf in fp16, as there)."""
    mn = torch.finfo(dtype).min
    past = L - Tq
    j = torch.arange(L)[None, :]
    t = torch.arange(Tq)[:, None]
    causal = torch.where(j > past + t, mn, 0.0).to(dtype)
    m = causal[None, None].repeat(bs, 1, 1, 1)
    for b, p in enumerate(pads):
        m[b, 0, :, :p] += torch.tensor(mn, dtype=dtype)
    return m.to(DEV)


def _case(dtype, hd, nh, nkv, bs, Tq, L, kind, cap=None, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    cap = cap or L
    q = torch.randn(bs, Tq, nh, hd, generator=g, device=DEV).to(dtype)
    kc = torch.randn(bs, nkv, cap, hd, generator=g, device=DEV).to(dtype)
    vc = torch.randn(bs, nkv, cap, hd, generator=g, device=DEV).to(dtype)
    mask = None
    if kind == "hf":
        past = L - Tq
        mask = _hf_mask(bs, Tq, L, [min(p, past) for p in (0, 2, 5)][:bs])
    elif kind == "broadcast":
        mask = (torch.randn(1, 1, Tq, L, generator=g, device=DEV) * 2.0).float()
    return q, kc, vc, mask


def _ref(q, kc, vc, L, scale, mask):
    """float64 softmax(max(scale q k^T + mask, lowest)) v over the first L cache rows, and sum_j p_j |v_j|."""
    nh, nkv = q.shape[2], kc.shape[1]
    k = kc[:, :, :L].double().repeat_interleave(nh // nkv, dim=1)
    v = vc[:, :, :L].double().repeat_interleave(nh // nkv, dim=1)
    s = torch.einsum("bthd,bhld->bhtl", q.double(), k) * scale
    if mask is not None:
        s = torch.clamp(s + mask.double(), min=LOWEST)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhtl,bhld->bthd", p, v), torch.einsum("bhtl,bhld->bthd", p, v.abs())


def _check(dtype, hd, nh, nkv, bs, Tq, L, kind):
    q, kc, vc, mask = _case(dtype, hd, nh, nkv, bs, Tq, L, kind, seed=bs * 1000 + Tq * 10 + L)
    scale = 1.0 / math.sqrt(hd)
    o = ops.decode_attention(q, kc, vc, L, scale, mask)
    ref, mag = _ref(q, kc, vc, L, scale, mask)
    # fp32 scores / online softmax / accumulation: a few fp32 ulps of the scores move p by ~1e-6 relative, i.e. 1e-6 of
    # sum p|v|; then ONE rounding of the output to its dtype (half an ulp of |o|)
    bound = UNIT[dtype] * ref.abs() + 2e-5 * mag
    err = (o.double() - ref).abs()
    assert o.dtype == dtype and o.shape == q.shape and bool(torch.isfinite(o).all())
    assert bool((err <= bound).all()), (bs, Tq, L, kind, float((err - bound).max()))


@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (64, 8)])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_decode_attention_matches_float64(dtype, hd, heads):
    nh, nkv = heads
    for bs in (1, 3):
        for Tq in (1, 4, 16, 33):
            for L in sorted({Tq, Tq + 1, 255, 256, 257, 2048 + Tq}):
                if L < Tq:
                    continue
                for kind in ("none", "hf", "broadcast"):
                    _check(dtype, hd, nh, nkv, bs, Tq, L, kind)
    for kind in ("none", "hf"):
        _check(dtype, hd, nh, nkv, 3, 4, BIG_L, kind)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_decode_attention_deterministic_cap_independent_and_bounded(dtype):
    for nh, nkv, hd, bs, Tq, L, kind in ((8, 2, 128, 3, 1, 3000, "hf"), (64, 8, 128, 1, 4, BIG_L, "none"),
                                         (4, 4, 64, 3, 16, 257, "broadcast"), (32, 32, 128, 1, 1, 9000, "none")):
        q, kc, vc, mask = _case(dtype, hd, nh, nkv, bs, Tq, L, kind, seed=L)
        a = ops.decode_attention(q, kc, vc, L, 0.125, mask)
        b = ops.decode_attention(q, kc, vc, L, 0.125, mask)
        assert _same(a, b)
        # the same rows in a cache of twice the capacity whose rows >= L are NaN: never read, same bits
        kc2 = torch.full((bs, nkv, 2 * L, hd), float("nan"), dtype=dtype, device=DEV)
        vc2 = torch.full_like(kc2, float("nan"))
        kc2[:, :, :L], vc2[:, :, :L] = kc, vc
        c = ops.decode_attention(q, kc2, vc2, L, 0.125, mask)
        assert bool(torch.isfinite(c).all()) and _same(a, c)


def _rope_ref_tables(pos_row, hd, theta=10000.0):
    """cos / sin of the given positions with the formula of QuantLlamaAttention._rope_tables (restated)."""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float32, device=DEV) / hd))
    fr = torch.outer(pos_row.to(device=DEV, dtype=torch.float32), inv)
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().contiguous(), emb.sin().contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("hd", [64, 128])
def test_kv_append_matches_rope_and_touches_only_its_rows(dtype, hd):
    bs, Tq, nh, nkv, past, cap = 3, 5, 8, 2, 11, 24
    g = torch.Generator(device=DEV).manual_seed(hd)
    q = torch.randn(bs, Tq, nh, hd, generator=g, device=DEV).to(dtype)
    k = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV).to(dtype)
    v = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV).to(dtype)
    attn = SimpleNamespace(rope_theta=10000.0, head_dim=hd, max_position_embeddings=64)
    cos, sin = QuantLlamaAttention._rope_table(attn, past + Tq, DEV)
    shared = torch.arange(past, past + Tq, device=DEV)[None]
    per_sample = torch.stack([torch.arange(past, past + Tq) - 3, torch.arange(past, past + Tq), torch.arange(Tq) * 7 + 2]).to(DEV)
    for pos in (shared, per_sample):
        kc = torch.full((bs, nkv, cap, hd), 12345.0, dtype=dtype, device=DEV)
        vc = torch.full_like(kc, -777.0)
        kc0, vc0 = kc.clone(), vc.clone()
        qo = ops.kv_append(k, v, kc, vc, past, q=q, q_out=torch.empty_like(q), cos=cos, sin=sin, positions=pos)
        for b in range(bs):
            c, s = _rope_ref_tables(pos[b if pos.shape[0] > 1 else 0], hd)
            assert _same(qo[b:b + 1], ops.RopeFn.apply(q[b:b + 1], c, s))
            assert _same(kc[b, :, past:past + Tq], ops.RopeFn.apply(k[b:b + 1], c, s)[0].transpose(0, 1))
        assert _same(vc[:, :, past:past + Tq], v.transpose(1, 2))
        for t, t0 in ((kc, kc0), (vc, vc0)):
            assert _same(t[:, :, :past], t0[:, :, :past]) and _same(t[:, :, past + Tq:], t0[:, :, past + Tq:])


# ---------------------------------------------------------------------------------------------------------------------
# blocks (the calibrate -> pack_block fixtures of test_hip_packed.py, restated)
# ---------------------------------------------------------------------------------------------------------------------
BLOCKS = {"llama_base": ("llama", 256, 64, 2, 2), "llama_gqa": ("llama", 256, 64, 4, 2),
          "llama_hd128_fused": ("llama", 256, 256, 2, 2), "opt": ("opt", 256, 64, 4, 4)}
_BUILT = {}


def _calibrated(family, H, T, heads, kv_heads, wbits=4, group=64, seed=2):
    from omniquant_amd.calibrate import calibrate_layers, default_args
    from omniquant_amd.synthetic import causal_mask, make_calib_inputs, make_config, make_layer
    cfg = make_config(None, family=family, hidden_size=H, inter=2 * H, heads=heads, kv_heads=kv_heads)
    args = default_args(wbits=wbits, abits=16, group_size=group, lwc=True, let=False, epochs=1, nsamples=2, net=family,
                        real_quant=False)
    x = make_calib_inputs(2, T, H, dtype=torch.float16).to(DEV)
    mask = causal_mask(T).to(DEV)
    pos = torch.arange(T, device=DEV)[None] if family == "llama" else None
    layer = make_layer(cfg, seed=seed, device=DEV, outliers=False)
    qlayers, _, _, _ = calibrate_layers([layer], cfg, args, x, mask, pos, use_graph=False)
    return cfg, qlayers[0]


def _block(name):
    if name not in _BUILT:
        fam, H, T, nh, nkv = BLOCKS[name]
        cfg, fq = _calibrated(fam, H, T, nh, nkv)
        _BUILT[name] = (cfg, fq, pack_block(copy.deepcopy(fq), 4))
    return _BUILT[name]


def _causal(T, past=0, dtype=torch.float32):
    """additive [1, 1, T, past + T] mask: row t sees columns <= past + t."""
    j = torch.arange(past + T)[None, :]
    t = torch.arange(T)[:, None]
    return torch.where(j > past + t, torch.finfo(dtype).min, 0.0).to(dtype)[None, None].to(DEV)


def _fwd(blk, x, mask=None, pos=None, past=None, use_cache=False):
    kw = dict(attention_mask=mask, past_key_value=past, use_cache=use_cache)
    if pos is not None and isinstance(blk.self_attn, QuantLlamaAttention):
        kw["position_ids"] = pos
    with torch.no_grad():
        return blk(x, **kw)


def _is_llama(name):
    return BLOCKS[name][0] == "llama"


def _inputs(name, bs, T, seed):
    from omniquant_amd.synthetic import make_calib_inputs
    return make_calib_inputs(bs, T, BLOCKS[name][1], seed=seed, dtype=torch.float16).to(DEV)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_prefill_with_cache_is_bit_identical_and_present_is_k_proj_rope(name):
    cfg, _, pk = _block(name)
    T, nh, nkv = BLOCKS[name][2], BLOCKS[name][3], BLOCKS[name][4]
    hd = BLOCKS[name][1] // nh
    for cd in (torch.bfloat16, torch.float32):
        pk.compute_dtype = cd
        x = _inputs(name, 2, T, 11)
        mask = _causal(T).expand(2, 1, T, T)
        pos = torch.arange(T, device=DEV)[None]
        a = _fwd(pk, x, mask, pos)
        out = _fwd(pk, x, mask, pos, use_cache=True)
        assert len(a) == 1 and len(out) == 2 and isinstance(out[1], PackedKVCache)
        assert _same(a[0], out[0])
        present = out[1]
        assert present.length == T and present[0].shape == (2, nkv, T, hd) and present[0].dtype == cd
        with torch.no_grad():
            xe = ops.cast(x, cd)
            if _is_llama(name):
                h = pk.input_layernorm(xe)
                k = pk.self_attn.k_proj(h).view(2, T, nkv, hd)
                cos, sin = pk.self_attn._rope_tables(pos, T, DEV)
                k = ops.RopeFn.apply(k, cos, sin)
            else:
                h = pk.self_attn_layer_norm(xe)
                k = pk.self_attn.k_proj(h).view(2, T, nkv, hd)
            v = pk.self_attn.v_proj(h).view(2, T, nkv, hd)
        assert _same(present[0], k.transpose(1, 2)) and _same(present[1], v.transpose(1, 2))
    pk.compute_dtype = torch.bfloat16


def _agree(inc, ref, cd):
    inc, ref = inc.float(), ref.float()
    assert inc.shape == ref.shape and bool(torch.isfinite(inc).all())
    err, top = float((inc - ref).abs().max()), float(ref.abs().max())
    if cd == torch.float32:
        # same weights, same fp32 products: only the summation order of the attention differs
        assert err <= 1e-4 * top, (err, top)
    else:
        # the bar of test_hip_packed._block_parity: a few bf16 ulps of the output (the decode rows take the gemv, the full
        # sequence the GEMM; the attention sums in another order)
        cos = float(torch.nn.functional.cosine_similarity(inc.flatten(), ref.flatten(), dim=0))
        assert cos >= 0.9999 and err <= 2e-2 * top, (cos, err, top)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_incremental_decode_matches_full_sequence(name):
    cfg, _, pk = _block(name)
    T0 = 200 if name == "llama_hd128_fused" else 40
    chunks = [1, 1, 1, 5, 1, 1, 1, 1, 4]       # (full-sequence lengths stay multiples of 8, as the no-cache GEMMs need)
    N = T0 + sum(chunks)
    for cd in (torch.bfloat16, torch.float32):
        pk.compute_dtype = cd
        x = _inputs(name, 1, N, 5)
        pos = torch.arange(N, device=DEV)[None]
        ref = _fwd(pk, x, _causal(N), pos)[0]
        out, cache = _fwd(pk, x[:, :T0], _causal(T0), pos[:, :T0], use_cache=True)
        outs, p = [out], T0
        for i, n in enumerate(chunks):
            mask = _causal(n, p) if (n > 1 or i % 2) else None      # single tokens: mask or none (equivalent)
            o, cache2 = _fwd(pk, x[:, p:p + n], mask, None if i == 2 else pos[:, p:p + n], past=cache, use_cache=True)
            assert cache2 is cache and cache.length == p + n       # appended in place
            outs.append(o)
            p += n
        _agree(torch.cat(outs, dim=1), ref, cd)
    pk.compute_dtype = torch.bfloat16


def test_tuple_past_equals_packed_cache_and_is_left_alone():
    cfg, _, pk = _block("llama_gqa")
    T0, n = 32, 3
    x = _inputs("llama_gqa", 2, T0 + n, 7)
    pos = torch.arange(T0 + n, device=DEV)[None]
    _, cache = _fwd(pk, x[:, :T0], _causal(T0).expand(2, 1, T0, T0), pos[:, :T0], use_cache=True)
    tup = cache.to_tuple()
    snap = [t.clone() for t in tup]
    c2 = cache.clone()
    m = _causal(n, T0)
    a, pa = _fwd(pk, x[:, T0:], m, pos[:, T0:], past=tup, use_cache=True)
    b, pb = _fwd(pk, x[:, T0:], m, pos[:, T0:], past=c2, use_cache=True)
    assert pb is c2 and isinstance(pa, PackedKVCache) and pa.length == pb.length == T0 + n
    assert _same(a, b) and _same(pa[0], pb[0]) and _same(pa[1], pb[1])
    assert all(_same(t, s) for t, s in zip(tup, snap))
    # another float dtype is converted once; the caller's tensors are still not touched
    t16 = tuple(t.half() for t in tup)
    s16 = [t.clone() for t in t16]
    c, pc = _fwd(pk, x[:, T0:], m, pos[:, T0:], past=t16, use_cache=True)
    assert bool(torch.isfinite(c).all()) and pc.dtype == torch.bfloat16
    assert all(_same(t, s) for t, s in zip(t16, s16))
    # HF's beam _reorder_cache: index_select over the iterated cache gives a tuple the tuple path accepts
    beam = torch.tensor([1, 0], device=DEV)
    reordered = tuple(t.index_select(0, beam) for t in cache)
    assert len(cache) == 2 and cache[0].shape[2] == T0
    _fwd(pk, x[:, T0:], m, pos[:, T0:], past=reordered, use_cache=True)


def test_grown_cache_is_bit_identical_to_preallocated():
    cfg, _, pk = _block("llama_base")
    nh, nkv, hd = 2, 2, 128
    T0, steps = 16, 12
    x = _inputs("llama_base", 1, T0 + steps, 9)
    pre = PackedKVCache(1, nkv, hd, torch.bfloat16, DEV, capacity=T0 + steps)
    small = PackedKVCache(1, nkv, hd, torch.bfloat16, DEV, capacity=4)
    res = []
    for c in (pre, small):
        outs = [_fwd(pk, x[:, :T0], _causal(T0), None, past=c, use_cache=True)[0]]
        for p in range(T0, T0 + steps):
            outs.append(_fwd(pk, x[:, p:p + 1], None, None, past=c, use_cache=True)[0])
        res.append(torch.cat(outs, dim=1))
    assert small.capacity >= T0 + steps and pre.capacity == T0 + steps
    assert _same(res[0], res[1]) and _same(pre[0], small[0]) and _same(pre[1], small[1])


@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float32])
def test_left_padded_batch_matches_each_sample_alone(cd):
    cfg, _, pk = _block("llama_gqa")
    pk.compute_dtype = cd
    lens, steps = [24, 16, 8], 8
    Tp = max(lens)
    seqs = [_inputs("llama_gqa", 1, n + steps, 30 + i) for i, n in enumerate(lens)]
    X = torch.zeros(3, Tp, BLOCKS["llama_gqa"][1], dtype=torch.float16, device=DEV)
    am = torch.zeros(3, Tp, dtype=torch.int64, device=DEV)
    for i, n in enumerate(lens):
        X[i, Tp - n:] = seqs[i][0, :n]
        am[i, Tp - n:] = 1

    def hf_mask(am, Tq):
        L = am.shape[1]
        mn = torch.finfo(torch.float16).min
        causal = _causal(Tq, L - Tq, torch.float16)
        pad = (1 - am[:, None, None, :].to(torch.float16)) * mn
        return causal + pad                                      # (-inf where both apply, as transformers 4.31 builds it)

    def pos_of(am):
        p = am.cumsum(-1) - 1
        return p.masked_fill(am == 0, 1)

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
        _agree(got, ref, cd)
    pk.compute_dtype = torch.bfloat16


# ---- greedy generation: the three-layer synthetic LM of test_hip_packed.py, 2 heads of 64 -----------------------------
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
    args = default_args(wbits=4, abits=16, group_size=64, lwc=True, let=False, epochs=2, nsamples=NSAMP, net="llama")
    hip_layers = [make_layer(cfg, weights=dict(w), device=DEV) for w in layers]
    qlayers, _, _, _ = calibrate_layers(hip_layers, cfg, args, emb[tokens].to(DEV), mask, pos, use_graph=False,
                                        compute_dtype=torch.float32)
    packed = [pack_block(copy.deepcopy(q), 4) for q in qlayers]
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
    for step in range(24):
        T = len(seq)
        Tp = -(-T // 8) * 8                 # right-padded to the no-cache GEMMs' multiple of 8: causal rows < T never see it
        hf = emb_d[torch.tensor(seq + [0] * (Tp - T), device=DEV)][None]
        for blk in packed:
            hf = _fwd(blk, hf, _causal(Tp), torch.arange(Tp, device=DEV)[None])[0]
        lf = logits(hf[0, T - 1])
        diff = float((lc - lf).abs().max())
        top2 = torch.topk(lf, 2).values
        assert float(top2[0] - top2[1]) > 2 * diff, (step, float(top2[0] - top2[1]), diff)   # no near-tie can flip the pick
        tok_c, tok_f = int(lc.argmax()), int(lf.argmax())
        assert tok_c == tok_f, step
        seq.append(tok_f)
        hs = emb_d[tok_f][None, None]
        for i, blk in enumerate(packed):
            hs, caches[i] = _fwd(blk, hs, None, torch.tensor([[T]], device=DEV), past=caches[i], use_cache=True)
        lc = logits(hs[0, -1])
    assert len(seq) == 16 + 24


# ---- errors stay loud ----------------------------------------------------------------------------------------------
def test_errors_stay_loud():
    cfg, fq, pk = _block("llama_gqa")
    _, _, po = _block("opt")
    T = 8
    x = _inputs("llama_gqa", 1, T, 3)
    pos = torch.arange(T, device=DEV)[None]
    with pytest.raises(NotImplementedError):
        with torch.no_grad():
            pk(x, attention_mask=_causal(T), position_ids=pos, output_attentions=True)
    with pytest.raises(NotImplementedError):
        with torch.no_grad():
            pk(x, attention_mask=_causal(T), position_ids=pos, output_attentions=True, use_cache=True)
    with pytest.raises(NotImplementedError):                 # the fake-quant calibration block keeps its refusal
        with torch.no_grad():
            fq(x, attention_mask=_causal(T), position_ids=pos, use_cache=True)
    with pytest.raises(NotImplementedError):
        with torch.no_grad():
            po(_inputs("opt", 1, T, 3), attention_mask=_causal(T), layer_head_mask=torch.ones(4, device=DEV), use_cache=True)
    _, cache = _fwd(pk, x, _causal(T), pos, use_cache=True)
    with pytest.raises(ValueError, match="Attention mask should be of size"):
        _fwd(pk, x[:, :1], _causal(1, T + 1), pos[:, :1] + T, past=cache, use_cache=True)
    assert cache.length == T                                  # a refused step leaves the cache as it was
    with pytest.raises(OQError):                              # batch mismatch
        _fwd(pk, _inputs("llama_gqa", 2, 1, 4), None, None, past=cache, use_cache=True)
    with pytest.raises(OQError):                              # heads mismatch
        _fwd(pk, x[:, :1], None, None, past=PackedKVCache(1, 4, 64, torch.bfloat16, DEV, 16), use_cache=True)
    with pytest.raises(OQError):
        PackedKVCache(1, 2, 64, torch.bfloat16, "cpu")
    q = torch.randn(1, 1, 4, 64, device=DEV).bfloat16()
    kc = torch.randn(1, 4, 16, 64, device=DEV).bfloat16()
    with pytest.raises(OQError):
        ops.decode_attention(q.cpu(), kc.cpu(), kc.cpu(), 8, 0.125)
    with pytest.raises(OQError):
        ops.decode_attention(q, kc, kc, 8, 0.125, torch.zeros(1, 1, 1, 8))          # CPU mask
    q32 = torch.randn(1, 1, 4, 32, device=DEV).bfloat16()
    kc32 = torch.randn(1, 4, 16, 32, device=DEV).bfloat16()
    with pytest.raises(OQError):                              # head_dim the decode kernel does not cover
        ops.decode_attention(q32, kc32, kc32, 8, 0.125)
    with pytest.raises(OQError):                              # L beyond the cache
        ops.decode_attention(q, kc, kc, 17, 0.125)
    torch.cuda.synchronize()
