"""Chunked-prefill ("extend") attention over the ragged and the paged KV cache (csrc/oq_extend.hip): the MFMA kernel against a
float64 softmax, the rows it must never read, the lengths it clamps, paged == slab bit for bit, and the block forwards that
route long steps with a past to it."""
import math

import pytest
import torch

import test_hip_kv_decode as KD
import test_hip_kv_ragged as RG
from omniquant_amd import OQError, block_common, ops
from omniquant_amd.kvcache import PackedKVCache, PagedKVCache, unpack_codes
from test_hip_kv_paged import UNIT, _perm, _pool_of, _slab
from test_hip_kv_ragged import PROMPTS, RAGGED_BLOCKS, _i32, _ragged_ref64, _rows, _same, _x

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
NROWS = 1152                    # >= 700 + 130 + 300, a multiple of every page size
# (lens, what L exceeds max(lens) + Tq by): no past and a diagonal in the first key tile; key-tile edges; several splits, some
# of them empty for the short sequences
LENS = (([0, 5, 130], 0), ([63, 64, 65], 0), ([0, 130, 700], 300))
KINDS = ("bf16", "codes")


def _values(kind, hd, nkv):
    """The cache rows of a kind as contiguous buffers [3, nkv, NROWS, ...] and the float32 values they stand for."""
    kf, vf, codes = _rows(hd, 3, nkv, NROWS)
    if kind == "codes":
        return list(codes), unpack_codes(codes[0], codes[2]), unpack_codes(codes[1], codes[3])
    kc, vc = kf.to(BF16), vf.to(BF16)
    return [kc, vc], kc.float(), vc.float()


def _query(hd, nh, Tq):
    g = torch.Generator(device=DEV).manual_seed(3 * nh + Tq)
    return torch.randn(3, Tq, nh, hd, generator=g, device=DEV).to(BF16)


def _extend(kind, q, bufs, L, scale, lens, table=None):
    kw = {} if table is None else {"page_table": torch.tensor(table, dtype=torch.int32, device=DEV)}
    if kind == "codes":
        return ops.extend_attention_codes(q, tuple(bufs), L, scale, _i32(lens), **kw)
    return ops.extend_attention(q, bufs[0], bufs[1], L, scale, _i32(lens), **kw)


@pytest.mark.parametrize("Tq", [16, 17, 40, 130])
@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (6, 1)])
@pytest.mark.parametrize("hd", [64, 128])
def test_extend_attention_matches_float64(hd, heads, Tq):
    """|o - ref| <= UNIT[bf16] |ref| + (2^-8 + 2e-5) mag, mag = sum_j p_j |v_j|: one rounding of the output; the un-normalised
    probabilities (code caches: p * s_v) rounded to bf16 once in front of the PV product (2^-9 mag); the same again should the
    row sum come from the rounded values; the fp32 summation term of the decode tests (2e-5 mag)."""
    nh, nkv = heads
    scale = 1.0 / math.sqrt(hd)
    q = _query(hd, nh, Tq)
    for kind in KINDS:
        bufs, kf, vf = _values(kind, hd, nkv)
        for lens, extra in LENS:
            L = max(lens) + Tq + extra
            o = _extend(kind, q, [_slab(t, L) for t in bufs], L, scale, lens)
            ref, mag = _ragged_ref64(q, kf, vf, lens, scale)
            err = (o.double() - ref).abs()
            bound = UNIT[BF16] * ref.abs() + (2.0 ** -8 + 2e-5) * mag
            print(f"extend {kind} hd {hd} heads {heads} Tq {Tq} lens {lens}: max err {float(err.max()):.3e}, "
                  f"max (err - bound) {float((err - bound).max()):.3e}")
            assert o.dtype == BF16 and bool(torch.isfinite(o).all())
            assert bool((err <= bound).all()), (kind, lens, float((err - bound).max()))


def _scatter_held(pool, table, slab, held):
    """Write the first held[b] pages of each sequence's slab [bs, nkv, rows, x] into the pool pages table[b] names."""
    ps = pool.shape[2]
    for b, n in enumerate(held):
        for i in range(n):
            pool[table[b][i]] = slab[b, :, i * ps:(i + 1) * ps]


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_extend_attention_never_reads_invisible_rows(kind, paged):
    """NaN (codes 0xFF under NaN meta) in every row at or beyond lens[b] + Tq, in every page no sequence holds, and -1 in the
    table entries beyond a sequence's pages: the bits of the clean run, and finite."""
    hd, (nh, nkv), Tq, ps = 128, (8, 2), 40, 16
    lens, extra = LENS[2]
    L, scale = max(lens) + Tq + extra, 1.0 / math.sqrt(hd)
    q = _query(hd, nh, Tq)
    bufs, _, _ = _values(kind, hd, nkv)
    fills = (0xFF, 0xFF, NAN, NAN) if kind == "codes" else (NAN, NAN)
    if not paged:
        clean = _extend(kind, q, [_slab(t, L) for t in bufs], L, scale, lens)
        dirty = []
        for t, fill in zip(bufs, fills):
            s = _slab(t, L + 9, fill)
            for b, n in enumerate(lens):
                s[b, :, n + Tq:] = fill
            dirty.append(s)
        o = _extend(kind, q, dirty, L, scale, lens)
    else:
        mp = -(-L // ps)
        num_pages = 3 * mp + 3
        perm = _perm(num_pages, 9)
        full = [perm[b * mp:(b + 1) * mp] for b in range(3)]
        vals = [_slab(t, mp * ps) for t in bufs]
        clean = _extend(kind, q, _pool_of(vals, full, num_pages, ps), L, scale, lens, full)
        held = [-(-(n + Tq) // ps) for n in lens]
        table = [full[b][:held[b]] + [-1] * (mp - held[b]) for b in range(3)]
        pools = []
        for t, fill in zip(vals, fills):
            s = t.clone()
            for b, n in enumerate(lens):
                s[b, :, n + Tq:] = fill                              # the rest of the sequence's last page
            pool = torch.full((num_pages, nkv, ps, t.shape[3]), fill, dtype=t.dtype, device=DEV)
            _scatter_held(pool, table, s, held)
            pools.append(pool)
        o = _extend(kind, q, pools, L, scale, lens, table)
    assert bool(torch.isfinite(clean).all()) and bool(torch.isfinite(o).all())
    assert _same(o, clean), (kind, paged)


@pytest.mark.parametrize("kind", KINDS)
def test_extend_attention_clamps_the_lengths_the_host_cannot_see(kind):
    hd, (nh, nkv), Tq, L = 64, (8, 2), 17, 140
    scale = 1.0 / math.sqrt(hd)
    q = _query(hd, nh, Tq)
    bufs, _, _ = _values(kind, hd, nkv)
    fills = (0xFF, 0xFF, NAN, NAN) if kind == "codes" else (NAN, NAN)
    slabs = []
    for t, fill in zip(bufs, fills):
        s = _slab(t, L + 9, fill)
        s[:, :, L:] = fill                                           # nothing beyond row L may be read
        slabs.append(s)
    a = _extend(kind, q, slabs, L, scale, [-5, L + 7, 60])
    b = _extend(kind, q, slabs, L, scale, [0, L - Tq, 60])
    assert bool(torch.isfinite(a).all()) and _same(a, b)


@pytest.mark.parametrize("Tq", [17, 40])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_extend_attention_paged_equals_the_slab_bit_for_bit(kind, hd, Tq):
    nh, nkv = 8, 2
    lens, extra = LENS[2]
    L, scale = max(lens) + Tq + extra, 1.0 / math.sqrt(hd)
    q = _query(hd, nh, Tq)
    bufs, _, _ = _values(kind, hd, nkv)
    ref = _extend(kind, q, [_slab(t, L) for t in bufs], L, scale, lens)
    assert bool(torch.isfinite(ref).all())
    for ps in (16, 32, 128):
        mp = -(-L // ps)
        vals = [_slab(t, mp * ps) for t in bufs]
        for num_pages, seed in ((3 * mp + 1, 1), (6 * mp, 2)):
            perm = _perm(num_pages, seed + ps + Tq)
            table = [perm[b * mp:(b + 1) * mp] for b in range(3)]
            o = _extend(kind, q, _pool_of(vals, table, num_pages, ps), L, scale, lens, table)
            assert _same(o, ref), (kind, hd, Tq, ps, seed)


@pytest.mark.parametrize("kind", KINDS)
def test_extend_attention_is_bitwise_reproducible(kind):
    hd, (nh, nkv), Tq = 128, (8, 2), 40
    lens, extra = LENS[2]
    L, scale = max(lens) + Tq + extra, 1.0 / math.sqrt(hd)
    q = _query(hd, nh, Tq)
    slabs = [_slab(t, L) for t in _values(kind, hd, nkv)[0]]
    ws = torch.full((64 << 20,), 0xFF, dtype=torch.uint8, device=DEV)    # a caller's workspace, dirty
    a = _extend(kind, q, slabs, L, scale, lens)
    o = torch.empty_like(q)
    if kind == "codes":
        b = ops.extend_attention_codes(q, tuple(slabs), L, scale, _i32(lens), out=o, workspace=ws)
    else:
        b = ops.extend_attention(q, slabs[0], slabs[1], L, scale, _i32(lens), out=o, workspace=ws)
    assert b is o and _same(a, b)


def test_extend_attention_support_and_loud_errors():
    assert ops.extend_attention_supported(BF16, 32, 128) and ops.extend_attention_supported(BF16, 16, 64)
    assert not ops.extend_attention_supported(F32, 32, 128) and not ops.extend_attention_supported(BF16, 32, 96)
    hd, nh, nkv, Tq, L = 64, 4, 2, 16, 48
    scale = 1.0 / math.sqrt(hd)
    q = _query(hd, nh, Tq)
    bufs, _, _ = _values("bf16", hd, nkv)
    kc, vc = (_slab(t, L) for t in bufs)
    codes = [_slab(t, L) for t in _values("codes", hd, nkv)[0]]
    lens = _i32([0, 5, 32])
    with pytest.raises(OQError, match="lengths"):
        ops.extend_attention(q, kc, vc, L, scale, None)
    with pytest.raises(OQError, match="lengths"):
        ops.extend_attention_codes(q, codes, L, scale, None)
    for bad in (lens.cpu(), lens.long(), lens[:2]):
        with pytest.raises(OQError, match="lengths"):
            ops.extend_attention(q, kc, vc, L, scale, bad)
    with pytest.raises(OQError):                                     # fp32 q (and an fp32 cache): the decode kernel's
        ops.extend_attention(q.float(), kc.float(), vc.float(), L, scale, lens)
    with pytest.raises(OQError, match="bfloat16"):
        ops.extend_attention_codes(q.float(), codes, L, scale, lens)
    with pytest.raises(OQError, match="capacity"):                   # L beyond the capacity
        ops.extend_attention(q, kc, vc, L + 1, scale, lens)
    with pytest.raises(OQError, match="capacity"):
        ops.extend_attention_codes(q, codes, L + 1, scale, lens)
    table = torch.zeros(3, 3, dtype=torch.int32, device=DEV)
    pool = torch.zeros(4, nkv, 16, hd, dtype=BF16, device=DEV)
    for bad_k, bad_v in ((pool, pool[:, :, :, :32]), (pool[:, :, :8], pool[:, :, :8]), (pool.float(), pool.float())):
        with pytest.raises(OQError, match="pool"):                   # pools of the wrong shape, page size or dtype
            ops.extend_attention(q, bad_k, bad_v, L, scale, lens, page_table=table)
    with pytest.raises(OQError, match="page_table"):
        ops.extend_attention(q, pool, pool, L, scale, lens, page_table=table[:2])
    # the ABI refuses what it does not cover with its error code, before any launch
    from omniquant_amd import _capi as C
    lib = C.load()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    o = torch.empty_like(q)
    args = (3, Tq, nh, nkv, hd, L, C.ptr(lens), L, scale, C.ptr(ws), ws.numel(), C.stream())
    assert lib.oq_attn_extend(C.ptr(q), C.ptr(kc), C.ptr(vc), C.ptr(o), C.OQ_F32, *args) != 0
    assert "bf16" in lib.oq_last_error().decode()
    bad_hd = (3, Tq, nh, nkv, 96) + args[5:]
    assert lib.oq_attn_extend(C.ptr(q), C.ptr(kc), C.ptr(vc), C.ptr(o), C.OQ_BF16, *bad_hd) != 0
    assert lib.oq_attn_extend(C.ptr(q), C.ptr(kc), C.ptr(vc), C.ptr(o), C.OQ_BF16, *args) == 0


# ---------------------------------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------------------------------
EXT_BLOCKS = ("wo_llama_gqa", "wo_opt", "a4_gqa", "a4_gqa_codes", "a4_hd128_fused_codes")
CHUNK, CHUNK_TOKENS, TAIL = 32, [32, 20, 0], 2
NUM_PAGES, PS = 12, 16          # sum over the sequences of ceil((rows written) / 16) = 4 + 3 + 3 pages


class _Counter:
    """Counting wrappers around the two ops, installed with monkeypatch."""

    def __init__(self, monkeypatch):
        self.calls = 0
        for name in ("extend_attention", "extend_attention_codes"):
            monkeypatch.setattr(ops, name, self._wrap(getattr(ops, name)))

    def _wrap(self, fn):
        def counted(*a, **kw):
            self.calls += 1
            return fn(*a, **kw)
        return counted


def _cache(name, cd, paged, Tp):
    _, _, nh, nkv, code_bits, _ = RAGGED_BLOCKS[name]
    if paged:
        return PagedKVCache(3, nkv, RG.H // nh, cd, DEV, NUM_PAGES, page_size=PS, code_bits=code_bits)
    return PackedKVCache(3, nkv, RG.H // nh, cd, DEV, capacity=Tp, code_bits=code_bits, ragged=True)


def _prefill_chunk_decode(name, cd, paged, counter=None, chunk=CHUNK, tokens=CHUNK_TOKENS):
    """Right-padded prefill of PROMPTS, one `chunk`-row step with new_tokens = tokens, then TAIL single-token steps, none of them
    with a mask or positions.  Returns (block, family, cache, the sequences' inputs, each sequence's valid output rows)."""
    build, fam = RAGGED_BLOCKS[name][:2]
    blk = build()
    blk.compute_dtype = cd
    Tp = max(PROMPTS)
    seqs = [_x(1, n + chunk + TAIL + 8, 30 + i) for i, n in enumerate(PROMPTS)]
    X = _x(3, Tp, 29)                  # the pad rows hold some token's hidden state (a zero row has scale 0 on W4A4: NaN)
    for i, n in enumerate(PROMPTS):
        X[i, :n] = seqs[i][0, :n]
    cache = _cache(name, cd, paged, Tp)
    out = RG._step(blk, fam, X, cache, KD._causal(Tp).expand(3, 1, Tp, Tp), torch.arange(Tp, device=DEV)[None], new_tokens=PROMPTS)
    rows = [[out[i:i + 1, :n]] for i, n in enumerate(PROMPTS)]
    at = list(PROMPTS)
    assert counter is None or counter.calls == 0                     # the prefill has no past
    X = _x(3, chunk, 28)
    for i, n in enumerate(tokens):
        X[i, :n] = seqs[i][0, at[i]:at[i] + n]
    out = RG._step(blk, fam, X, cache, new_tokens=tokens)
    assert bool(torch.isfinite(out).all())                          # pad query rows: finite, unspecified
    assert cache.length == Tp + max(tokens)
    for i, n in enumerate(tokens):
        rows[i].append(out[i:i + 1, :n])
        at[i] += n
    called = None if counter is None else counter.calls
    for _ in range(TAIL):
        xs = torch.stack([seqs[i][0, at[i]] for i in range(3)])[:, None]
        o = RG._step(blk, fam, xs, cache)
        for i in range(3):
            rows[i].append(o[i:i + 1])
            at[i] += 1
    assert counter is None or counter.calls == called                # single-token steps stay on the decode kernel
    return blk, fam, cache, seqs, rows, at, called


@pytest.mark.parametrize("name", EXT_BLOCKS)
def test_blocks_route_long_steps_with_a_past_to_the_extend_kernel(name, monkeypatch):
    a4 = RAGGED_BLOCKS[name][5]
    counter = _Counter(monkeypatch)
    try:
        blk, fam, cache, seqs, rows, at, called = _prefill_chunk_decode(name, BF16, False, counter)
        assert called == 1                                           # once per block forward of the 32-row step
        assert at == [n + m + TAIL for n, m in zip(PROMPTS, CHUNK_TOKENS)]
        for i in range(3):
            x = seqs[i][:, :at[i]]
            RG._agree(torch.cat(rows[i], dim=1), RG._alone(blk, fam, x)[0], x, BF16, a4)
        counter.calls = 0
        _, _, paged, _, prows, pat, pcalled = _prefill_chunk_decode(name, BF16, True, counter)
        assert pcalled == 1 and pat == at
        for i in range(3):
            assert _same(torch.cat(prows[i], dim=1), torch.cat(rows[i], dim=1)), (name, i)
        assert cache.lengths.tolist() == at and paged.lengths.tolist() == at          # read once, at the end
    finally:
        RAGGED_BLOCKS[name][0]().compute_dtype = BF16


def test_forked_prefix_then_two_suffix_chunks(monkeypatch):
    counter = _Counter(monkeypatch)
    name = "wo_llama_gqa"
    build, fam, nh, nkv, _, a4 = RAGGED_BLOCKS[name]
    blk = build()
    n, m = 40, 32
    prefix, tails = _x(1, n, 61), [_x(1, m, 62), _x(1, m, 63)]
    cache = PagedKVCache(2, nkv, RG.H // nh, BF16, DEV, 8, page_size=PS)
    X = torch.cat([prefix, _x(1, n, 64)])
    RG._step(blk, fam, X, cache, KD._causal(n).expand(2, 1, n, n), torch.arange(n, device=DEV)[None], new_tokens=[n, 0])
    cache.fork(0, 1)
    full = n // PS
    assert counter.calls == 0
    out = RG._step(blk, fam, torch.cat(tails), cache)
    assert counter.calls == 1                                        # the 32-row step took the extend kernel
    assert cache.lengths.tolist() == [n + m, n + m]
    p0, p1 = cache.pages(0), cache.pages(1)
    assert p0[:full] == p1[:full] and all(cache.allocator.refcount(p) == 2 for p in p0[:full])
    assert not set(p0[full:]) & set(p1[full:])
    assert not _same(out[0], out[1])
    for i in range(2):
        x = torch.cat([prefix, tails[i]], dim=1)
        RG._agree(out[i:i + 1], RG._alone(blk, fam, x)[0][:, n:], x[:, n:], BF16, a4)


@pytest.mark.parametrize("why", ["float32", "OQ_NO_EXTEND", "Tq5"])
def test_fallbacks_stay_on_the_decode_kernel(why, monkeypatch):
    name = "wo_llama_gqa"
    cd = F32 if why == "float32" else BF16
    chunk, tokens = (5, [5, 3, 0]) if why == "Tq5" else (CHUNK, CHUNK_TOKENS)
    try:
        # today's path: the routing cannot reach the new ops at all
        monkeypatch.setattr(block_common, "EXTEND_MIN_TQ", 1 << 30)
        ref = _prefill_chunk_decode(name, cd, False, chunk=chunk, tokens=tokens)[4]
        monkeypatch.undo()
        counter = _Counter(monkeypatch)
        if why == "OQ_NO_EXTEND":
            monkeypatch.setenv("OQ_NO_EXTEND", "1")
        rows = _prefill_chunk_decode(name, cd, False, counter, chunk=chunk, tokens=tokens)[4]
        assert counter.calls == 0
        for i in range(3):
            assert _same(torch.cat(rows[i], dim=1), torch.cat(ref[i], dim=1)), (why, i)
    finally:
        RAGGED_BLOCKS[name][0]().compute_dtype = BF16


def test_a_mask_with_a_long_step_stays_a_loud_error():
    blk = RAGGED_BLOCKS["wo_llama_gqa"][0]()
    T = 16
    cache = PackedKVCache(3, 2, 64, BF16, DEV, capacity=64, ragged=True)
    RG._step(blk, "llama", _x(3, T, 3), cache, KD._causal(T).expand(3, 1, T, T), torch.arange(T, device=DEV)[None], new_tokens=[16, 8, 4])
    with pytest.raises(OQError, match="takes no attention_mask"):
        RG._step(blk, "llama", _x(3, CHUNK, 4), cache, KD._causal(CHUNK, T))
    assert cache.length == T and cache.lengths.tolist() == [16, 8, 4]
