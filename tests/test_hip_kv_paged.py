"""Paged KV cache: the paged appends and decode attentions of csrc/oq_decode.hip (page pools found through a page table, in
the place of the [bs, nkv, cap, ...] slab), kvcache.PagedKVCache and the block forwards on it.  The references are the ragged
contiguous entry points and PackedKVCache(ragged=True) -- bit for bit, for every page size and page order, because the paged
kernels run the same loops and sums on the same row values -- and, to anchor that to something else, the float64 softmax and
each sequence run alone, with the bounds the ragged tests assert."""
import math

import pytest
import torch

import test_hip_kv_decode as KD
import test_hip_kv_ragged as RG
from omniquant_amd import OQError, ops
from omniquant_amd.kvcache import PackedKVCache, PagedKVCache, unpack_codes
from test_hip_kv_codes import _bound as _code_bound
from test_hip_kv_codes import _same_nan
from test_hip_kv_ragged import APPENDS, PROMPTS, RAGGED_BLOCKS, STEPS, _append, _buffers, _i32, _ragged_ref64, _rows, _same, _x

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
UNIT = KD.UNIT
NAN = float("nan")


def _perm(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()


def _gather(pool, row):
    """The slab [nkv, len(row) * PS, x] of a sequence whose table row is `row` (a list of page ids)."""
    t = pool[torch.tensor(row, device=DEV)]
    return t.transpose(0, 1).reshape(pool.shape[1], -1, pool.shape[3])


def _scatter(pool, table, slab):
    """Write the contiguous [bs, nkv, mp * PS, x] slab into the pages table [bs, mp] (lists) names."""
    bs, nkv, _, x = slab.shape
    ps, mp = pool.shape[2], len(table[0])
    idx = torch.tensor(table, device=DEV).flatten()
    pool[idx] = slab.reshape(bs, nkv, mp, ps, x).permute(0, 2, 1, 3, 4).reshape(bs * mp, nkv, ps, x)


def _append_paged(kind, q, k, v, pools, table, dout, cos, sin, positions, lens):
    qo = torch.empty(q.shape, dtype=dout, device=DEV)
    ko = torch.empty(k.shape, dtype=dout, device=DEV)
    vo = None if kind == "plain" else torch.empty(v.shape, dtype=dout, device=DEV)
    kw = dict(q=q, q_out=qo, k_out=ko, cos=cos, sin=sin, positions=positions, lengths=_i32(lens),
              page_table=torch.tensor(table, dtype=torch.int32, device=DEV))
    if kind == "plain":
        ops.kv_append(k, v, pools[0], pools[1], 0, **kw)
    elif kind == "quant":
        ops.kv_append_quant(k, v, 4, dout, k_cache=pools[0], v_cache=pools[1], v_out=vo, **kw)
    else:
        ops.kv_append_codes(k, v, dout, *pools, v_out=vo, **kw)
    return qo, ko, vo


# ---------------------------------------------------------------------------------------------------------------------
# 1. append: the bytes of the ragged contiguous append, found through the table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [16, 128])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kind,din,dout", APPENDS)
def test_paged_append_equals_the_ragged_append(kind, din, dout, hd, ps):
    bs, Tq, nkv = 3, 4, 2
    q, k, v, cos, sin = RG._step_inputs(hd, din)
    explicit = torch.stack([torch.arange(Tq) + 3, torch.arange(Tq) * 7 + 2, torch.arange(Tq) + 40]).to(DEV)
    for lens in ([0, 5, 17], [0, 14, 30])[:2 if ps == 16 else 1]:         # [0, 14, 30]: the steps straddle a page boundary
        mp = -(-(max(lens) + Tq) // ps)
        num_pages = bs * mp + 2
        perm = _perm(num_pages, hd + ps + lens[1])
        table, unused = [perm[b * mp:(b + 1) * mp] for b in range(bs)], perm[bs * mp:]
        for pos in (None, explicit):
            ref = _buffers(kind, bs, nkv, mp * ps, hd, dout)
            ref_outs = _append(kind, q, k, v, ref, dout, cos, sin, pos, lengths=_i32(lens))
            pools = _buffers(kind, num_pages, nkv, ps, hd, dout)
            outs = _append_paged(kind, q, k, v, pools, table, dout, cos, sin, pos, lens)
            for b in range(bs):
                # each sequence's pages in table order: its rows and every sentinel around them
                assert all(_same_nan(_gather(p, table[b]), r[b]) for p, r in zip(pools, ref)), (kind, b, lens)
            assert all(_same_nan(o, r) for o, r in zip(outs, ref_outs) if o is not None), kind
            for p, fresh in zip(pools, _buffers(kind, num_pages, nkv, ps, hd, dout)):
                assert _same(p[unused], fresh[unused])                         # pages in no table row are untouched
                assert not _same(p, fresh)


# ---------------------------------------------------------------------------------------------------------------------
# 2. append guards: rows beyond the table's reach, table entries outside the pool
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kind,din,dout", APPENDS)
def test_paged_append_guards_rows_and_table_entries(kind, din, dout, hd):
    """The pools are the middle of a larger sentinel allocation with one extra page on each side, so that an entry of -1 or
    num_pages, were it followed, would still land inside memory the test owns (and be seen).  Sequence 0: the second page it
    would write has entry -1; sequence 1: the first has entry num_pages; sequence 2: rows at and beyond max_pages * PS
    (never the last sequence: a missing range guard would read the table row after its own); sequence 3: a negative
    length, whose step row 3 lands at row 0 and is stored like any other."""
    bs, Tq, nkv, ps, mp, P = 4, 4, 2, 16, 2, 64
    num_pages = 8
    lens = [14, 14, 30, -3]
    table = [[5, -1], [num_pages, 2], [7, 0], [3, 6]]
    g = torch.Generator(device=DEV).manual_seed(hd)
    q = (torch.randn(bs, Tq, 4, hd, generator=g, device=DEV) * 3).to(din)
    k = torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV).to(din)
    v = (torch.randn(bs, Tq, nkv, hd, generator=g, device=DEV) + 2).to(din)
    _, _, _, cos, sin = RG._step_inputs(hd, din)
    big = _buffers(kind, num_pages, nkv, ps, hd, dout, lead=1)
    expect = [t.clone() for t in big]
    outs = _append_paged(kind, q, k, v, [t[1:1 + num_pages] for t in big], table, dout, cos, sin, None, lens)
    # the rows that fit, as (sequence, step rows, logical row of the first, page): each equals the uniform append of those
    # step rows alone
    for b, rows, past, page in ((0, slice(0, 2), 14, 5), (1, slice(2, 4), 16, 2), (2, slice(0, 2), 30, 0), (3, slice(3, 4), 0, 3)):
        ref = _buffers(kind, 1, nkv, mp * ps, hd, dout)
        n = rows.stop - rows.start
        _append(kind, q[b:b + 1, rows], k[b:b + 1, rows], v[b:b + 1, rows], ref, dout, cos, sin, None, past=past)
        for e, r in zip(expect, ref):
            e[1 + page, :, past % ps:past % ps + n] = r[0, :, past:past + n]
    assert all(_same_nan(t, e) for t, e in zip(big, expect)), kind       # nothing else, lead pages included
    pos = torch.stack([(torch.arange(Tq) + n).clamp(0, P - 1) for n in lens]).to(DEV)
    ref_outs = _append(kind, q, k, v, _buffers(kind, bs, nkv, mp * ps, hd, dout), dout, cos, sin, pos, past=0)
    assert all(_same_nan(o, r) for o, r in zip(outs, ref_outs) if o is not None), kind


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
NROWS = 2047 + 4
LENS = ([0, 130, 300], [0, 130, 2047])
_REF = {}


def _values(cache, hd, nkv, cd):
    """The row values of a cache kind as contiguous buffers [3, nkv, NROWS, ...] (floats in cd, or the four code buffers)."""
    kf, vf, codes = _rows(hd, 3, nkv, NROWS)
    return list(codes) if cache == "codes" else [kf.to(cd), vf.to(cd)]


def _slab(t, rows, fill=0):
    """The first `rows` rows of t [bs, nkv, n, x], padded with `fill` where rows > n."""
    out = torch.full((t.shape[0], t.shape[1], rows, t.shape[3]), fill, dtype=t.dtype, device=DEV)
    n = min(rows, t.shape[2])
    out[:, :, :n] = t[:, :, :n]
    return out


def _attend(cache, q, bufs, L, scale, lens, table=None):
    kw = dict(lengths=_i32(lens))
    if table is not None:
        kw["page_table"] = torch.tensor(table, dtype=torch.int32, device=DEV)
    if cache == "codes":
        return ops.decode_attention_codes(q, tuple(bufs), L, scale, **kw)
    return ops.decode_attention(q, bufs[0], bufs[1], L, scale, **kw)


def _query(cache, hd, nh, Tq):
    cd = F32 if cache == "f32" else BF16
    g = torch.Generator(device=DEV).manual_seed(nh + Tq)
    return torch.randn(3, Tq, nh, hd, generator=g, device=DEV).to(cd), cd


def _ragged_out(cache, hd, heads, Tq, li):
    """The ragged contiguous kernel's output for a case (computed once, left alone), with its inputs."""
    key = (cache, hd, heads, Tq, li)
    if key not in _REF:
        nh, nkv = heads
        q, cd = _query(cache, hd, nh, Tq)
        L = max(LENS[li]) + Tq
        bufs = [_slab(t, L) for t in _values(cache, hd, nkv, cd)]
        o = _attend(cache, q, bufs, L, 1.0 / math.sqrt(hd), LENS[li])
        assert bool(torch.isfinite(o).all())
        _REF[key] = o
    return _REF[key]


def _pool_of(vals, table, num_pages, ps, fills=None, lead=0):
    """Pools [lead + num_pages + lead, nkv, ps, x] filled with `fills` holding the slabs `vals` in the pages of `table`;
    returns the views of the middle num_pages pages."""
    pools = []
    for i, t in enumerate(vals):
        big = torch.full((num_pages + 2 * lead, t.shape[1], ps, t.shape[3]), 0 if fills is None else fills[i], dtype=t.dtype,
                         device=DEV)
        p = big[lead:lead + num_pages]
        _scatter(p, table, t)
        pools.append(p)
    return pools


@pytest.mark.parametrize("heads", [(8, 2), (4, 4)])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("cache", ["bf16", "f32", "codes"])
def test_paged_attention_is_the_ragged_kernel_bit_for_bit(cache, hd, heads):
    nh, nkv = heads
    scale = 1.0 / math.sqrt(hd)
    for Tq in (1, 4):
        q, cd = _query(cache, hd, nh, Tq)
        for li, lens in enumerate(LENS):
            L = max(lens) + Tq                                  # several splits whose boundaries fall inside pages
            ref = _ragged_out(cache, hd, heads, Tq, li)
            for ps in (16, 128):
                mp = -(-L // ps)
                vals = [_slab(t, mp * ps) for t in _values(cache, hd, nkv, cd)]
                outs = []
                for num_pages, seed in ((3 * mp + 1, 1), (6 * mp, 2)):      # and a pool twice the size, another permutation
                    perm = _perm(num_pages, seed + ps + Tq)
                    table = [perm[b * mp:(b + 1) * mp] for b in range(3)]
                    pools = _pool_of(vals, table, num_pages, ps)
                    outs += [_attend(cache, q, pools, L, scale, lens, table) for _ in range(2)]
                assert all(_same(o, ref) for o in outs), (cache, hd, heads, Tq, lens, ps)


@pytest.mark.parametrize("ps", [16, 128])
@pytest.mark.parametrize("Tq", [1, 4])
@pytest.mark.parametrize("cache", ["bf16", "f32", "codes"])
def test_paged_attention_never_reads_invisible_rows(cache, Tq, ps):
    """NaN (0xFF codes under NaN meta) in every pool row no query may see: the rest of each sequence's last page, every page in
    no table, and the poison page that all unused table entries name."""
    hd, heads = 128, (8, 2)
    nh, nkv = heads
    scale = 1.0 / math.sqrt(hd)
    q, cd = _query(cache, hd, nh, Tq)
    fills = (0xFF, 0xFF, NAN, NAN) if cache == "codes" else (NAN, NAN)
    for li, lens in enumerate(LENS):
        L = max(lens) + Tq
        mp = -(-L // ps)
        num_pages = 3 * mp + 3
        perm = _perm(num_pages, 5 + ps + Tq)
        poison = perm[-1]
        table, vals = [], []
        for b, n in enumerate(lens):
            used = -(-(n + Tq) // ps)
            table.append(perm[b * mp:b * mp + used] + [poison] * (mp - used))
        for t, fill in zip(_values(cache, hd, nkv, cd), fills):
            s = _slab(t, mp * ps, fill)
            for b, n in enumerate(lens):
                s[b, :, n + Tq:] = fill
            vals.append(s)
        pools = _pool_of(vals, table, num_pages, ps, fills)
        for p, fill in zip(pools, fills):
            p[poison] = fill                                     # (the scatter wrote the slabs' fill rows there: the same)
        o = _attend(cache, q, pools, L, scale, lens, table)
        assert o.dtype == cd and bool(torch.isfinite(o).all())
        assert _same(o, _ragged_out(cache, hd, heads, Tq, li)), (cache, Tq, ps, lens)
        kf, vf, codes = _rows(hd, 3, nkv, NROWS)
        if cache == "codes":
            ref, _ = _ragged_ref64(q, unpack_codes(codes[0], codes[2]), unpack_codes(codes[1], codes[3]), lens, scale)
            err, top = float((o.double() - ref).abs().max()), float(ref.abs().max())
            print(f"paged codes {cd} Tq {Tq} PS {ps} lens {lens}: max err {err:.3e} of max|ref| {top:.3e}")
            assert err <= _code_bound(cd, top), (err, top)
        else:
            ref, mag = _ragged_ref64(q, kf.to(cd).float(), vf.to(cd).float(), lens, scale)
            err = (o.double() - ref).abs()
            bound = UNIT[cd] * ref.abs() + 2e-5 * mag
            print(f"paged float {cd} Tq {Tq} PS {ps} lens {lens}: max (err - bound) {float((err - bound).max()):.3e}")
            assert bool((err <= bound).all()), float((err - bound).max())


def _ref64_kept(q, kf, vf, n, scale, keep):
    """float64 softmax of one sequence: query row t over the rows j <= n + t with keep[j]; (o, sum p |v|) [Tq, nh, hd]."""
    Tq, nh, hd = q.shape
    rep = nh // kf.shape[0]
    o = torch.empty(q.shape, dtype=torch.float64, device=DEV)
    mag = torch.empty_like(o)
    for t in range(Tq):
        idx = torch.nonzero(keep[:n + t + 1]).flatten()
        k = kf[:, idx].double().repeat_interleave(rep, dim=0)
        v = vf[:, idx].double().repeat_interleave(rep, dim=0)
        p = torch.softmax(torch.einsum("hd,hjd->hj", q[t].double(), k) * scale, dim=-1)
        o[t] = torch.einsum("hj,hjd->hd", p, v)
        mag[t] = torch.einsum("hj,hjd->hd", p, v.abs())
    return o, mag


@pytest.mark.parametrize("cache", ["f32", "codes"])
def test_paged_attention_guards_table_entries_and_clamps_lengths(cache):
    hd, nh, nkv, Tq, ps = 64, 8, 2, 2, 16
    scale = 1.0 / math.sqrt(hd)
    lens = [40, 130, 300]
    L = max(lens) + Tq
    mp = -(-L // ps)
    num_pages = 3 * mp
    q, cd = _query(cache, hd, nh, Tq)
    fills = (0xFF, 0xFF, NAN, NAN) if cache == "codes" else (NAN, NAN)
    vals = [_slab(t, mp * ps) for t in _values(cache, hd, nkv, cd)]
    perm = _perm(num_pages, 11)
    table = [perm[b * mp:(b + 1) * mp] for b in range(3)]
    pools = _pool_of(vals, table, num_pages, ps, fills, lead=1)            # one NaN page before and one behind the pool
    good = _attend(cache, q, pools, L, scale, lens, table)
    contiguous = _attend(cache, q, [_slab(t, L) for t in _values(cache, hd, nkv, cd)], L, scale, lens)
    assert _same(good, contiguous)
    # entries -1 and num_pages at visible positions of sequence 1: rows [32, 48) and [80, 96) are invisible
    bad = [list(r) for r in table]
    bad[1][2], bad[1][5] = -1, num_pages
    o = _attend(cache, q, pools, L, scale, lens, bad)
    assert bool(torch.isfinite(o).all())                                    # nothing from the lead pages
    assert _same(o[0], good[0]) and _same(o[2], good[2]) and not _same(o[1], good[1])
    keep = torch.ones(mp * ps, dtype=torch.bool, device=DEV)
    keep[32:48] = False
    keep[80:96] = False
    kf, vf, codes = _rows(hd, 3, nkv, NROWS)
    if cache == "codes":
        kf, vf = unpack_codes(codes[0], codes[2]), unpack_codes(codes[1], codes[3])
    ref, mag = _ref64_kept(q[1], kf[1], vf[1], lens[1], scale, keep)
    err = (o[1].double() - ref).abs()
    if cache == "codes":
        assert float(err.max()) <= _code_bound(cd, float(ref.abs().max())), float(err.max())
    else:
        assert bool((err <= UNIT[cd] * ref.abs() + 2e-5 * mag).all()), float(err.max())
    # lengths the host cannot see: negative counts as 0, beyond L - Tq as L - Tq
    wild, clamped = [-5, L + 7, 60], [0, L - Tq, 60]
    a, b = _attend(cache, q, pools, L, scale, wild, table), _attend(cache, q, pools, L, scale, clamped, table)
    c = _attend(cache, q, [_slab(t, L) for t in _values(cache, hd, nkv, cd)], L, scale, clamped)
    assert bool(torch.isfinite(a).all()) and _same(a, b) and _same(a, c)


# ---------------------------------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------------------------------
NUM_PAGES, PS = 6, 16           # 96 rows for the three sequences together: sum(ceil((n + STEPS) / 16)) = 2 + 2 + 1 pages
_RUNS = {}


def _prefill_and_decode(name, cd, paged):
    """test_hip_kv_ragged._prefill_and_decode on a PagedKVCache or on its PackedKVCache(ragged=True) sibling: right-padded
    prefill of PROMPTS with new_tokens, then STEPS mask-free single-token steps."""
    build, fam, nh, nkv, code_bits, a4 = RAGGED_BLOCKS[name]
    blk = build()
    blk.compute_dtype = cd
    Tp = max(PROMPTS)
    seqs = [_x(1, n + STEPS + 8, 30 + i) for i, n in enumerate(PROMPTS)]
    X = _x(3, Tp, 29)                  # the pad rows hold some token's hidden state (a zero row has scale 0 on W4A4: NaN)
    for i, n in enumerate(PROMPTS):
        X[i, :n] = seqs[i][0, :n]
    if paged:
        cache = PagedKVCache(3, nkv, RG.H // nh, cd, DEV, NUM_PAGES, page_size=PS, code_bits=code_bits)
    else:
        cache = PackedKVCache(3, nkv, RG.H // nh, cd, DEV, capacity=Tp, code_bits=code_bits, ragged=True)
    out = RG._step(blk, fam, X, cache, KD._causal(Tp).expand(3, 1, Tp, Tp), torch.arange(Tp, device=DEV)[None], new_tokens=PROMPTS)
    assert cache.length == Tp
    rows = [[out[i:i + 1, :n]] for i, n in enumerate(PROMPTS)]
    for s in range(STEPS):
        xs = torch.stack([seqs[i][0, n + s] for i, n in enumerate(PROMPTS)])[:, None]
        o = RG._step(blk, fam, xs, cache)
        assert cache.length == Tp + s + 1
        for i in range(3):
            rows[i].append(o[i:i + 1])
    return blk, fam, cache, seqs, rows


@pytest.mark.parametrize("cd", [BF16, F32])
@pytest.mark.parametrize("name", list(RAGGED_BLOCKS))
def test_blocks_on_a_paged_cache_equal_the_ragged_cache_bit_for_bit(name, cd):
    a4 = RAGGED_BLOCKS[name][5]
    try:
        blk, fam, cache, seqs, rows = _prefill_and_decode(name, cd, True)
        _, _, sibling, _, ref_rows = _prefill_and_decode(name, cd, False)
        assert "paged" in repr(cache) and f"of {NUM_PAGES} pages free" in repr(cache)
        assert cache.paged and cache.ragged and cache.capacity == NUM_PAGES * PS
        assert [len(cache.pages(i)) for i in range(3)] == [-(-(n + STEPS) // PS) for n in PROMPTS]
        for i, n in enumerate(PROMPTS):
            assert _same(torch.cat(rows[i], dim=1), torch.cat(ref_rows[i], dim=1)), (name, i)
            (k, v), (rk, rv) = cache.sequence(i), sibling.sequence(i)
            assert k.shape == (cache.nkv, n + STEPS, cache.hd) and k.dtype == cd
            assert _same_nan(k, rk) and _same_nan(v, rv), (name, i)
        if name == "wo_llama_gqa":
            # anchored to something other than the sibling cache: each sequence alone, the ragged tests' bounds
            for i, n in enumerate(PROMPTS):
                x = seqs[i][:, :n + STEPS]
                RG._agree(torch.cat(rows[i], dim=1), RG._alone(blk, fam, x, use_cache=True)[0], x, cd, a4)
    finally:
        RAGGED_BLOCKS[name][0]().compute_dtype = BF16


def _no_sync_steps(blk, fam, cache, xs_list):
    """Decode steps under the sync debug mode: any device-to-host read raises."""
    outs = []
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for xs in xs_list:
            outs.append(RG._step(blk, fam, xs, cache))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    return outs


def test_slot_reuse_fork_and_exhaustion():
    name, cd = "wo_llama_gqa", F32
    blk, fam, cache, seqs, rows = _prefill_and_decode(name, cd, True)
    alloc = cache.allocator
    try:
        # ---- slot reuse: slot 1's pages return to the pool, a fresh 5-token prompt starts there
        n0, n2 = PROMPTS[0] + STEPS, PROMPTS[2] + STEPS
        free, mine = cache.n_free, len(cache.pages(1))
        assert mine == 2
        cache.set_lengths([n0, 0, n2])
        assert cache.n_free == free + mine and cache.pages(1) == [] and cache.length == n0
        fresh = _x(1, 8, 55)
        seqs[1], rows[1] = fresh, []
        at = [n0, 0, n2]
        X = _x(3, 5, 56)
        X[0, 0], X[1, :5], X[2, 0] = seqs[0][0, at[0]], fresh[0, :5], seqs[2][0, at[2]]
        o = RG._step(blk, fam, X, cache, new_tokens=[1, 5, 1])
        assert cache.length == n0 + 5
        for i, n in enumerate([1, 5, 1]):
            rows[i].append(o[i:i + 1, :n])
            at[i] += n
        steps = []
        for s in range(2):
            steps.append(torch.stack([seqs[i][0, at[i] + s] for i in range(3)])[:, None])
        for o in _no_sync_steps(blk, fam, cache, steps):
            for i in range(3):
                rows[i].append(o[i:i + 1])
                at[i] += 1
        assert at == [n0 + 3, 7, n2 + 3]
        for i in range(3):
            KD._agree(torch.cat(rows[i], dim=1), RG._alone(blk, fam, seqs[i][:, :at[i]])[0], cd)
        assert cache.lengths.tolist() == at
        assert [len(cache.pages(i)) for i in range(3)] == [-(-n // PS) for n in at]

        # ---- fork: slot 1 becomes a copy of slot 0; full pages shared, the partial page private
        cache.set_lengths([at[0], 0, at[2]])
        cache.fork(0, 1)
        at[1] = at[0]
        full = at[0] // PS
        p0, p1 = cache.pages(0), cache.pages(1)
        assert at[0] % PS and len(p0) == len(p1) == full + 1
        assert p0[:full] == p1[:full] and all(alloc.refcount(p) == 2 for p in p0[:full])
        assert p0[full] != p1[full] and alloc.refcount(p0[full]) == alloc.refcount(p1[full]) == 1
        assert cache.page_table[:2, :full + 1].tolist() == [p0, p1] and cache.lengths.tolist() == at
        assert all(_same(a, b) for a, b in zip(cache.sequence(0), cache.sequence(1)))
        same = []
        for s in range(2):
            tok = seqs[0][0, at[0] + s]
            same.append(torch.stack([tok, tok, seqs[2][0, at[2] + s]])[:, None])
        for o in _no_sync_steps(blk, fam, cache, same):
            assert _same(o[0], o[1])
            at = [n + 1 for n in at]
        before = [cache.sequence(i) for i in range(2)]
        other = torch.stack([seqs[0][0, at[0]], fresh[0, 0], seqs[2][0, at[2]]])[:, None]
        (o,) = _no_sync_steps(blk, fam, cache, [other])
        at = [n + 1 for n in at]
        assert not _same(o[0], o[1])
        for i in range(2):
            k, v = cache.sequence(i)
            assert k.shape[1] == at[i] and _same(k[:, :-1], before[i][0]) and _same(v[:, :-1], before[i][1])
        assert not _same(cache.sequence(0)[0][:, -1], cache.sequence(1)[0][:, -1])
        assert cache.pages(0)[:full] == cache.pages(1)[:full]

        # ---- exhaustion: refused before any launch, the cache unchanged, and the next legal step still works
        state = (cache.length, cache.lengths.tolist(), cache.page_table.tolist(), cache.n_free)
        assert cache.n_free == 0
        with pytest.raises(OQError, match="pages"):
            cache.reserve(PS)
        with pytest.raises(OQError, match="pages"):
            RG._step(blk, fam, _x(3, PS, 57), cache)
        with pytest.raises(OQError, match="max_pages"):
            cache.reserve(NUM_PAGES * PS)
        assert (cache.length, cache.lengths.tolist(), cache.page_table.tolist(), cache.n_free) == state
        xs = torch.stack([seqs[0][0, at[0]], fresh[0, 1], seqs[2][0, at[2]]])[:, None]
        (o,) = _no_sync_steps(blk, fam, cache, [xs])
        assert bool(torch.isfinite(o).all()) and cache.lengths.tolist() == [n + 1 for n in at]
        c2 = cache.clone()
        assert c2.pages(0) == cache.pages(0) and c2.n_free == cache.n_free and _same(c2.sequence(2)[0], cache.sequence(2)[0])
        for surface in (lambda: cache[0], lambda: list(cache), lambda: cache.to_tuple(), lambda: cache.dequantize()):
            with pytest.raises(OQError, match="ragged"):
                surface()
        with pytest.raises(OQError, match="not empty"):
            cache.fork(0, 2)
    finally:
        blk.compute_dtype = BF16
    torch.cuda.synchronize()
