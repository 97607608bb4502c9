"""Tree attention for speculative decoding (csrc/oq_extend.hip, the TREE form; csrc/oq_kvpool.hip, kv_tree_commit_kernel): the
masked kernel against a float64 softmax under the tree's mask, a chain against the causal kernel bit for bit, paged == slab,
the rows it must never read, the row compaction that commits an accepted path, and the block forwards with tree= followed by
cache.commit_tree against the ordinary linear step of the accepted tokens."""
import math

import pytest
import torch

import test_hip_kv_extend as EX
import test_hip_kv_ragged as RG
from omniquant_amd import OQError, ops
from omniquant_amd.kvcache import PackedKVCache, PagedKVCache, PagedKVPool, TokenTree, unpack_codes
from test_hip_kv_paged import UNIT, _perm, _pool_of, _slab
from test_hip_kv_ragged import PROMPTS, RAGGED_BLOCKS, _i32, _rows, _same, _x

KD = RG.KD
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
LENS, NROWS = EX.LENS, EX.NROWS
KINDS = ("bf16", "codes", "codes8")
_V8 = {}


def _values(kind, hd, nkv):
    """test_hip_kv_extend._values plus the 8-bit code kind: (contiguous buffers [3, nkv, NROWS, ...], float32 K, float32 V)."""
    if kind != "codes8":
        return EX._values(kind, hd, nkv)
    if (hd, nkv) not in _V8:
        kf, vf, _ = _rows(hd, 3, nkv, NROWS)
        kc = torch.empty(3, nkv, NROWS, hd, dtype=torch.uint8, device=DEV)
        km = torch.empty(3, nkv, NROWS, 2, dtype=F32, device=DEV)
        bufs = [kc, kc.clone(), km, km.clone()]
        ops.kv_append_codes(kf.transpose(1, 2).contiguous(), vf.transpose(1, 2).contiguous(), F32, *bufs, past=0)
        _V8[(hd, nkv)] = (bufs, unpack_codes(bufs[0], bufs[2], bits=8), unpack_codes(bufs[1], bufs[3], bits=8))
    return _V8[(hd, nkv)]


def _fills(kind):
    return (NAN, NAN) if kind == "bf16" else (0xFF, 0xFF, NAN, NAN)


def _branching(Tq):
    """Node 0 a root with three children, every later node t a child of (t - 1) // 3: siblings at every level."""
    return TokenTree([-1] + [(t - 1) // 3 for t in range(1, Tq)])


def _forest(Tq):
    """Two roots (0 and 1), node t >= 2 a child of (t - 2) // 2."""
    return TokenTree([-1, -1][:Tq] + [(t - 2) // 2 for t in range(2, Tq)])


def _tree_attn(q, bufs, L, scale, lens, tree, table=None, **kw):
    if table is not None:
        kw["page_table"] = torch.tensor(table, dtype=torch.int32, device=DEV)
    return ops.tree_attention(q, tuple(bufs), L, scale, _i32(lens), tree, **kw)


def _tree_ref64(q, kf, vf, lens, scale, tree):
    """test_hip_kv_ragged._ragged_ref64 with the tree's mask: node t of sequence b attends rows [0, lens[b]) and rows
    lens[b] + u for u on the root path of t.  Returns (o, sum_j p_j |v_j|), each [bs, Tq, nh, hd] float64."""
    bs, Tq, nh, hd = q.shape
    rep = nh // kf.shape[1]
    o = torch.empty(q.shape, dtype=torch.float64, device=q.device)
    mag = torch.empty_like(o)
    for b, n in enumerate(lens):
        for t in range(Tq):
            rows = torch.tensor(list(range(n)) + [n + u for u in tree.path(t, b)], device=q.device)
            k = kf[b][:, rows].double().repeat_interleave(rep, dim=0)
            v = vf[b][:, rows].double().repeat_interleave(rep, dim=0)
            p = torch.softmax(torch.einsum("hd,hjd->hj", q[b, t].double(), k) * scale, dim=-1)
            o[b, t] = torch.einsum("hj,hjd->hd", p, v)
            mag[b, t] = torch.einsum("hj,hjd->hd", p, v.abs())
    return o, mag


# ---------------------------------------------------------------------------------------------------------------------
# 1. float64 reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tq", [5, 33, 64])
@pytest.mark.parametrize("heads", [(4, 4), (8, 2)])
@pytest.mark.parametrize("hd", [64, 128])
def test_tree_attention_matches_float64(hd, heads, Tq):
    """The bound test_extend_attention_matches_float64 derives, |o - ref| <= UNIT[bf16] |ref| + (2^-8 + 2e-5) mag, against that
    test's float64 softmax with the tree's mask applied; one tree for the batch, and once a different tree per sequence."""
    nh, nkv = heads
    scale = 1.0 / math.sqrt(hd)
    q = EX._query(hd, nh, Tq)
    shared = _branching(Tq)
    chain = [-1] + list(range(Tq - 1))
    per_seq = TokenTree([shared.parents, _forest(Tq).parents, chain])
    for kind in KINDS:
        bufs, kf, vf = _values(kind, hd, nkv)
        for li, (lens, extra) in enumerate(LENS):
            L = max(lens) + Tq + extra
            slabs = [_slab(t, L) for t in bufs]
            for tree in (shared, per_seq)[:2 if li == 1 else 1]:
                o = _tree_attn(q, slabs, L, scale, lens, tree)
                ref, mag = _tree_ref64(q, kf, vf, lens, scale, tree)
                err = (o.double() - ref).abs()
                bound = UNIT[BF16] * ref.abs() + (2.0 ** -8 + 2e-5) * mag
                print(f"tree {kind} hd {hd} heads {heads} Tq {Tq} lens {lens} {tree!r}: max err {float(err.max()):.3e}, "
                      f"max (err - bound) {float((err - bound).max()):.3e}")
                assert o.dtype == BF16 and bool(torch.isfinite(o).all())
                assert bool((err <= bound).all()), (kind, lens, float((err - bound).max()))


# ---------------------------------------------------------------------------------------------------------------------
# 2. a chain is the causal kernel, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _causal(kind, q, bufs, L, scale, lens, table=None):
    kw = {} if table is None else {"page_table": torch.tensor(table, dtype=torch.int32, device=DEV)}
    if kind == "bf16":
        return ops.extend_attention(q, bufs[0], bufs[1], L, scale, _i32(lens), **kw)
    return ops.extend_attention_codes(q, tuple(bufs), L, scale, _i32(lens), **kw)


@pytest.mark.parametrize("Tq", [16, 40, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_a_chain_is_the_causal_extend_kernel_bit_for_bit(kind, Tq):
    chain = TokenTree([-1] + list(range(Tq - 1)))
    for hd, (nh, nkv), li, ps in ((128, (8, 2), 2, 16), (64, (4, 4), 1, 32)):
        lens, extra = LENS[li]
        L, scale = max(lens) + Tq + extra, 1.0 / math.sqrt(hd)
        q = EX._query(hd, nh, Tq)
        bufs, _, _ = _values(kind, hd, nkv)
        slabs = [_slab(t, L) for t in bufs]
        ref = _causal(kind, q, slabs, L, scale, lens)
        assert bool(torch.isfinite(ref).all())
        assert _same(_tree_attn(q, slabs, L, scale, lens, chain), ref), (kind, Tq, hd, "slab")
        mp = -(-L // ps)
        num_pages = 3 * mp + 2
        perm = _perm(num_pages, Tq + hd)
        table = [perm[b * mp:(b + 1) * mp] for b in range(3)]
        pools = _pool_of([_slab(t, mp * ps) for t in bufs], table, num_pages, ps)
        assert _same(_causal(kind, q, pools, L, scale, lens, table), ref)
        assert _same(_tree_attn(q, pools, L, scale, lens, chain, table), ref), (kind, Tq, hd, "paged")


# ---------------------------------------------------------------------------------------------------------------------
# 3. paged == slab bit for bit, run to run reproducible
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_tree_attention_paged_equals_the_slab_and_is_reproducible(kind, hd):
    nh, nkv, Tq = 8, 2, 33
    tree = _branching(Tq)
    lens, extra = LENS[2]
    L, scale = max(lens) + Tq + extra, 1.0 / math.sqrt(hd)
    q = EX._query(hd, nh, Tq)
    bufs, _, _ = _values(kind, hd, nkv)
    slabs = [_slab(t, L) for t in bufs]
    ref = _tree_attn(q, slabs, L, scale, lens, tree)
    assert bool(torch.isfinite(ref).all())
    ws = torch.full((64 << 20,), 0xFF, dtype=torch.uint8, device=DEV)          # a caller's workspace, dirty
    o = torch.empty_like(q)
    again = _tree_attn(q, slabs, L, scale, lens, tree, out=o, workspace=ws)
    assert again is o and _same(again, ref)
    assert not _same(ref, _causal(kind, q, slabs, L, scale, lens))             # (the mask is not the causal one)
    for ps in (16, 128):
        mp = -(-L // ps)
        vals = [_slab(t, mp * ps) for t in bufs]
        num_pages = 3 * mp + 1
        perm = _perm(num_pages, ps + hd)
        table = [perm[b * mp:(b + 1) * mp] for b in range(3)]
        assert _same(_tree_attn(q, _pool_of(vals, table, num_pages, ps), L, scale, lens, tree, table), ref), (kind, hd, ps)


# ---------------------------------------------------------------------------------------------------------------------
# 4. rows it must not read
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_tree_attention_never_reads_invisible_rows(kind, paged):
    """NaN (codes 0xFF under NaN meta) in every row at or beyond lens[b] + Tq, in every page no sequence holds, and -1 in the
    table entries beyond a sequence's pages: the bits of the clean run, and finite.  (Sibling tree rows stay clean: they share
    tiles with rows other queries see, as step rows do in the causal kernel.)"""
    hd, (nh, nkv), Tq, ps = 128, (8, 2), 33, 16
    tree = _branching(Tq)
    lens, extra = LENS[2]
    L, scale = max(lens) + Tq + extra, 1.0 / math.sqrt(hd)
    q = EX._query(hd, nh, Tq)
    bufs, _, _ = _values(kind, hd, nkv)
    fills = _fills(kind)
    if not paged:
        clean = _tree_attn(q, [_slab(t, L) for t in bufs], L, scale, lens, tree)
        dirty = []
        for t, fill in zip(bufs, fills):
            s = _slab(t, L + 9, fill)
            for b, n in enumerate(lens):
                s[b, :, n + Tq:] = fill
            dirty.append(s)
        o = _tree_attn(q, dirty, L, scale, lens, tree)
    else:
        mp = -(-L // ps)
        num_pages = 3 * mp + 3
        perm = _perm(num_pages, 11)
        full = [perm[b * mp:(b + 1) * mp] for b in range(3)]
        vals = [_slab(t, mp * ps) for t in bufs]
        clean = _tree_attn(q, _pool_of(vals, full, num_pages, ps), L, scale, lens, tree, full)
        held = [-(-(n + Tq) // ps) for n in lens]
        table = [full[b][:held[b]] + [-1] * (mp - held[b]) for b in range(3)]
        pools = []
        for t, fill in zip(vals, fills):
            s = t.clone()
            for b, n in enumerate(lens):
                s[b, :, n + Tq:] = fill
            pool = torch.full((num_pages, nkv, ps, t.shape[3]), fill, dtype=t.dtype, device=DEV)
            EX._scatter_held(pool, table, s, held)
            pools.append(pool)
        o = _tree_attn(q, pools, L, scale, lens, tree, table)
    assert bool(torch.isfinite(clean).all()) and bool(torch.isfinite(o).all())
    assert _same(o, clean), (kind, paged)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the commit kernel
# ---------------------------------------------------------------------------------------------------------------------
LAYERS, CBS, CNKV, CTQ = 3, 4, 2, 8
ROW_KINDS = ((F32, 2), (torch.uint8, 64), (BF16, 128))                # rows of 8, 64 and 256 bytes


def _random_bytes(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    return torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8).view(dtype).reshape(shape).to(DEV)


def _valid_moves(path, Tq):
    """The (destination i, source a) pairs the commit's rule admits for one sequence's accept row."""
    moves, prev = [], -1
    for i, a in enumerate(path):
        if not (i <= a < Tq and a > prev):
            break
        prev = a
        if a != i:
            moves.append((i, a))
    return moves


def _pad(paths, Tq):
    return torch.tensor([p + [-1] * (Tq - len(p)) for p in paths], dtype=torch.int32, device=DEV)


ACCEPTS = {
    "paths": [[0, 2, 5], [], [1, 2, 3], [0, 1, 2, 3]],                # [1, 2, 3]: destination 1 is the first move's source
    "ascent": [[0, 3, 2, 5], [2, 1, 4], [0, 0, 5], [1, 8, 3]],         # the entry that breaks the rule ends the moves
    "full": [[4, 5, 6, 7], [7], [0, 1, 2, 3, 4, 5, 6, 7], [1, 3, 5, 7]],
}


@pytest.mark.parametrize("case", list(ACCEPTS))
def test_commit_compacts_the_accepted_rows_of_a_slab(case):
    cap, lens = 48, [5, 0, 17, 30]
    acc = ACCEPTS[case]
    for si, (dtype, x) in enumerate(ROW_KINDS):
        big = _random_bytes((LAYERS + 2, CBS, CNKV, cap, x), dtype, 7 + si)
        want = big.clone()
        for b, path in enumerate(acc):
            for i, a in _valid_moves(path, CTQ):
                want[1:-1, b, :, lens[b] + i] = big[1:-1, b, :, lens[b] + a]
        got = ops.kv_tree_commit(big[1:-1], _i32(lens), _pad(acc, CTQ))
        assert got.data_ptr() == big[1:-1].data_ptr()
        assert _same(big, want), (case, dtype)                       # the compacted rows, and every other byte unchanged
        if case == "paths":
            assert not _same(big[1, 2, :, lens[2] + 1], big[1, 2, :, lens[2] + 0])
        one = _random_bytes((CBS, CNKV, cap, x), dtype, 17 + si)      # a per-layer cache's buffer: layers = 1
        want = one.clone()
        for b, path in enumerate(acc):
            for i, a in _valid_moves(path, CTQ):
                want[b, :, lens[b] + i] = one[b, :, lens[b] + a]
        ops.kv_tree_commit(one, _i32(lens), _pad(acc, CTQ))
        assert _same(one, want)


def test_commit_skips_rows_out_of_range_on_a_slab():
    """Sequence 0: sources beyond the capacity; sequence 1: a negative length, whose rows below 0 are skipped as a source and
    as a destination; sequence 2: a length beyond the capacity; sequence 3 (never the last rows of the allocation: the guard
    layers follow) moves as usual."""
    cap, lens = 40, [36, -2, 45, 20]
    acc = [[1, 5, 6], [1, 3, 4], [2, 3], [3, 4]]
    for si, (dtype, x) in enumerate(ROW_KINDS):
        big = _random_bytes((LAYERS + 2, CBS, CNKV, cap, x), dtype, 27 + si)
        want = big.clone()
        want[1:-1, 0, :, 36] = big[1:-1, 0, :, 37]
        want[1:-1, 1, :, 0] = big[1:-1, 1, :, 2]
        want[1:-1, 3, :, 20] = big[1:-1, 3, :, 23]
        want[1:-1, 3, :, 21] = big[1:-1, 3, :, 24]
        ops.kv_tree_commit(big[1:-1], _i32(lens), _pad(acc, CTQ))
        assert _same(big, want), dtype


@pytest.mark.parametrize("ps", [16, 64])
def test_commit_on_page_pools(ps):
    """The same paths through a page table, the moves crossing page edges; entries of -1 and num_pages (unheld pages) skip the
    moves that touch them, and pages no sequence holds keep their bytes."""
    mp, lens = 3, [ps - 3, 0, ps + 13 if ps == 16 else ps - 1, 2 * ps - 2]
    num_pages = CBS * mp + 3
    perm = _perm(num_pages, ps)
    table = [perm[b * mp:(b + 1) * mp] for b in range(CBS)]
    for name, acc in list(ACCEPTS.items()) + [("unheld", ACCEPTS["full"])]:
        tab = [list(r) for r in table]
        if name == "unheld":
            tab[0][1] = -1                                           # sequence 0's moves reach into its second page
            tab[3][1] = num_pages
        dev_tab = torch.tensor(tab, dtype=torch.int32, device=DEV)

        def where(b, j):
            page = tab[b][j // ps] if 0 <= j < mp * ps else -1
            return (page, j % ps) if 0 <= page < num_pages else None
        for si, (dtype, x) in enumerate(ROW_KINDS):
            big = _random_bytes((LAYERS + 2, num_pages, CNKV, ps, x), dtype, 37 + si)
            want = big.clone()
            for b, path in enumerate(acc):
                for i, a in _valid_moves(path, CTQ):
                    src, dst = where(b, lens[b] + a), where(b, lens[b] + i)
                    if src is not None and dst is not None:
                        want[1:-1, dst[0], :, dst[1]] = big[1:-1, src[0], :, src[1]]
            ops.kv_tree_commit(big[1:-1], _i32(lens), _pad(acc, CTQ), page_table=dev_tab)
            assert _same(big, want), (name, ps, dtype)
            assert name == "ascent" or not _same(big, _random_bytes(big.shape, dtype, 37 + si))       # (something moved)


# ---------------------------------------------------------------------------------------------------------------------
# 6. blocks end to end
# ---------------------------------------------------------------------------------------------------------------------
#       0          6
#     1   2        7
#    3 4   5       8
TREE9 = [-1, 0, 0, 1, 1, 2, -1, 6, 7]
LEAF_PATHS = ([0, 1, 3], [0, 1, 4], [0, 2, 5], [6, 7, 8])
ACCEPT9 = [[0, 1, 4], [], [6, 7]]
TREE_BLOCKS = {                                         # RAGGED_BLOCKS entry, code_bits of the cache
    "wo_llama_gqa": ("wo_llama_gqa", None),
    "wo_opt": ("wo_opt", None),
    "a4_gqa_codes": ("a4_gqa_codes", 4),
    "wo_llama_gqa_codes8": ("wo_llama_gqa", 8),
}
TP = max(PROMPTS)
NUM_PAGES, PS = 12, 16


def _new_cache(case, storage, layers=1):
    name, code_bits = TREE_BLOCKS[case]
    _, _, nh, nkv, _, _ = RAGGED_BLOCKS[name]
    hd = RG.H // nh
    if storage == "pool":
        pool = PagedKVPool(layers, 3, nkv, hd, BF16, DEV, NUM_PAGES, page_size=PS, code_bits=code_bits)
        return [pool.layer(l) for l in range(layers)], pool
    if storage == "paged":
        return [PagedKVCache(3, nkv, hd, BF16, DEV, NUM_PAGES, page_size=PS, code_bits=code_bits) for _ in range(layers)], None
    return [PackedKVCache(3, nkv, hd, BF16, DEV, capacity=TP + 16, code_bits=code_bits, ragged=True) for _ in range(layers)], None


def _model(blk, fam, x, caches, mask=None, pos=None, chain=True, **kw):
    """The block applied once per cache.  chain=False: every layer receives the same rows x and the last layer's output is
    returned (a tree step and the linear step round their outputs differently, so only layers fed the same inputs can hold the
    same rows bit for bit)."""
    for c in caches:
        args = dict(attention_mask=mask, past_key_value=c, use_cache=True, **kw)
        if pos is not None and fam == "llama":
            args["position_ids"] = pos
        with torch.no_grad():
            out, present = blk(x, **args)
        assert present is c
        x = out if chain else x
    return out


def _prompts():
    seqs = [_x(1, n, 30 + i) for i, n in enumerate(PROMPTS)]
    X = _x(3, TP, 29)
    for i, n in enumerate(PROMPTS):
        X[i, :n] = seqs[i][0]
    return seqs, X


def _prefill(blk, fam, caches):
    return _model(blk, fam, _prompts()[1], caches, KD._causal(TP).expand(3, 1, TP, TP), torch.arange(TP, device=DEV)[None],
                  new_tokens=PROMPTS)


@pytest.mark.parametrize("storage", ["slab", "paged", "pool"])
@pytest.mark.parametrize("case", list(TREE_BLOCKS))
def test_blocks_verify_a_tree_and_commit_a_path(case, storage):
    name, _ = TREE_BLOCKS[case]
    build, fam, _, _, _, a4 = RAGGED_BLOCKS[name]
    blk = build()
    layers = 2 if storage == "pool" else 1
    tree = TokenTree(TREE9)
    assert tree.Tq == 9 and tree.height == 3
    nodes = _x(3, 9, 55)                                             # the draft tokens' hidden states
    counts = [len(p) for p in ACCEPT9]
    caches, pool = _new_cache(case, storage, layers)
    _prefill(blk, fam, caches)
    free0 = caches[0].n_free if storage != "slab" else None
    out = _model(blk, fam, nodes, caches, chain=False, tree=tree)
    assert bool(torch.isfinite(out).all())
    top = pool or caches[0]
    assert top._tree_pending == 9 and top.length == TP                                           # nothing moved
    assert storage == "pool" or top.lengths.tolist() == PROMPTS      # (the pool's lengths are read once, at the end)
    if layers == 1:
        # every root path: the tree step's rows of a path are the rows of the sequence continued by that path alone
        seqs = _prompts()[0]
        for i, n in enumerate(PROMPTS):
            for path in LEAF_PATHS:
                x = torch.cat([seqs[i], nodes[i:i + 1, path]], dim=1)
                RG._agree(out[i:i + 1, path], RG._alone(blk, fam, x)[0][:, n:], x[:, n:], BF16, a4)
    # commit one path per sequence; the second cache runs the ordinary linear step of the accepted tokens
    lin_caches, lin_pool = _new_cache(case, storage, layers)
    _prefill(blk, fam, lin_caches)
    X = _x(3, 9, 56)
    for i, path in enumerate(ACCEPT9):
        X[i, :len(path)] = nodes[i, path]
    if storage == "pool":
        accept = torch.tensor([p + [-1] * (9 - len(p)) for p in ACCEPT9], dtype=torch.int32, device=DEV)
        pool.commit_tree(tree, accept)
        assert pool._tree_pending is None and pool.length == TP + tree.height
        _model(blk, fam, X, lin_caches, chain=False, new_tokens=_i32(counts))
        # the host bounds differ (tree.height against the step's 9 rows) and the decode kernel walks its keys by the bound:
        # give the next step of both pools one bound, without reading a length
        assert lin_pool.length == TP + 9
        pool.set_lengths(pool.lengths.clone(), bound=lin_pool.length)
    else:
        caches[0].commit_tree(tree, ACCEPT9)
        assert caches[0]._tree_pending is None and caches[0].length == TP + max(counts)
        _model(blk, fam, X, lin_caches, new_tokens=counts)
    if storage == "paged":
        assert caches[0].n_free == lin_caches[0].n_free and caches[0].n_free > free0 - 3
        assert [len(caches[0].pages(b)) for b in range(3)] == [-(-(n + c) // PS) for n, c in zip(PROMPTS, counts)]
    def same_rows(rows):
        for l, (c, lc) in enumerate(zip(caches, lin_caches)):
            for b in range(3):
                for got, ref in zip(c.sequence(b), lc.sequence(b)):
                    assert got.shape[1] == rows[b] and _same(got, ref), (case, storage, l, b)
    if storage != "pool":                                          # (the pool's lengths are read once, at the end)
        same_rows([n + c for n, c in zip(PROMPTS, counts)])
    step = _x(3, 1, 57)
    o_tree, o_lin = _model(blk, fam, step, caches, chain=False), _model(blk, fam, step, lin_caches, chain=False)
    assert _same(o_tree, o_lin), (case, storage)
    after = [n + c + 1 for n, c in zip(PROMPTS, counts)]
    same_rows(after)
    assert (pool or caches[0]).lengths.tolist() == after == (lin_pool or lin_caches[0]).lengths.tolist()      # read at the end


# ---------------------------------------------------------------------------------------------------------------------
# 7. loud errors
# ---------------------------------------------------------------------------------------------------------------------
def _state(c):
    paged = [[c.pages(b) for b in range(c.bs)], c.n_free] if getattr(c, "paged", False) else []
    return [c.lengths.tolist(), c.length, c._tree_pending] + paged


def test_tree_steps_refuse_what_they_do_not_cover():
    blk = RAGGED_BLOCKS["wo_llama_gqa"][0]()
    tree = TokenTree(TREE9)
    nodes = _x(3, 9, 55)
    (cache,), _ = _new_cache("wo_llama_gqa", "slab")
    _prefill(blk, "llama", [cache])
    before = _state(cache)

    def refused(match, c=cache, b=blk, x=nodes, **kw):
        with pytest.raises(OQError, match=match):
            with torch.no_grad():
                b(x, past_key_value=c, use_cache=True, tree=tree, **kw)
    refused("attention_mask", attention_mask=KD._causal(9, TP))
    refused("position_ids", position_ids=torch.arange(TP, TP + 9, device=DEV)[None])
    refused("new_tokens", new_tokens=[9, 9, 9])
    assert _state(cache) == before
    refused("does not fit", x=_x(3, 8, 55))                          # a step of 8 rows for a tree of 9
    uniform = PackedKVCache(3, 2, 64, BF16, DEV, capacity=TP + 16)
    _model(blk, "llama", _prompts()[1], [uniform], KD._causal(TP).expand(3, 1, TP, TP), torch.arange(TP, device=DEV)[None])
    refused("ragged", c=uniform)
    assert uniform.length == TP
    empty = PackedKVCache(3, 2, 64, BF16, DEV, capacity=TP + 16, ragged=True)
    refused("past", c=empty)
    refused("ragged", c=None)
    assert empty.length == 0 and empty.lengths.tolist() == [0, 0, 0]
    try:
        blk.compute_dtype = F32
        f32 = PackedKVCache(3, 2, 64, F32, DEV, capacity=TP + 16, ragged=True)
        _prefill(blk, "llama", [f32])
        refused("bfloat16", c=f32)
        assert f32.length == TP and f32.lengths.tolist() == PROMPTS
    finally:
        blk.compute_dtype = BF16
    _, fq, _ = KD._block("llama_gqa")                                # the fake-quant (unpacked) block
    with pytest.raises(OQError, match="packed"):
        fq(nodes, tree=tree)
    _, fq_opt, _ = KD._block("opt")
    with pytest.raises(OQError, match="packed"):
        fq_opt(nodes, tree=tree)
    assert _state(cache) == before


@pytest.mark.parametrize("storage", ["slab", "paged", "pool"])
def test_commit_refuses_what_it_cannot_apply(storage):
    blk = RAGGED_BLOCKS["wo_llama_gqa"][0]()
    tree = TokenTree(TREE9)
    layers = 2 if storage == "pool" else 1
    caches, pool = _new_cache("wo_llama_gqa", storage, layers)
    top = pool or caches[0]
    _prefill(blk, "llama", caches)
    before = _state(top)
    with pytest.raises(OQError, match="no pending tree"):
        top.commit_tree(tree, ACCEPT9)
    assert _state(top) == before
    if storage == "pool":
        with torch.no_grad():                                        # one of two layers has stepped: mid-step
            blk(_x(3, 9, 55), past_key_value=caches[0], use_cache=True, tree=tree)
        with pytest.raises(OQError, match="mid-step"):
            pool.commit_tree(tree, ACCEPT9)
        with torch.no_grad():
            blk(_x(3, 9, 55), past_key_value=caches[1], use_cache=True, tree=tree)
        with pytest.raises(OQError, match="on the pool"):
            caches[0].commit_tree(tree, ACCEPT9)
    else:
        _model(blk, "llama", _x(3, 9, 55), caches, tree=tree)
    pending = _state(top)
    assert pending[:3] == [PROMPTS, TP, 9]
    for bad in ([[0, 1, 4], [], [7]], [[0, 4], [], []], [[1, 3], [], []], [[0, 1, 9], [], []], [[0, 1, 4], []]):
        with pytest.raises(OQError, match="root path|paths for a batch"):
            top.commit_tree(tree, bad)
    with pytest.raises(OQError, match="pending tree step has 9"):
        top.commit_tree(TokenTree(TREE9[:8]), [[0], [], []])
    with pytest.raises(OQError, match="int32"):
        top.commit_tree(tree, torch.zeros(3, 9, dtype=torch.int64, device=DEV))
    assert _state(top) == pending
    # any other change of state drops the pending tree: its rows are scratch
    top.set_lengths(PROMPTS)
    assert top._tree_pending is None
    with pytest.raises(OQError, match="no pending tree"):
        top.commit_tree(tree, ACCEPT9)
    _model(blk, "llama", _x(3, 9, 55), caches, tree=tree)
    assert top._tree_pending == 9
    _model(blk, "llama", _x(3, 1, 57), caches)                       # a normal step
    assert top._tree_pending is None and top.lengths.tolist() == [n + 1 for n in PROMPTS]


def test_the_abi_refuses_by_return_code():
    from omniquant_amd import _capi as C
    lib = C.load()
    hd, nh, nkv, Tq, L = 64, 4, 2, 16, 48
    q = EX._query(hd, nh, Tq)
    bufs, _, _ = _values("bf16", hd, nkv)
    kc, vc = (_slab(t, L) for t in bufs)
    lens = _i32([0, 5, 32])
    anc = TokenTree([-1] + list(range(Tq - 1))).to(DEV).anc
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    o = torch.full_like(q, 7.0)

    def call(dtype=C.OQ_BF16, bits=0, Tq=Tq, hd=hd, L=L, anc=anc, anc_bs=1):
        return lib.oq_attn_tree(C.ptr(q), C.ptr(kc), C.ptr(vc), None, None, C.ptr(o), dtype, bits, 3, Tq, nh, nkv, hd, L, None, 0, 0, 0,
                                C.ptr(lens), L, C.ptr(anc), anc_bs, 1.0 / math.sqrt(hd), C.ptr(ws), ws.numel(), C.stream())
    assert call(Tq=65, L=96) != 0 and "64" in lib.oq_last_error().decode()
    assert call(dtype=C.OQ_F32) != 0 and "bf16" in lib.oq_last_error().decode()
    assert call(hd=96) != 0
    assert call(anc=None) != 0 and "anc" in lib.oq_last_error().decode()
    assert call(anc_bs=2) != 0 and "anc_bs" in lib.oq_last_error().decode()
    assert call(bits=3) != 0
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                                    # nothing was launched
    assert call() == 0
    assert _same(o, ops.extend_attention(q, kc, vc, L, 1.0 / math.sqrt(hd), lens))
    buf = torch.zeros(3, 2, 16, 8, dtype=torch.uint8, device=DEV)
    accept = torch.full((3, 4), -1, dtype=torch.int32, device=DEV)

    def commit(row_bytes=8, Tq=4, buf=buf, accept=accept):
        return lib.oq_kv_tree_commit(C.ptr(buf), row_bytes, 1, 0, 3, 2, 16, None, 0, 0, 0, C.ptr(lens), C.ptr(accept), Tq, C.stream())
    assert commit(Tq=65) != 0 and commit(Tq=0) != 0 and commit(row_bytes=6) != 0 and commit(accept=None) != 0
    assert commit() == 0
    with pytest.raises(OQError, match="64 nodes"):
        ops.tree_attention(torch.zeros(3, 65, nh, hd, dtype=BF16, device=DEV), (kc, vc), 96, 0.125, lens, anc)
    with pytest.raises(OQError, match="ancestor sets"):
        ops.tree_attention(q, (kc, vc), L, 0.125, lens, TokenTree([-1, 0, 1]))
    with pytest.raises(OQError, match="bfloat16"):
        ops.tree_attention(q.float(), (kc.float(), vc.float()), L, 0.125, lens, anc)
    with pytest.raises(OQError, match="accept"):
        ops.kv_tree_commit(buf, lens, accept.long())
    with pytest.raises(OQError, match="contiguous"):
        ops.kv_tree_commit(buf[:, :, ::2], lens, accept)
