"""The model-wide paged KV pool: the page-move kernels of csrc/oq_kvpool.hip against torch indexing (bit for bit), and
kvcache.PagedKVPool -- one allocator, one page table and one set of lengths for all layers -- against per-layer PagedKVCaches
driven by the same calls (bit for bit, because a layer's view hands the same kernels the same pools, table and lengths): the
model step, one table upload per step, the step protocol, set_lengths / fork for all layers at once, and the swap of a sequence
to pinned host memory and back.  The "model" is one packed block applied LAYERS times, layer l reading layer l - 1's output,
on LAYERS per-layer caches or on the LAYERS views of one pool."""
import pytest
import torch

import test_hip_kv_decode as KD
import test_hip_kv_ragged as RG
from omniquant_amd import OQError, ops
from omniquant_amd.block_common import EXTEND_MIN_TQ
from omniquant_amd.kvcache import PagedKVCache, PagedKVPool, SwappedSequence
from test_hip_kv_ragged import PROMPTS, RAGGED_BLOCKS, STEPS, _same, _x

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
LAYERS, PS, CHUNK = 3, 16, 16
assert CHUNK >= EXTEND_MIN_TQ


# ---------------------------------------------------------------------------------------------------------------------
# 1. the page-move kernels against torch indexing
# ---------------------------------------------------------------------------------------------------------------------
SENT = 0x5A


def _u8(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=g)


def _ids(seq):
    return torch.tensor(seq, dtype=torch.int32, device=DEV)


def _pool_slice(layers, num_pages, pb, seed):
    """`layers` layers from the middle of a larger allocation (a layer offset), and the whole allocation."""
    big = _u8((layers + 2, num_pages, pb), seed)
    return big[1:1 + layers], big


def _valid(ids, num_pages):
    return [j for j, p in enumerate(ids) if 0 <= p < num_pages]


@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("pb", [256, 384, 20480, 65536])
def test_gather_and_scatter_equal_torch_indexing(pb, layers):
    num_pages = 9
    pool, big = _pool_slice(layers, num_pages, pb, pb + layers)
    ids = [4, -1, 0, 8, num_pages, 4, 2, num_pages + 7, -5, 0]            # skipped ids and duplicates
    keep = _valid(ids, num_pages)
    # gather: the pages named, in order; the rows of skipped ids keep the sentinel; the pool is only read
    before = big.clone()
    dst = torch.full((layers, len(ids), pb), SENT, dtype=torch.uint8, device=DEV)
    want = dst.clone()
    want[:, keep] = pool[:, [ids[j] for j in keep]]
    assert ops.kv_pages_gather(pool, _ids(ids), dst) is dst
    assert torch.equal(dst, want) and torch.equal(big, before)
    fresh = ops.kv_pages_gather(pool, _ids([p for p in ids if 0 <= p < num_pages]))
    assert fresh.shape == (layers, len(keep), pb) and fresh.dtype == torch.uint8 and torch.equal(fresh, want[:, keep])
    # scatter: duplicates carry the same bytes (which of two different ones would win is not defined, here as in torch)
    src = _u8((layers, len(ids), pb), 3 * pb + layers)
    for j, p in enumerate(ids):
        src[:, j] = src[:, ids.index(p)]
    want = big.clone()
    want[1:1 + layers][:, [ids[j] for j in keep]] = src[:, keep]
    ops.kv_pages_scatter(src, pool, _ids(ids))
    assert torch.equal(big, want)                                          # the layers around the slice and unnamed pages included
    # n = 0: nothing moves
    empty = torch.empty((layers, 0, pb), dtype=torch.uint8, device=DEV)
    ops.kv_pages_gather(pool, _ids([]), empty)
    ops.kv_pages_scatter(empty, pool, _ids([]))
    ops.kv_pages_copy(pool, _ids([]), _ids([]))
    assert torch.equal(big, want)


@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("pb", [256, 65536])
def test_copy_equals_torch_indexing(pb, layers):
    num_pages = 12
    pool, big = _pool_slice(layers, num_pages, pb, 7 * pb + layers)
    # disjoint sources and destinations, one source copied twice
    src, dst = [0, 3, 5, 3], [7, 8, 10, 11]
    want = big.clone()
    want[1:1 + layers][:, dst] = pool[:, src]
    ops.kv_pages_copy(pool, _ids(src), _ids(dst))
    assert torch.equal(big, want)
    # pairs with src == dst and pairs with an id outside the pool are skipped
    src, dst = [2, 4, -1, 6, num_pages, 9], [2, 1, 0, num_pages, 5, 9]
    want[1:1 + layers][:, 1] = want[1:1 + layers][:, 4]
    ops.kv_pages_copy(pool, _ids(src), _ids(dst))
    assert torch.equal(big, want)


def test_moves_whose_grid_strides():
    """More page slices than the launch has workgroups: 36 MiB of 64 KiB pages (192 pages x 3 layers), and 12000 ids of 256-byte
    pages x 3 layers."""
    layers, num_pages, pb = 3, 192, 65536
    pool, big = _pool_slice(layers, num_pages, pb, 11)
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(5)).tolist()
    got = ops.kv_pages_gather(pool, _ids(perm))
    assert torch.equal(got, pool[:, perm])
    target = torch.full_like(pool, SENT)
    ops.kv_pages_scatter(got, target, _ids(perm))
    assert torch.equal(target, pool)
    half = num_pages // 2
    want = big.clone()
    want[1:1 + layers][:, perm[half:]] = pool[:, perm[:half]]
    ops.kv_pages_copy(pool, _ids(perm[:half]), _ids(perm[half:]))
    assert torch.equal(big, want)
    small, _ = _pool_slice(layers, 500, 256, 13)
    many = torch.randint(-3, 503, (12000,), generator=torch.Generator().manual_seed(6)).tolist()
    keep = _valid(many, 500)
    dst = torch.full((layers, len(many), 256), SENT, dtype=torch.uint8, device=DEV)
    want = dst.clone()
    want[:, keep] = small[:, [many[j] for j in keep]]
    ops.kv_pages_gather(small, _ids(many), dst)
    assert len(keep) < len(many) and torch.equal(dst, want)


# ---------------------------------------------------------------------------------------------------------------------
# the model: one block applied LAYERS times
# ---------------------------------------------------------------------------------------------------------------------
CASES = {                                  # RAGGED_BLOCKS entry, code_bits of the cache, compute dtype
    "bf16": ("wo_llama_gqa", None, BF16),
    "f32": ("wo_llama_gqa", None, F32),
    "opt_bf16": ("wo_opt", None, BF16),
    "codes4": ("a4_gqa_codes", 4, BF16),
    "codes8": ("wo_llama_gqa", 8, BF16),
}
NUM_PAGES, MAX_PAGES = 20, 8
TP = max(PROMPTS)
AFTER = [n + STEPS + CHUNK for n in PROMPTS]            # the lengths after _run: [48, 40, 32]


def _block(case):
    name, code_bits, cd = CASES[case]
    build, fam, nh, nkv, _, _ = RAGGED_BLOCKS[name]
    blk = build()
    blk.compute_dtype = cd
    return blk, fam, nkv, RG.H // nh, code_bits, cd


def _caches(case, pooled, num_pages=NUM_PAGES, max_pages=MAX_PAGES, **kw):
    """(what the layers step on, the pool or None): the LAYERS views of one pool, or LAYERS PagedKVCaches."""
    _, _, nkv, hd, code_bits, cd = _block(case)
    if pooled:
        pool = PagedKVPool(LAYERS, 3, nkv, hd, cd, DEV, num_pages, page_size=PS, max_pages=max_pages, code_bits=code_bits, **kw)
        return [pool.layer(l) for l in range(LAYERS)], pool
    return [PagedKVCache(3, nkv, hd, cd, DEV, num_pages, page_size=PS, max_pages=max_pages, code_bits=code_bits)
            for _ in range(LAYERS)], None


def _model(blk, fam, x, caches, mask=None, pos=None, new_tokens=None):
    for c in caches:
        x = RG._step(blk, fam, x, c, mask, pos, new_tokens)
    return x


def _inputs():
    """The right-padded prompt batch, the decode tokens and the 16-row chunk (the same for every run)."""
    seqs = [_x(1, n + STEPS, 30 + i) for i, n in enumerate(PROMPTS)]
    X = _x(3, TP, 29)
    for i, n in enumerate(PROMPTS):
        X[i, :n] = seqs[i][0, :n]
    steps = [torch.stack([seqs[i][0, n + s] for i, n in enumerate(PROMPTS)])[:, None] for s in range(STEPS)]
    return X, steps, _x(3, CHUNK, 41)


def _prefill(blk, fam, caches):
    X = _inputs()[0]
    return _model(blk, fam, X, caches, KD._causal(TP).expand(3, 1, TP, TP), torch.arange(TP, device=DEV)[None], new_tokens=PROMPTS)


def _state(c):
    """(lengths, length, pages, n_free) of a pool or a per-layer cache."""
    return c.lengths.tolist(), c.length, [c.pages(b) for b in range(3)], c.n_free


def _run(case, pooled, check=None, **kw):
    """Right-padded prefill with new_tokens, STEPS mask-free decode steps, one CHUNK-row step with a past.  Returns (block,
    family, caches, pool, the outputs of every step, the state after every step)."""
    blk, fam = _block(case)[:2]
    caches, pool = _caches(case, pooled, **kw)
    _, steps, chunk = _inputs()
    outs, states = [_prefill(blk, fam, caches)], []
    states.append(_state(pool or caches[0]))
    for xs in steps + [chunk]:
        outs.append(_model(blk, fam, xs, caches))
        states.append(_state(pool or caches[0]))
    return blk, fam, caches, pool, outs, states


_REF = {}


def _per_layer(case):
    """The model on per-layer PagedKVCaches: computed once per case and left alone."""
    if case not in _REF:
        _, _, caches, _, outs, states = _run(case, False)
        _REF[case] = (caches, outs, states, [[c.sequence(b) for b in range(3)] for c in caches])
    return _REF[case]


def _restore(case):
    RAGGED_BLOCKS[CASES[case][0]][0]().compute_dtype = BF16


# ---------------------------------------------------------------------------------------------------------------------
# 2. a model on the pool equals the model on per-layer caches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_model_on_the_pool_equals_per_layer_caches_bit_for_bit(case):
    try:
        ref_caches, ref_outs, ref_states, ref_rows = _per_layer(case)
        _, _, views, pool, outs, states = _run(case, True)
        assert len(outs) == STEPS + 2 and all(_same(o, r) for o, r in zip(outs, ref_outs)), case
        assert states == ref_states                               # lengths, length, pages(b), n_free after every step
        assert states[-1][0] == AFTER and states[-1][1] == TP + STEPS + CHUNK
        for c in ref_caches[1:]:
            assert _state(c) == ref_states[-1]
        cd, code_bits = CASES[case][2], CASES[case][1]
        for l, view in enumerate(views):
            assert view is pool.layer(l) and isinstance(view, PagedKVCache) and view.ragged and view.paged
            assert (view.bs, view.nkv, view.hd, view.dtype, view.device) == (3, pool.nkv, pool.hd, cd, torch.device(DEV))
            assert (view.code_bits, view.page_size, view.capacity, view.length) == (code_bits, PS, MAX_PAGES * PS, pool.length)
            assert view.page_table is pool.page_table and view.lengths is pool.lengths
            for name in pool._buffers():
                t = getattr(view, name)
                assert t.is_contiguous() and t.data_ptr() == getattr(pool, name)[l].data_ptr()
            for b in range(3):
                assert view.pages(b) == pool.pages(b)
                (k, v), (rk, rv) = view.sequence(b), ref_rows[l][b]
                assert k.shape == (pool.nkv, AFTER[b], pool.hd) and _same(k, rk) and _same(v, rv), (case, l, b)
        shape = (LAYERS, NUM_PAGES, pool.nkv, PS)
        if code_bits is None:
            assert pool.k.shape == pool.v.shape == shape + (pool.hd,) and pool.k.dtype == cd
        else:
            assert pool.k_codes.shape == shape + (pool.hd * code_bits // 8,) and pool.k_meta.shape == shape + (2,)
        assert pool.nbytes() == sum(c.nbytes() for c in ref_caches) - (LAYERS - 1) * pool.page_table.numel() * 4
        assert "PagedKVPool(layers=3" in repr(pool) and f"of {NUM_PAGES} pages free" in repr(pool)
        blk, fam = _block(case)[:2]
        with pytest.raises(OQError, match="pass pool.layer"):
            RG._step(blk, fam, _inputs()[1][0], pool)
        for call in (lambda: views[0].set_lengths([0, 0, 0]), lambda: views[1].fork(0, 1), lambda: views[2].clone(),
                     lambda: pool.sequence(0)):
            with pytest.raises(OQError, match="pool"):
                call()
    finally:
        _restore(case)


# ---------------------------------------------------------------------------------------------------------------------
# 3. one upload per step, no host reads
# ---------------------------------------------------------------------------------------------------------------------
def _count_uploads(obj, counter):
    inner = obj._upload

    def counted():
        counter.append(obj)
        inner()
    obj._upload = counted


def test_one_table_upload_per_step_and_no_host_reads():
    case = "bf16"
    blk, fam = _block(case)[:2]
    steps = _inputs()[1]
    for pooled, want in ((True, 1), (False, LAYERS)):
        caches, pool = _caches(case, pooled)
        _prefill(blk, fam, caches)
        uploads = []
        for obj in ([pool] if pooled else caches):
            _count_uploads(obj, uploads)
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            # sequence 1 stands at 16 rows: its next row opens a page; the step after it stays inside the pages held
            _model(blk, fam, steps[0], caches)
            crossing = len(uploads)
            _model(blk, fam, steps[1], caches)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert crossing == want and len(uploads) == want, (pooled, crossing, len(uploads))
        assert (pool or caches[0]).lengths.tolist() == [n + 2 for n in PROMPTS]


# ---------------------------------------------------------------------------------------------------------------------
# 4. the step protocol
# ---------------------------------------------------------------------------------------------------------------------
def test_step_protocol_violations_leave_the_pool_unchanged():
    case = "bf16"
    blk, fam = _block(case)[:2]
    steps = _inputs()[1]
    views, pool = _caches(case, True)
    _prefill(blk, fam, views)
    start = _state(pool)
    assert start[:2] == (PROMPTS, TP)
    two = _x(3, 2, 43)

    def violates(match, call):
        before = _state(pool), pool.page_table.tolist()
        with pytest.raises(OQError, match=match):
            call()
        assert (_state(pool), pool.page_table.tolist()) == before
        assert before[0][:2] == start[:2]                         # and no length has moved since the prefill

    # layer 0 steps twice before layer 1
    RG._step(blk, fam, steps[0], views[0])
    violates("layer 0 steps twice", lambda: RG._step(blk, fam, steps[0], views[0]))
    # a pool call in mid-step
    violates("fork in mid-step", lambda: pool.fork(0, 1))
    violates("swap_out in mid-step", lambda: pool.swap_out(1))
    violates("set_lengths in mid-step", lambda: pool.set_lengths(PROMPTS))
    violates("swap_in in mid-step", lambda: pool.swap_in(1, None))
    violates("reserve in mid-step", lambda: pool.reserve(1))
    violates("advance in mid-step", lambda: pool.advance(1))
    # a differing Tq
    violates("layer 1 steps 2 rows, the step's first layer 1", lambda: RG._step(blk, fam, two, views[1]))
    pool.abort_step()
    # differing new_tokens: Python counts, and a device tensor against counts
    RG._step(blk, fam, two, views[0], new_tokens=[1, 2, 1])
    violates("layer 1's new_tokens differ", lambda: RG._step(blk, fam, two, views[1], new_tokens=[2, 1, 1]))
    pool.abort_step()
    RG._step(blk, fam, two, views[2], new_tokens=[1, 2, 1])
    dev = torch.tensor([1, 2, 1], dtype=torch.int32, device=DEV)
    violates("layer 0's new_tokens differ", lambda: RG._step(blk, fam, two, views[0], new_tokens=dev))
    pool.abort_step()
    assert _state(pool)[:2] == start[:2]
    # after abort_step a full step (layers in another order: each reads and writes its own pools) succeeds and matches
    ref_caches, _ = _caches(case, False)
    _prefill(blk, fam, ref_caches)
    want = [RG._step(blk, fam, steps[0], c) for c in ref_caches]
    got = {l: RG._step(blk, fam, steps[0], views[l]) for l in (2, 0, 1)}
    assert all(_same(got[l], want[l]) for l in range(LAYERS))
    assert _state(pool) == _state(ref_caches[0]) and pool.lengths.tolist() == [n + 1 for n in PROMPTS]
    for l in range(LAYERS):
        for b in range(3):
            assert all(_same(a, r) for a, r in zip(views[l].sequence(b), ref_caches[l].sequence(b)))
    # a device tensor as new_tokens: the same tensor for every layer; the host then holds bounds only
    _model(blk, fam, two, views, new_tokens=dev)
    assert pool.lengths.tolist() == [n + 1 + d for n, d in zip(PROMPTS, [1, 2, 1])] and pool.length == TP + 3
    with pytest.raises(OQError, match="swap_out: the host holds only an upper bound"):
        pool.swap_out(0)


def test_a_failed_fork_leaves_no_queued_page_copies():
    """An exception behind fork's page copy (here: the table upload) must not leave the pair queued for the next launch."""
    _, pool = _caches("bf16", True)
    pool.set_lengths([20, 0, 0])

    def broken():
        raise RuntimeError("upload failed")
    pool._upload = broken
    with pytest.raises(RuntimeError, match="upload failed"):
        pool.fork(0, 1)
    assert pool._copies == []


# ---------------------------------------------------------------------------------------------------------------------
# 5. set_lengths and fork on the pool
# ---------------------------------------------------------------------------------------------------------------------
def test_pool_slot_reuse_fork_and_exhaustion():
    """The sequence of test_hip_kv_paged.test_slot_reuse_fork_and_exhaustion on the pool and on per-layer caches alike (6
    pages): every output and every layer's rows agree bit for bit, and that test's invariants hold on the pool."""
    case = "f32"
    try:
        blk, fam = _block(case)[:2]
        views, pool = _caches(case, True, num_pages=6, max_pages=6)
        refs, _ = _caches(case, False, num_pages=6, max_pages=6)
        alloc = pool.allocator
        seqs = [_x(1, n + STEPS + 8, 30 + i) for i, n in enumerate(PROMPTS)]

        def both(x, **kw):
            o, r = _model(blk, fam, x, views, **kw), _model(blk, fam, x, refs, **kw)
            assert _same(o, r) and _state(pool) == _state(refs[0])
            return o

        def rows_agree():
            for l in range(LAYERS):
                for b in range(3):
                    assert all(_same(a, r) for a, r in zip(views[l].sequence(b), refs[l].sequence(b))), (l, b)

        def set_lengths(seq):
            pool.set_lengths(seq)
            for c in refs:
                c.set_lengths(seq)

        assert _same(_prefill(blk, fam, views), _prefill(blk, fam, refs))
        for s in range(STEPS):
            both(torch.stack([seqs[i][0, n + s] for i, n in enumerate(PROMPTS)])[:, None])
        # ---- slot reuse
        n0, n2 = PROMPTS[0] + STEPS, PROMPTS[2] + STEPS
        free, mine = pool.n_free, len(pool.pages(1))
        assert mine == 2
        set_lengths([n0, 0, n2])
        assert pool.n_free == free + mine and pool.pages(1) == [] and pool.length == n0
        fresh = _x(1, 8, 55)
        at = [n0, 0, n2]
        X = _x(3, 5, 56)
        X[0, 0], X[1, :5], X[2, 0] = seqs[0][0, at[0]], fresh[0, :5], seqs[2][0, at[2]]
        both(X, new_tokens=[1, 5, 1])
        at = [n0 + 1, 5, n2 + 1]
        assert pool.length == n0 + 5
        for s in range(2):
            both(torch.stack([seqs[0][0, at[0]], fresh[0, 5 + s], seqs[2][0, at[2]]])[:, None])
            at = [n + 1 for n in at]
        assert pool.lengths.tolist() == at == [n0 + 3, 7, n2 + 3]
        assert [len(pool.pages(i)) for i in range(3)] == [-(-n // PS) for n in at]
        rows_agree()
        # ---- fork: full pages shared with reference count 2 (once, not per layer), the partial page private
        set_lengths([at[0], 0, at[2]])
        pool.fork(0, 1)
        for c in refs:
            c.fork(0, 1)
        at[1] = at[0]
        full = at[0] // PS
        p0, p1 = pool.pages(0), pool.pages(1)
        assert at[0] % PS and len(p0) == len(p1) == full + 1
        assert p0[:full] == p1[:full] and all(alloc.refcount(p) == 2 for p in p0[:full])
        assert p0[full] != p1[full] and alloc.refcount(p0[full]) == alloc.refcount(p1[full]) == 1
        assert pool.page_table[:2, :full + 1].tolist() == [p0, p1] and pool.lengths.tolist() == at
        assert _state(pool) == _state(refs[0])
        for l in range(LAYERS):
            assert all(_same(a, b) for a, b in zip(views[l].sequence(0), views[l].sequence(1))), l
            for name in pool._buffers():                          # the partial page: equal bytes, in every layer
                t = getattr(pool, name)
                assert _same(t[l, p0[full]], t[l, p1[full]]), (l, name)
        rows_agree()
        for s in range(2):                                         # equal tokens give equal rows on both slots
            tok = seqs[0][0, at[0]]
            o = both(torch.stack([tok, tok, seqs[2][0, at[2]]])[:, None])
            assert _same(o[0], o[1])
            at = [n + 1 for n in at]
        before = [[views[l].sequence(i) for i in range(2)] for l in range(LAYERS)]
        o = both(torch.stack([seqs[0][0, at[0]], fresh[0, 0], seqs[2][0, at[2]]])[:, None])
        at = [n + 1 for n in at]
        assert not _same(o[0], o[1])
        for l in range(LAYERS):                                    # a differing token leaves the shared prefix untouched
            for i in range(2):
                k, v = views[l].sequence(i)
                assert k.shape[1] == at[i] and _same(k[:, :-1], before[l][i][0]) and _same(v[:, :-1], before[l][i][1])
            assert not _same(views[l].sequence(0)[0][:, -1], views[l].sequence(1)[0][:, -1])
        assert pool.pages(0)[:full] == pool.pages(1)[:full]
        # ---- exhaustion: refused before any launch, the pool unchanged, and the next legal step still works
        state = (_state(pool), pool.page_table.tolist())
        assert pool.n_free == 0
        with pytest.raises(OQError, match="more rows per sequence need 3 pages, 0 are free"):
            views[1].reserve(PS)
        with pytest.raises(OQError, match="more rows per sequence need 3 pages, 0 are free"):
            _model(blk, fam, _x(3, PS, 57), views)
        with pytest.raises(OQError, match="beyond max_pages = 6"):
            views[0].reserve(6 * PS)
        assert (_state(pool), pool.page_table.tolist()) == state
        both(torch.stack([seqs[0][0, at[0]], fresh[0, 1], seqs[2][0, at[2]]])[:, None])
        assert pool.lengths.tolist() == [n + 1 for n in at]
        with pytest.raises(OQError, match="not empty"):
            pool.fork(0, 2)
        c2 = pool.clone()
        assert _state(c2) == _state(pool) and _same(c2.layer(2).sequence(2)[0], views[2].sequence(2)[0])
    finally:
        _restore(case)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 6. swap round trip
# ---------------------------------------------------------------------------------------------------------------------
def _no_sync(call):
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return call()
    finally:
        torch.cuda.set_sync_debug_mode(mode)


# (case, swap_staging_bytes).  Sequence 1 holds 3 pages.  bf16: 4096-byte pages, 12288 bytes a layer: 2 + 1 pages per layer.
# codes4: code pages of 1024 bytes go one by one, the 256-byte meta pages two layers (1536 bytes) and then one at a time.
# codes8: code pages of 2048 bytes as 2 + 1 per layer, all meta pages (2304 bytes) at once.
SWAPS = [("bf16", 10000), ("codes4", 1600), ("codes8", 5000)]


@pytest.mark.parametrize("case,staging", SWAPS)
def test_swap_round_trip(case, staging):
    try:
        blk, fam, views, pool, _, _ = _run(case, True, swap_staging_bytes=staging)
        _, _, tviews, twin, _, _ = _run(case, True, swap_staging_bytes=staging)
        assert _state(pool) == _state(twin) and _state(pool)[0] == AFTER
        page_bytes = {n: getattr(pool, n)[0, 0].numel() * getattr(pool, n).element_size() for n in pool._buffers()}
        held = pool.pages(1)
        assert len(held) == 3 and 3 * max(page_bytes.values()) > staging and (3 * max(page_bytes.values())) % staging
        before = [[v.sequence(b) for b in range(3)] for v in views]
        raw = {n: getattr(pool, n)[:, held].clone() for n in pool._buffers()}
        free = pool.n_free
        # ---- out
        h = _no_sync(lambda: pool.swap_out(1))
        assert isinstance(h, SwappedSequence) and (h.length, h.n_pages) == (AFTER[1], 3)
        assert h.nbytes == LAYERS * 3 * sum(page_bytes.values()) and h.geometry == pool.geometry
        assert pool.n_free == free + 3 and pool.pages(1) == [] and pool.lengths.tolist() == [AFTER[0], 0, AFTER[2]]
        assert pool.page_table[1].tolist() == [-1] * MAX_PAGES
        h.event.synchronize()
        for n in pool._buffers():                                 # the documented layout: [layers, n_pages, page_bytes], pinned
            t = h.buffers[n]
            assert t.is_pinned() and t.dtype == torch.uint8 and t.shape == (LAYERS, 3, page_bytes[n])
            assert torch.equal(t, raw[n].reshape(LAYERS, 3, -1).view(torch.uint8).cpu())
        # ---- a fresh prompt takes slot 1 and the freed pages, slots 0 and 2 decode on; on the twin slot 1 only idles
        n = 40
        X = _x(3, n, 61)
        o = _model(blk, fam, X, views, new_tokens=[1, n, 1])
        t = _model(blk, fam, X, tviews, new_tokens=[1, 0, 1])
        assert _same(o[0, :1], t[0, :1]) and _same(o[2, :1], t[2, :1])
        assert all(not _same(getattr(pool, name)[:, held], raw[name]) for name in pool._buffers())      # the pages were overwritten
        at = [AFTER[0] + 1, AFTER[1], AFTER[2] + 1]
        assert pool.lengths.tolist() == [at[0], n, at[2]] and twin.lengths.tolist() == at
        # ---- in
        pool.set_lengths([at[0], 0, at[2]])
        twin.set_lengths(at)
        state = (_state(pool), pool.page_table.tolist())
        other = _caches(case, True, num_pages=4)[1]
        geo = dict(nkv=pool.nkv, hd=pool.hd, dtype=pool.dtype, device=DEV, code_bits=pool.code_bits)
        tiny = PagedKVPool(LAYERS, 3, num_pages=2, page_size=PS, max_pages=MAX_PAGES, **geo)
        wide = PagedKVPool(LAYERS, 3, num_pages=8, page_size=32, **geo)
        deep = PagedKVPool(LAYERS + 1, 3, num_pages=8, page_size=PS, **geo)
        for target, slot, match in ((pool, 0, "not empty"), (wide, 1, "geometry"), (deep, 1, "geometry"),
                                    (tiny, 1, "needs 3 pages, 2 are free"), (other, 3, "sequence 3")):
            kept = _state(target), target.page_table.tolist()
            with pytest.raises(OQError, match=match):
                target.swap_in(slot, h)
            assert (_state(target), target.page_table.tolist()) == kept
        assert (_state(pool), pool.page_table.tolist()) == state
        _no_sync(lambda: pool.swap_in(1, h))
        assert pool.lengths.tolist() == at and pool.length == twin.length and len(pool.pages(1)) == 3
        assert all(pool.allocator.refcount(p) == 1 for p in pool.pages(1)) and pool.n_free == state[0][3] - 3
        for l in range(LAYERS):
            assert all(_same(a, r) for a, r in zip(views[l].sequence(1), before[l][1])), (case, l)
            for b in (0, 2):                                      # slots 0 and 2: their earlier rows, plus one
                for a, r, tw in zip(views[l].sequence(b), before[l][b], tviews[l].sequence(b)):
                    assert _same(a[:, :-1], r) and _same(a, tw), (case, l, b)
        for s in range(2):
            xs = _x(3, 1, 70 + s)
            assert _same(_model(blk, fam, xs, views), _model(blk, fam, xs, tviews)), (case, s)
        assert pool.lengths.tolist() == twin.lengths.tolist() == [a + 2 for a in at]
        # ---- the handle stays valid: the same rows in slot 2 of the twin, and in a pool that never held them
        twin.set_lengths([at[0] + 2, at[1] + 2, 0])
        twin.swap_in(2, h)
        other.swap_in(0, h)
        for l in range(LAYERS):
            for got in (tviews[l].sequence(2), other.layer(l).sequence(0)):
                assert all(_same(a, r) for a, r in zip(got, before[l][1])), (case, l)
        assert twin.lengths.tolist() == [at[0] + 2, at[1] + 2, AFTER[1]] and other.lengths.tolist() == [AFTER[1], 0, 0]
        # an empty sequence swaps as nothing
        e = other.swap_out(1)
        assert (e.length, e.n_pages, e.nbytes) == (0, 0, 0)
        other.swap_in(2, e)
        assert other.pages(2) == [] and other.lengths.tolist() == [AFTER[1], 0, 0]
    finally:
        _restore(case)
    torch.cuda.synchronize()
