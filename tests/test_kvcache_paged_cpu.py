"""Host-side checks of the paged KV cache that need no GPU: the page allocator (pure Python), the cache's refusal of a CPU
device, and the `page_table` keyword of the five ops, which validates the table, the pools and the excluded arguments on the
host before any device call (every message below comes from those checks, not from the CPU-tensor refusal of the C binding)."""
import pytest
import torch

from omniquant_amd import OQError, ops
from omniquant_amd.kvcache import PageAllocator, PagedKVCache

BS, TQ, NH, NKV, HD, NP, MP, PS = 3, 2, 4, 2, 64, 5, 4, 16
F32 = torch.float32


# ---- PageAllocator ------------------------------------------------------------------------------------------------------
def test_allocator_hands_out_ascending_ids_deterministically():
    runs = []
    for _ in range(2):
        a = PageAllocator(8)
        got = [a.alloc(3), a.alloc(2)]
        a.release([1, 3])
        got += [a.alloc(1), a.alloc(2), a.alloc(0)]
        runs.append(got)
    assert runs[0] == runs[1] == [[0, 1, 2], [3, 4], [1], [3, 5], []]


def test_allocator_alloc_is_all_or_nothing():
    a = PageAllocator(4)
    assert a.alloc(3) == [0, 1, 2]
    state = (a.n_free, [a.refcount(p) for p in range(4)])
    with pytest.raises(OQError, match="alloc"):
        a.alloc(2)
    assert (a.n_free, [a.refcount(p) for p in range(4)]) == state == (1, [1, 1, 1, 0])
    assert a.alloc(1) == [3] and a.n_free == 0
    with pytest.raises(OQError, match="alloc"):
        a.alloc(1)
    with pytest.raises(OQError):
        PageAllocator(0)


def test_allocator_refcounts_free_a_page_only_at_zero():
    a = PageAllocator(4)
    pages = a.alloc(2)
    a.retain(pages)
    a.retain([0])
    assert [a.refcount(p) for p in range(4)] == [3, 2, 0, 0] and a.n_free == 2
    a.release(pages)
    assert [a.refcount(p) for p in range(4)] == [2, 1, 0, 0] and a.n_free == 2
    a.release([1])
    assert a.refcount(1) == 0 and a.n_free == 3
    a.release([0, 0])
    assert a.refcount(0) == 0 and a.n_free == 4
    assert a.alloc(4) == [0, 1, 2, 3]


def test_allocator_n_free_bookkeeping():
    a = PageAllocator(6)
    assert a.n_free == 6
    x = a.alloc(4)
    assert a.n_free == 2
    a.release(x[1:3])
    assert a.n_free == 4
    y = a.alloc(3)
    assert y == [1, 2, 4] and a.n_free == 1
    a.retain(y)
    a.release(y)
    assert a.n_free == 1
    a.release(y + [x[0], x[3]])
    assert a.n_free == 6 and "6 of 6" in repr(a)


def test_allocator_refuses_a_double_release_and_strangers():
    a = PageAllocator(3)
    a.alloc(2)
    a.release([1])
    for bad in ([1], [2], [0, 0], [3], [-1]):
        state = (a.n_free, [a.refcount(p) for p in range(3)])
        with pytest.raises(OQError, match="release"):
            a.release(bad)
        assert (a.n_free, [a.refcount(p) for p in range(3)]) == state
    with pytest.raises(OQError, match="retain"):
        a.retain([1])
    c = a.clone()
    c.release([0])
    assert a.refcount(0) == 1 and c.refcount(0) == 0


# ---- PagedKVCache ---------------------------------------------------------------------------------------------------------
def test_paged_cache_refuses_a_cpu_device():
    for kw in (dict(), dict(code_bits=4), dict(page_size=128, max_pages=2)):
        with pytest.raises(OQError, match="GPU device"):
            PagedKVCache(BS, NKV, HD, torch.bfloat16, "cpu", NP, **kw)


# ---- the page_table keyword of the ops ------------------------------------------------------------------------------------
def _step(ps=PS):
    q = torch.zeros(BS, TQ, NH, HD)
    k = torch.zeros(BS, TQ, NKV, HD)
    pool = torch.zeros(NP, NKV, ps, HD)
    return q, k, k.clone(), pool, pool.clone()


def _codes(ps=PS):
    c = torch.zeros(NP, NKV, ps, HD // 2, dtype=torch.uint8)
    m = torch.zeros(NP, NKV, ps, 2)
    return c, c.clone(), m, m.clone()


def _table(**kw):
    return torch.zeros(BS, MP, dtype=torch.int32, **kw)


def _calls(lens, table, past=0, mask=None, ps=PS, L=TQ):
    """The five ops on CPU tensors with the given paged arguments, as (name, thunk)."""
    q, k, v, kp, vp = _step(ps)
    return [
        ("kv_append", lambda: ops.kv_append(k, v, kp, vp, past, lengths=lens, page_table=table)),
        ("kv_append_quant", lambda: ops.kv_append_quant(k, v, 4, F32, k_cache=kp, v_cache=vp, past=past, lengths=lens,
                                                        page_table=table)),
        ("kv_append_codes", lambda: ops.kv_append_codes(k, v, F32, *_codes(ps), past=past, lengths=lens, page_table=table)),
        ("decode_attention", lambda: ops.decode_attention(q, kp, vp, L, 0.125, mask, lengths=lens, page_table=table)),
        ("decode_attention_codes", lambda: ops.decode_attention_codes(q, _codes(ps), L, 0.125, mask, lengths=lens,
                                                                      page_table=table)),
    ]


LENS = torch.zeros(BS, dtype=torch.int32)
BAD_TABLES = [torch.zeros(BS, MP, dtype=torch.int64), torch.zeros(BS, MP), torch.zeros(BS + 1, MP, dtype=torch.int32),
              torch.zeros(BS * MP, dtype=torch.int32), torch.zeros(BS, MP, 1, dtype=torch.int32),
              torch.zeros(BS, 0, dtype=torch.int32), [[0] * MP] * BS]


@pytest.mark.parametrize("table", BAD_TABLES)
def test_page_table_dtype_and_shape(table):
    for name, call in _calls(LENS, table):
        with pytest.raises(OQError, match=f"{name}: page_table must be an int32"):
            call()


def test_page_table_must_live_on_the_pools_device():
    for name, call in _calls(LENS, _table(device="meta")):
        with pytest.raises(OQError, match=f"{name}: page_table on meta, the pool on cpu"):
            call()


def test_page_table_needs_lengths_and_takes_no_past():
    for name, call in _calls(None, _table()):
        with pytest.raises(OQError, match=f"{name}: page_table needs lengths"):
            call()
    for name, call in _calls(LENS, _table(), past=3)[:3]:
        with pytest.raises(OQError, match=f"{name}: page_table excludes past = 3"):
            call()
    for bad in (torch.zeros(BS, dtype=torch.int64), torch.zeros(BS + 1, dtype=torch.int32)):
        for name, call in _calls(bad, _table()):
            with pytest.raises(OQError, match=f"{name}: lengths.*int32"):
                call()


def test_paged_decode_takes_no_mask_and_bounds_L():
    mask = torch.zeros(1, 1, TQ, MP * PS)
    for name, call in _calls(LENS, _table(), mask=mask, L=MP * PS)[3:]:
        with pytest.raises(OQError, match=f"{name}: page_table excludes a mask"):
            call()
    for L in (TQ - 1, MP * PS + 1):
        for name, call in _calls(LENS, _table(), L=L)[3:]:
            with pytest.raises(OQError, match=f"{name}: the bound L = {L}"):
                call()


@pytest.mark.parametrize("ps", [8, 24, 48, 256])
def test_pool_page_size_must_be_a_supported_one(ps):
    for name, call in _calls(LENS, _table(), ps=ps):
        with pytest.raises(OQError, match=f"{name}: pool.*page size of {ps}"):
            call()


def test_pool_shape_and_dtype():
    q, k, v, kp, vp = _step()
    t = _table()
    with pytest.raises(OQError, match="kv_append: pool"):
        ops.kv_append(k, v, kp, vp[:-1], 0, lengths=LENS, page_table=t)                 # v pool of another size
    with pytest.raises(OQError, match="kv_append: pool"):
        ops.kv_append(k, v, kp.double(), vp.double(), 0, lengths=LENS, page_table=t)
    with pytest.raises(OQError, match="decode_attention: pool"):
        ops.decode_attention(q, kp, vp.bfloat16(), TQ, 0.125, lengths=LENS, page_table=t)
    with pytest.raises(OQError, match="kv_append_quant: page_table needs the page pools"):
        ops.kv_append_quant(k, v, 4, F32, k_out=torch.empty_like(k), v_out=torch.empty_like(v), lengths=LENS, page_table=t)
    c = _codes()
    with pytest.raises(OQError, match="kv_append_codes: pool"):
        ops.kv_append_codes(k, v, F32, c[0], c[1], c[2], c[3][..., :1], lengths=LENS, page_table=t)
    with pytest.raises(OQError, match="decode_attention_codes: pool"):
        ops.decode_attention_codes(q, (c[0], c[1].to(torch.int8), c[2], c[3]), TQ, 0.125, lengths=LENS, page_table=t)
    # well-formed paged arguments pass every host check and reach the binding, which refuses CPU tensors
    for name, call in _calls(LENS, t):
        with pytest.raises(OQError, match="GPU tensors"):
            call()
