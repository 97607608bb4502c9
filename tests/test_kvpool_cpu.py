"""Host-side checks of the model-wide paged KV pool that need no GPU: kvcache.PagedKVPool refuses a CPU device and the
constructor arguments PagedKVCache refuses, and the three page-move ops (ops.kv_pages_gather / kv_pages_scatter / kv_pages_copy)
validate the ids, the pool and the contiguous buffer on the host before any device call (every message below comes from those
checks, not from the CPU-tensor refusal of the C binding); the C entry points' own refusals and their empty moves return before
any launch and are called directly.  The new symbols' export, declaration and binding are test_capi_symbols.py's, unchanged."""
import pytest
import torch

from omniquant_amd import OQError, _capi, ops
from omniquant_amd.kvcache import PagedKVCache, PagedKVPool, SwappedSequence

LAYERS, NP, NKV, PS, HD, N = 3, 5, 2, 16, 64, 4
BF16 = torch.bfloat16


# ---- PagedKVPool ----------------------------------------------------------------------------------------------------------
def test_pool_refuses_a_cpu_device():
    for kw in (dict(), dict(code_bits=4), dict(code_bits=8, page_size=128, max_pages=2), dict(swap_staging_bytes=1 << 20)):
        with pytest.raises(OQError, match="PagedKVPool needs a GPU device"):
            PagedKVPool(LAYERS, 3, NKV, HD, BF16, "cpu", NP, **kw)


BAD_ARGS = [
    (dict(dtype=torch.float16), "dtype"),
    (dict(bs=0), "bs 0"),
    (dict(nkv=0), "nkv 0"),
    (dict(num_pages=0), "num_pages 0"),
    (dict(max_pages=0), "max_pages 0"),
    (dict(page_size=8), "page_size 8"),
    (dict(page_size=48), "page_size 48"),
    (dict(hd=96), "head_dim 96"),
    (dict(code_bits=3), "code_bits 3"),
]


@pytest.mark.parametrize("change,match", BAD_ARGS)
def test_pool_refuses_what_the_per_layer_cache_refuses(change, match):
    """The same argument, the same reason, under the pool's own name (an indexed GPU device is not touched before the
    arguments have passed)."""
    args = dict(bs=3, nkv=NKV, hd=HD, dtype=BF16, device="cuda:0", num_pages=NP, page_size=PS, max_pages=None, code_bits=None)
    args.update(change)
    seen = []
    for make in (lambda: PagedKVCache(**args), lambda: PagedKVPool(LAYERS, **args)):
        with pytest.raises(OQError, match=match) as e:
            make()
        seen.append(str(e.value))
    assert seen[0].startswith("PagedKVCache") and seen[1].startswith("PagedKVPool")
    assert seen[0].split(":", 1)[1] == seen[1].split(":", 1)[1]


def test_pool_refuses_bad_layers():
    for layers in (0, -1):
        with pytest.raises(OQError, match=f"PagedKVPool: layers {layers}"):
            PagedKVPool(layers, 3, NKV, HD, BF16, "cuda:0", NP)
    with pytest.raises(TypeError):
        PagedKVPool(1.5, 3, NKV, HD, BF16, "cuda:0", NP)


def test_swapped_sequence_surface():
    bufs = {"k": torch.zeros(LAYERS, 2, 4096, dtype=torch.uint8), "v": torch.zeros(LAYERS, 2, 4096, dtype=torch.uint8)}
    h = SwappedSequence(20, 2, (LAYERS, NKV, HD, PS, BF16, None), bufs, None, None)
    assert h.nbytes == 2 * LAYERS * 2 * 4096 and h.length == 20 and h.n_pages == 2
    assert "length=20" in repr(h) and "n_pages=2" in repr(h)


def test_the_new_symbols_are_bound():
    for name in ("oq_kv_pages_gather", "oq_kv_pages_scatter", "oq_kv_pages_copy"):
        assert len(_capi.SIGNATURES[name]) == 9
        assert hasattr(_capi.load(), name)


# ---- the page-move ops ------------------------------------------------------------------------------------------------------
def _pool(tail=(NKV, PS, HD), dtype=BF16):
    return torch.zeros((LAYERS, NP) + tuple(tail), dtype=dtype)


def _ids(n=N, **kw):
    return torch.zeros(n, dtype=torch.int32, **kw)


def _flat(pool, n=N):
    return torch.zeros(pool.shape[0], n, pool[0, 0].numel() * pool.element_size(), dtype=torch.uint8)


def _calls(pool, ids, flat=None, ids2=None):
    """The three ops on CPU tensors, as (name, the argument's name, thunk)."""
    flat = _flat(pool, N) if flat is None else flat
    ids2 = ids if ids2 is None else ids2
    return [("kv_pages_gather", "page_ids", lambda: ops.kv_pages_gather(pool, ids, flat)),
            ("kv_pages_scatter", "page_ids", lambda: ops.kv_pages_scatter(flat, pool, ids)),
            ("kv_pages_copy", "src_ids", lambda: ops.kv_pages_copy(pool, ids, ids2))]


BAD_IDS = [torch.zeros(N, dtype=torch.int64), torch.zeros(N), torch.zeros(N, 1, dtype=torch.int32),
           torch.zeros((), dtype=torch.int32), [0] * N, None]


@pytest.mark.parametrize("ids", BAD_IDS)
def test_ids_dtype_and_shape(ids):
    for name, arg, call in _calls(_pool(), ids):
        with pytest.raises(OQError, match=f"{name}: {arg} must be an int32 1-D device tensor"):
            call()
    with pytest.raises(OQError, match="kv_pages_copy: dst_ids must be an int32 1-D device tensor"):
        ops.kv_pages_copy(_pool(), _ids(), ids)


def test_ids_must_live_on_the_pools_device_and_pair_up():
    for name, arg, call in _calls(_pool(), _ids(device="meta")):
        with pytest.raises(OQError, match=f"{name}: {arg} on meta, the pool on cpu"):
            call()
    with pytest.raises(OQError, match="kv_pages_copy: dst_ids on meta, the pool on cpu"):
        ops.kv_pages_copy(_pool(), _ids(), _ids(device="meta"))
    with pytest.raises(OQError, match="kv_pages_copy: dst_ids names 3 pages, src_ids 4"):
        ops.kv_pages_copy(_pool(), _ids(), _ids(3))


def test_page_bytes_must_be_a_multiple_of_16():
    for tail, dtype, nbytes in (((1, 3, 2), torch.float32, 24), ((1, 8, 9), torch.uint8, 72), ((5,), BF16, 10)):
        pool = _pool(tail, dtype)
        for name, _, call in _calls(pool, _ids()):
            with pytest.raises(OQError, match=f"{name}: pool.*pages of {nbytes} bytes"):
                call()
    for bad in (torch.zeros(LAYERS, NP), torch.zeros(LAYERS * NP * 64), None):
        with pytest.raises(OQError, match=r"kv_pages_gather: pool must be a \[layers, num_pages, ...\] tensor"):
            ops.kv_pages_gather(bad, _ids())


def test_pool_must_be_contiguous():
    big = torch.zeros(LAYERS, 2 * NP, NKV, PS, HD, dtype=BF16)
    for pool in (big[:, ::2], big[:, :NP], big.transpose(2, 3)):
        for name, _, call in _calls(pool, _ids()):
            with pytest.raises(OQError, match=f"{name}: pool.*is not contiguous"):
                call()


def test_flat_buffer_size_and_device():
    pool = _pool()
    pb = NKV * PS * HD * 2
    for bad in (_flat(pool, N - 1), _flat(pool, N + 1), torch.zeros(LAYERS * N * pb - 16, dtype=torch.uint8),
                _flat(pool, 2 * N)[:, ::2], "dst"):
        with pytest.raises(OQError, match=f"kv_pages_gather: dst .*expected {LAYERS * N * pb} contiguous bytes"):
            ops.kv_pages_gather(pool, _ids(), bad)
        with pytest.raises(OQError, match=f"kv_pages_scatter: src .*expected {LAYERS * N * pb} contiguous bytes"):
            ops.kv_pages_scatter(bad, pool, _ids())
    meta = torch.zeros(LAYERS, N, pb, dtype=torch.uint8, device="meta")
    with pytest.raises(OQError, match="kv_pages_gather: dst on meta, the pool on cpu"):
        ops.kv_pages_gather(pool, _ids(), meta)
    with pytest.raises(OQError, match="kv_pages_scatter: src on meta, the pool on cpu"):
        ops.kv_pages_scatter(meta, pool, _ids())


def test_well_formed_arguments_reach_the_binding():
    """Every host check passes -- a layer range of the pool, a 1-D byte buffer of the right size, a meta page of 256 bytes -- and
    the binding refuses the CPU tensors."""
    for pool in (_pool(), _pool()[1:3], _pool((NKV, PS, 2), torch.float32)):
        pb = pool[0, 0].numel() * pool.element_size()
        for flat in (_flat(pool), torch.zeros(pool.shape[0] * N * pb, dtype=torch.uint8)):
            for name, _, call in _calls(pool, _ids(), flat):
                with pytest.raises(OQError, match="GPU tensors"):
                    call()


# ---- the C entry points' own argument checks (nothing is launched, so no GPU is needed) -----------------------------------------
def _c(name, *args):
    return getattr(_capi.load(), name)(*args), _capi.load().oq_last_error().decode()


def test_c_entry_points_refuse_bad_arguments_and_accept_empty_moves():
    p = 0x1000                       # a non-null, 16-byte aligned address that is never dereferenced: every call returns first
    # n == 0 or layers == 0: success without a launch, null pointers and all
    assert _c("oq_kv_pages_gather", None, 8, 256, 2048, 3, None, 0, None, None)[0] == 0
    assert _c("oq_kv_pages_gather", None, 8, 256, 2048, 0, None, 5, None, None)[0] == 0
    assert _c("oq_kv_pages_scatter", None, None, 8, 256, 2048, 3, None, 0, None)[0] == 0
    assert _c("oq_kv_pages_copy", None, 8, 256, 2048, 0, None, None, 5, None)[0] == 0
    for pb in (0, 8, 24, 250, 65537):
        rc, msg = _c("oq_kv_pages_gather", p, 8, pb, 8 * 256, 3, p, 4, p, None)
        assert rc != 0 and "oq_kv_pages_gather: page_bytes" in msg, (pb, msg)
        rc, msg = _c("oq_kv_pages_copy", p, 8, pb, 8 * 256, 3, p, p, 0, None)          # refused even when nothing would move
        assert rc != 0 and "oq_kv_pages_copy: page_bytes" in msg, (pb, msg)
    for args in ((p, -1, 256, 2048, 3, p, 4, p, None), (p, 8, -256, 2048, 3, p, 4, p, None), (p, 8, 256, -2048, 3, p, 4, p, None),
                 (p, 8, 256, 2048, -3, p, 4, p, None), (p, 8, 256, 2048, 3, p, -4, p, None)):
        rc, msg = _c("oq_kv_pages_gather", *args)
        assert rc != 0 and "negative size" in msg, (args, msg)
    for args in ((None, 8, 256, 2048, 3, p, 4, p, None), (p, 8, 256, 2048, 3, None, 4, p, None), (p, 8, 256, 2048, 3, p, 4, None, None)):
        rc, msg = _c("oq_kv_pages_gather", *args)
        assert rc != 0 and "null pointer with n = 4" in msg, (args, msg)
    rc, msg = _c("oq_kv_pages_scatter", None, p, 8, 256, 2048, 3, p, 4, None)
    assert rc != 0 and "oq_kv_pages_scatter: null pointer" in msg
    rc, msg = _c("oq_kv_pages_copy", p, 8, 256, 2048, 3, p, None, 4, None)
    assert rc != 0 and "oq_kv_pages_copy: null pointer" in msg
    # a layer stride below one layer's pages, misaligned pointers
    rc, msg = _c("oq_kv_pages_gather", p, 8, 256, 2047, 3, p, 4, p, None)
    assert rc != 0 and "layer_stride_bytes" in msg
    rc, msg = _c("oq_kv_pages_gather", p, 8, 256, 1024, 3, p, 4, p, None)
    assert rc != 0 and "layer_stride_bytes" in msg
    rc, msg = _c("oq_kv_pages_gather", p + 8, 8, 256, 2048, 3, p, 4, p, None)
    assert rc != 0 and "16-byte aligned" in msg
    rc, msg = _c("oq_kv_pages_gather", p, 8, 256, 2048, 3, p + 2, 4, p, None)
    assert rc != 0 and "page ids" in msg
