"""Host-side checks of the ragged KV cache (per-sequence lengths on the device) that need no GPU: the cache still refuses a
CPU device, and the `lengths` keywords of the ops validate dtype, shape, device and the excluded arguments on the host, before
any device call (every message below comes from those checks, not from the CPU-tensor refusal of the C binding)."""
import pytest
import torch

from omniquant_amd import OQError, ops
from omniquant_amd.kvcache import PackedKVCache

BS, TQ, NH, NKV, HD, CAP = 3, 2, 4, 2, 64, 16


def _step(dtype=torch.float32):
    q = torch.zeros(BS, TQ, NH, HD, dtype=dtype)
    k = torch.zeros(BS, TQ, NKV, HD, dtype=dtype)
    kc = torch.zeros(BS, NKV, CAP, HD, dtype=dtype)
    return q, k, k.clone(), kc, kc.clone()


def _codes():
    c = torch.zeros(BS, NKV, CAP, HD // 2, dtype=torch.uint8)
    m = torch.zeros(BS, NKV, CAP, 2)
    return c, c.clone(), m, m.clone()


def test_constructor_still_refuses_a_cpu_device():
    for kw in (dict(ragged=True), dict(ragged=True, code_bits=4), dict()):
        with pytest.raises(OQError, match="GPU device"):
            PackedKVCache(BS, NKV, HD, torch.bfloat16, "cpu", CAP, **kw)


def test_from_tuple_refuses_ragged():
    kv = (torch.zeros(1, NKV, 4, HD), torch.zeros(1, NKV, 4, HD))
    with pytest.raises(OQError, match="ragged"):
        PackedKVCache.from_tuple(kv, ragged=True)


BAD_LENGTHS = [(torch.zeros(BS, dtype=torch.int64), "int32"), (torch.zeros(BS + 1, dtype=torch.int32), "int32"),
               (torch.zeros(BS, 1, dtype=torch.int32), "int32"), ([0] * BS, "int32"), (torch.zeros(BS), "int32")]


@pytest.mark.parametrize("lengths,msg", BAD_LENGTHS)
def test_append_lengths_dtype_and_shape(lengths, msg):
    q, k, v, kc, vc = _step()
    with pytest.raises(OQError, match=f"kv_append: lengths.*{msg}"):
        ops.kv_append(k, v, kc, vc, 0, lengths=lengths)
    with pytest.raises(OQError, match=f"kv_append_quant: lengths.*{msg}"):
        ops.kv_append_quant(k, v, 4, torch.float32, k_cache=kc, v_cache=vc, lengths=lengths)
    with pytest.raises(OQError, match=f"kv_append_codes: lengths.*{msg}"):
        ops.kv_append_codes(k, v, torch.float32, *_codes(), lengths=lengths)


def test_append_lengths_exclude_a_past_and_need_a_cache():
    q, k, v, kc, vc = _step()
    lens = torch.zeros(BS, dtype=torch.int32)
    with pytest.raises(OQError, match="excludes past = 3"):
        ops.kv_append(k, v, kc, vc, 3, lengths=lens)
    with pytest.raises(OQError, match="excludes past = 1"):
        ops.kv_append_quant(k, v, 4, torch.float32, k_cache=kc, v_cache=vc, past=1, lengths=lens)
    with pytest.raises(OQError, match="excludes past = 2"):
        ops.kv_append_codes(k, v, torch.float32, *_codes(), past=2, lengths=lens)
    with pytest.raises(OQError, match="lengths without a cache"):
        ops.kv_append_quant(k, v, 4, torch.float32, k_out=torch.empty_like(k), v_out=torch.empty_like(v), lengths=lens)


def test_lengths_must_live_on_the_caches_device():
    q, k, v, kc, vc = _step()
    meta = torch.zeros(BS, dtype=torch.int32, device="meta")
    with pytest.raises(OQError, match="lengths on meta, the cache on cpu"):
        ops.kv_append(k, v, kc, vc, 0, lengths=meta)
    with pytest.raises(OQError, match="lengths on meta, the cache on cpu"):
        ops.decode_attention(q, kc, vc, CAP, 0.125, lengths=meta)
    with pytest.raises(OQError, match="lengths on meta, the cache on cpu"):
        ops.decode_attention_codes(q, _codes(), CAP, 0.125, lengths=meta)


def test_decode_lengths_exclude_a_mask_and_bound_the_capacity():
    q, k, v, kc, vc = _step()
    lens = torch.zeros(BS, dtype=torch.int32)
    mask = torch.zeros(1, 1, TQ, CAP)
    for fn, cache in ((ops.decode_attention, (kc, vc)), (ops.decode_attention_codes, (_codes(),))):
        name = fn.__name__
        with pytest.raises(OQError, match=f"{name}: lengths excludes a mask"):
            fn(q, *cache, CAP, 0.125, mask, lengths=lens)
        with pytest.raises(OQError, match=f"{name}: the bound L = {CAP + 1}"):
            fn(q, *cache, CAP + 1, 0.125, lengths=lens)
        with pytest.raises(OQError, match=f"{name}: the bound L = {TQ - 1}"):
            fn(q, *cache, TQ - 1, 0.125, lengths=lens)
        for bad, msg in BAD_LENGTHS:
            with pytest.raises(OQError, match=f"{name}: lengths.*{msg}"):
                fn(q, *cache, CAP, 0.125, lengths=bad)
