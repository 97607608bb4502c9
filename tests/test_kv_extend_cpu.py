"""Host side of the chunked-prefill attention (ops.extend_attention*): no GPU needed."""
import pytest
import torch

from omniquant_amd import OQError, block_common, ops


def test_cpu_tensors_are_refused():
    bs, Tq, nh, nkv, hd, L = 2, 16, 4, 2, 64, 48
    q = torch.zeros(bs, Tq, nh, hd, dtype=torch.bfloat16)
    kc = torch.zeros(bs, nkv, L, hd, dtype=torch.bfloat16)
    lens = torch.zeros(bs, dtype=torch.int32)
    with pytest.raises(OQError, match="CPU tensor"):
        ops.extend_attention(q, kc, kc.clone(), L, 0.125, lens)
    codes = torch.zeros(bs, nkv, L, hd // 2, dtype=torch.uint8)
    meta = torch.zeros(bs, nkv, L, 2)
    with pytest.raises(OQError, match="CPU tensor"):
        ops.extend_attention_codes(q, (codes, codes.clone(), meta, meta.clone()), L, 0.125, lens)
    with pytest.raises(OQError, match="lengths"):
        ops.extend_attention(q, kc, kc.clone(), L, 0.125, None)
    with pytest.raises(OQError, match="lengths"):
        ops.extend_attention(q, kc, kc.clone(), L, 0.125, lens.long())


def test_the_routing_threshold_never_drops_below_16():
    assert isinstance(block_common.EXTEND_MIN_TQ, int) and block_common.EXTEND_MIN_TQ >= 16


def test_support_and_workspace_depend_on_shapes_only():
    from omniquant_amd import _capi as C
    assert ops.extend_attention_supported(torch.bfloat16, 16, 64) and ops.extend_attention_supported(torch.bfloat16, 1024, 128)
    assert not ops.extend_attention_supported(torch.float32, 32, 128)
    assert not ops.extend_attention_supported(torch.float16, 32, 128)
    assert not ops.extend_attention_supported(torch.bfloat16, 32, 96)
    # one split (a chip's worth of query tiles): no workspace; a short chunk over a long past: partials for several splits
    assert C.size_call("oq_attn_extend_workspace", 8, 32, 32, 1024, 2048 + 1024, 128) == 0
    rows = 1 * 64 * 16
    n = C.size_call("oq_attn_extend_workspace", 1, 64, 8, 16, 8192 + 16, 128)
    assert n > 0 and n % (rows * 130 * 4) == 0 and 2 <= n // (rows * 130 * 4) <= 64
