"""CPU pins of the 4-bit KV-code layout and of the dequantisation expression (omniquant_amd.kvcache.unpack_codes, the pure-torch
value contract PackedKVCache.dequantize() applies to its GPU buffers).  The class itself refuses a CPU device."""
import pytest
import torch

from omniquant_amd import OQError
from omniquant_amd.kvcache import PackedKVCache, unpack_codes


def test_nibble_layout():
    hd = 64
    codes = (torch.arange(hd) * 7 + 3) % 16                       # dim d -> code
    packed = (codes[0::2] | (codes[1::2] << 4)).to(torch.uint8)   # byte i: dim 2i low nibble, dim 2i + 1 high nibble
    meta = torch.tensor([1.0, 0.0])
    assert torch.equal(unpack_codes(packed, meta), codes.float())
    # the same bytes as little-endian 32-bit words: dim d is nibble d % 8 of word d // 8
    words = packed.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    for d in range(hd):
        assert int((words[d // 8] >> (4 * (d % 8))) & 0xF) == int(codes[d])
    one = torch.tensor([0x0F], dtype=torch.uint8)
    assert unpack_codes(one, meta).tolist() == [15.0, 0.0]
    assert unpack_codes(torch.tensor([0xF0], dtype=torch.uint8), meta).tolist() == [0.0, 15.0]


def test_dequantisation_expression():
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 256, (2, 3, 5, 32), generator=g, dtype=torch.int64).to(torch.uint8)
    scale = torch.rand(2, 3, 5, 1, generator=g) * 0.3 + 1e-3
    zp = torch.randint(-40, 40, (2, 3, 5, 1), generator=g).float()          # not confined to 0..15
    zp[0, 0, 0] = 1e4
    out = unpack_codes(codes, torch.cat([scale, zp], dim=-1))
    assert out.dtype == torch.float32 and out.shape == (2, 3, 5, 64)
    c = torch.stack([codes & 0xF, codes >> 4], dim=-1).reshape(2, 3, 5, 64)
    # one exact subtraction and one float32 multiply: equal to the float64 product rounded once
    ref = ((c.double() - zp.double()) * scale.double()).float()
    assert torch.equal(out, ref)
    # a NaN scale over codes 0 is a NaN row (how a degenerate head row is stored); a zero scale is a zero row
    assert bool(torch.isnan(unpack_codes(torch.zeros(4, dtype=torch.uint8), torch.tensor([float("nan"), 3.0]))).all())
    assert unpack_codes(codes[0, 0, 0], torch.tensor([0.0, 3.0])).abs().max() == 0


def test_class_refuses_a_cpu_device():
    with pytest.raises(OQError, match="GPU"):
        PackedKVCache(1, 2, 64, torch.float32, "cpu", 4, code_bits=4)
    with pytest.raises(OQError, match="GPU"):
        PackedKVCache(1, 2, 64, torch.float32, "cpu", 4)
