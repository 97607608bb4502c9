"""The 8-bit code KV cache of the weight-only packed blocks, the parts that need no GPU: the value contract
(kvcache.unpack_codes(..., bits=8)), the quantiser's restatement against oracle.ref_cpu.fake_quant, and the refusals."""
import pytest
import torch

from omniquant_amd import OQError
from omniquant_amd.kvcache import PackedKVCache, PagedKVCache, unpack_codes
from omniquant_amd.realquant import _check_kv_cache_bits
from oracle import ref_cpu

F32 = torch.float32


def quant8(x):
    """The 8-bit code cache's quantiser in plain float32 torch, over the last dim: the asymmetric dynamic quantiser of
    quantize/quantizer.py:122-147 with 255 levels, the row range first widened to contain zero.  Returns (codes uint8 [..., hd],
    meta float32 [..., 2] = (scale, zero-point)).  A row of scale 0 (all zeros): codes 0, meta (0, 0); a row whose scale is not
    finite (a NaN or infinite element, an overflowing range): codes 0 under a NaN scale (its zero-point is unspecified)."""
    x = x.to(F32)
    lo = x.amin(dim=-1, keepdim=True).clamp(max=0.0)
    hi = x.amax(dim=-1, keepdim=True).clamp(min=0.0)
    scale = (hi - lo) / 255.0
    zp = (-lo / scale).clamp(min=-1e4, max=1e4).round()
    q = (torch.round(x / scale) + zp).clamp(0, 255)
    zero, bad = scale == 0, ~torch.isfinite(scale)
    codes = torch.where(zero | bad, torch.zeros_like(q), q).to(torch.uint8)
    scale = torch.where(bad, torch.full_like(scale, float("nan")), scale)
    zp = torch.where(zero | bad, torch.zeros_like(zp), zp)
    return codes, torch.cat((scale, zp), dim=-1)


def test_unpack_codes_8bit_layout_and_expression():
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 256, (2, 3, 5, 64), generator=g, dtype=torch.uint8)
    meta = torch.rand(2, 3, 5, 2, generator=g) + 0.5
    meta[..., 1] = torch.randint(0, 256, (2, 3, 5), generator=g).float()
    meta[1, 2, 4, 0] = float("nan")
    got = unpack_codes(codes, meta, bits=8)
    assert got.dtype == F32 and got.shape == (2, 3, 5, 64)
    for d in (0, 1, 31, 63):                                    # byte d holds dim d
        want = (codes[..., d].float() - meta[..., 1]) * meta[..., 0]
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got[..., d]), nan) and torch.equal(got[..., d][~nan], want[~nan])
    assert bool(torch.isnan(got[1, 2, 4]).all()) and int(torch.isnan(got).sum()) == 64
    # calls without bits, and bits=4, are the nibble layout as before
    c4 = codes[..., :32]
    want4 = (torch.stack((c4 & 0xF, c4 >> 4), dim=-1).reshape(2, 3, 5, 64).float() - meta[..., 1:2]) * meta[..., 0:1]
    for got4 in (unpack_codes(c4, meta), unpack_codes(c4, meta, bits=4)):
        nan = torch.isnan(want4)
        assert torch.equal(torch.isnan(got4), nan) and torch.equal(got4[~nan], want4[~nan])
    with pytest.raises(OQError, match="bits"):
        unpack_codes(codes, meta, bits=3)


@pytest.mark.parametrize("hd", [64, 128])
def test_restated_quantiser_equals_the_oracle_on_rows_that_straddle_zero(hd):
    g = torch.Generator().manual_seed(hd)
    x = torch.randn(257, hd, generator=g) * torch.logspace(-3, 3, 257)[:, None]
    x[:, 0], x[:, 1] = -x[:, 0].abs() - 1e-6, x[:, 1].abs() + 1e-6         # lo < 0 < hi in every row
    codes, meta = quant8(x)
    y, scale, zp = ref_cpu.fake_quant(x, 8, return_qparams=True)
    assert torch.equal(meta[:, 0:1], scale) and torch.equal(meta[:, 1:2], zp)
    assert torch.equal(unpack_codes(codes, meta, bits=8).view(torch.int32), y.view(torch.int32))
    assert bool((meta[:, 1] >= 0).all()) and bool((meta[:, 1] <= 255).all())


def test_restated_quantiser_special_rows():
    hd = 64
    x = torch.randn(7, hd, generator=torch.Generator().manual_seed(1))
    x[0] = x[0].abs() + 6.0                     # all positive: the range starts at 0
    x[1] = -x[1].abs() - 6.0                    # all negative: it ends at 0
    x[2] = 1.75                                 # constant
    x[3] = 0.0
    x[4, 5] = float("nan")
    x[5, 7] = float("inf")
    x[6, 0], x[6, 1] = 3e38, -3e38              # the range overflows
    codes, meta = quant8(x)
    y = unpack_codes(codes, meta, bits=8)
    assert float(meta[0, 1]) == 0.0 and float(meta[1, 1]) == 255.0 and float(meta[2, 1]) == 0.0
    assert bool((codes[2] == 255).all()) and torch.equal(y[2], x[2])
    for r in (0, 1):                            # within half a grid step
        assert float((y[r] - x[r]).abs().max()) <= 0.5 * float(meta[r, 0]) * (1 + 1e-6)
    assert bool((codes[3] == 0).all()) and meta[3].tolist() == [0.0, 0.0] and bool((y[3] == 0).all())
    for r in (4, 5, 6):
        assert bool((codes[r] == 0).all()) and bool(torch.isnan(meta[r, 0])) and bool(torch.isnan(y[r]).all())
    assert not bool(torch.isnan(y[:4]).any())


def test_check_kv_cache_bits():
    _check_kv_cache_bits(None, False)
    _check_kv_cache_bits(None, True)
    _check_kv_cache_bits(4, True)
    _check_kv_cache_bits(8, False)
    with pytest.raises(OQError, match="kv_cache_bits"):
        _check_kv_cache_bits(8, True)
    with pytest.raises(OQError, match="act_quant"):
        _check_kv_cache_bits(4, False)
    with pytest.raises(OQError, match="kv_cache_bits"):
        _check_kv_cache_bits(3, False)


def test_cpu_device_is_refused():
    with pytest.raises(OQError, match="GPU"):
        PackedKVCache(1, 2, 64, F32, "cpu", 4, code_bits=8)
    with pytest.raises(OQError, match="GPU"):
        PagedKVCache(1, 2, 64, F32, "cpu", 4, code_bits=8)
    raw = tuple(torch.randn(1, 2, 4, 64) for _ in range(2))
    with pytest.raises(OQError, match="GPU"):
        PackedKVCache.from_tuple(raw, code_bits=8)
