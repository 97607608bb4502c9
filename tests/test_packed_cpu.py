"""Host-side contract of realquant.PackedLinear (no GPU): CPU tensors are refused loudly (no CPU fallback), a saved packed
state dict loads into PackedLinear.empty() with every AutoGPTQ key, shape and dtype, and act-order groupings are refused
when the buffers are set, not per call."""
import pytest
import torch

from omniquant_amd import OQError
from omniquant_amd.realquant import PackedLinear


def _packed(bits, group, inn, out, bias, seed=0):
    g = torch.Generator().manual_seed(seed)
    ng = inn // group
    return dict(qweight=torch.randint(-2 ** 31, 2 ** 31 - 1, (inn // 32 * bits, out), generator=g, dtype=torch.int64).to(torch.int32),
                qzeros=torch.randint(-2 ** 31, 2 ** 31 - 1, (ng, out // 32 * bits), generator=g, dtype=torch.int64).to(torch.int32),
                scales=(torch.rand(ng, out, generator=g) * 0.01).half(),
                g_idx=torch.arange(inn, dtype=torch.int32) // group,
                bias=(torch.randn(out, generator=g).half() if bias else None))


def test_cpu_input_is_refused():
    pl = PackedLinear(4, 64, 128, 64, _packed(4, 64, 128, 64, True))
    with pytest.raises(OQError):
        pl(torch.randn(3, 128))
    with pytest.raises(OQError):
        pl(torch.randn(3, 128).half())


@pytest.mark.parametrize("bits,group,bias", [(4, 64, True), (3, 128, False), (2, None, True), (8, 32, False)])
def test_empty_then_load_state_dict_round_trips(bits, group, bias):
    inn, out = 256, 96
    src = PackedLinear(bits, group, inn, out, _packed(bits, group or inn, inn, out, bias, seed=bits))
    sd = src.state_dict()
    assert set(sd) == ({"qweight", "qzeros", "scales", "g_idx", "bias"} if bias else {"qweight", "qzeros", "scales", "g_idx"})
    dst = PackedLinear.empty(bits, group, inn, out, bias, "cpu")
    dst.load_state_dict(sd)
    got = dst.state_dict()
    assert set(got) == set(sd)
    for k, v in sd.items():
        assert got[k].shape == v.shape and got[k].dtype == v.dtype, k
        assert torch.equal(got[k], v), k
    assert dst.bias is None if not bias else dst.bias is not None
    assert torch.equal(dst.dequantize(), src.dequantize())


def test_act_order_g_idx_is_refused():
    inn, out, group = 256, 64, 64
    p = _packed(4, group, inn, out, False)
    p["g_idx"] = p["g_idx"][torch.randperm(inn, generator=torch.Generator().manual_seed(1))].contiguous()
    with pytest.raises(OQError):
        PackedLinear(4, group, inn, out, p)
    dst = PackedLinear.empty(4, group, inn, out, False, "cpu")
    with pytest.raises(OQError):
        dst.load_state_dict({k: v for k, v in p.items() if v is not None})


@pytest.mark.parametrize("bits,group,inn,out", [(5, 64, 128, 64), (4, 48, 96, 64), (4, 64, 128, 48), (4, 100, 128, 64)])
def test_unsupported_layouts_are_refused(bits, group, inn, out):
    with pytest.raises(OQError):
        PackedLinear.empty(bits, group, inn, out, False, "cpu")


#: (in, out) -> splits of the contraction in oq_packed_gemv (float) and oq_packed_gemv_a4 (integer).  The float GEMV's split
#: count fixes its summation order, hence its bits: the plan is part of the value contract.
_SPLIT_PLANS = [(96, 160, 3, 3), (416, 96, 13, 13), (256, 288, 8, 8), (4096, 4096, 32, 32), (4096, 11008, 12, 12),
                (11008, 4096, 32, 32), (8192, 1024, 128, 128), (4096, 32000, 8, 5)]


@pytest.mark.parametrize("inn,out,fsplits,isplits", _SPLIT_PLANS)
def test_gemv_split_plans_are_pinned(inn, out, fsplits, isplits):
    """The exported workspace sizes (no GPU needed) pin the split plans: splits * M * out * 4 bytes of fp32 partials for the
    float GEMV, splits * (M + 1) * out * 4 bytes of int32 partials (row M: the column code sums) for the integer one."""
    from omniquant_amd import _capi
    for M in (1, 16):
        assert _capi.size_call("oq_packed_gemv_workspace", M, inn, out, 4) == fsplits * M * out * 4
        assert _capi.size_call("oq_packed_gemv_a4_workspace", M, inn, out) == isplits * (M + 1) * out * 4


def test_gemv_split_plan_example_sizes():
    from omniquant_amd import _capi
    assert _capi.size_call("oq_packed_gemv_workspace", 16, 4096, 4096, 4) == 8388608
    assert _capi.size_call("oq_packed_gemv_a4_workspace", 16, 4096, 4096) == 8912896
