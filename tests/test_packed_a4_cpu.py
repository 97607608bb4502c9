"""Host-only eligibility of the W4A4 packed path (realquant.check_act_quant_eligible / pack_block(..., act_quant=True)):
refused configurations raise OQError naming the offending module, before any buffer is packed."""
import pytest

from omniquant_amd import OQError
from omniquant_amd.calibrate import decoder_layer_class, default_args
from omniquant_amd.realquant import PackedLinear, check_act_quant_eligible, pack_block
from omniquant_amd.synthetic import make_config, make_layer


def _block(family="llama", **kw):
    a = dict(wbits=4, abits=4, group_size=None, lwc=True, let=False)
    a.update(kw)
    args = default_args(net=family, **a)
    heads = 2 if family == "llama" else 4
    cfg = make_config(None, family=family, hidden_size=256, inter=512, heads=heads, kv_heads=heads)
    return decoder_layer_class(family)(cfg, make_layer(cfg, seed=0, device="cpu"), args), args


def test_w4a4_llama_block_is_eligible():
    blk, args = _block()
    check_act_quant_eligible(blk, 4)
    assert args.real_quant_act is False           # the calibration driver's opt-in defaults to off


@pytest.mark.parametrize("kw,match", [(dict(wbits=3), "3-bit weights"), (dict(group_size=64), "grouped weights"),
                                      (dict(abits=8), "8-bit"), (dict(abits=16), "16-bit")])
def test_refused_configurations_name_the_reason(kw, match):
    blk, args = _block(**kw)
    with pytest.raises(OQError, match=match):
        pack_block(blk, args.wbits, act_quant=True)
    assert not any(isinstance(m, PackedLinear) for m in blk.modules())      # refused before anything was packed


@pytest.mark.parametrize("attr,value,match", [("symmetric", True, "symmetric"), ("lwc", True, "LWC"),
                                              ("metric", "fix0to1", "fix0to1"), ("dynamic_method", "per_channel", "per_channel"),
                                              ("group_size", 64, "group")])
def test_refused_activation_quantisers(attr, value, match):
    for path in ("mlp.down_proj.act_quantizer", "self_attn.qkt_matmul.x2_quantizer"):
        blk, _ = _block()
        q = blk.get_submodule(path)
        setattr(q, attr, value)
        with pytest.raises(OQError, match=path.replace(".", r"\.")):
            check_act_quant_eligible(blk, 4)
        with pytest.raises(OQError, match=match):
            check_act_quant_eligible(blk, 4)


def test_probability_quantiser_must_stay_16_bit():
    blk, _ = _block()
    blk.self_attn.pv_matmul.x1_quantizer.n_bits = 8
    with pytest.raises(OQError, match=r"pv_matmul\.x1_quantizer"):
        check_act_quant_eligible(blk, 4)


def test_opt_is_refused():
    blk, _ = _block("opt")
    with pytest.raises(OQError, match="not a LLaMA block"):
        pack_block(blk, 4, act_quant=True)


def test_act_bits_4_needs_4bit_per_channel_linears():
    with pytest.raises(OQError):
        PackedLinear.empty(4, 64, 256, 64, False, "cpu", act_bits=4)
    with pytest.raises(OQError):
        PackedLinear.empty(3, None, 256, 64, False, "cpu", act_bits=4)
    with pytest.raises(OQError):
        PackedLinear.empty(4, None, 256, 64, False, "cpu", act_bits=8)
    assert PackedLinear.empty(4, None, 256, 64, False, "cpu", act_bits=4).act_bits == 4
    assert PackedLinear.empty(4, None, 256, 64, False, "cpu").act_bits == 16
