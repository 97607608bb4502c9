"""Host-side contract of kvcache.PackedKVCache (no GPU): CPU tensors are refused loudly (no CPU fallback), as are dtypes the
packed blocks do not compute in and impossible sizes."""
import pytest
import torch

from omniquant_amd import OQError
from omniquant_amd.kvcache import PackedKVCache


def test_cpu_cache_is_refused():
    with pytest.raises(OQError):
        PackedKVCache(1, 2, 64, torch.bfloat16, "cpu", capacity=8)
    with pytest.raises(OQError):
        PackedKVCache.from_tuple((torch.zeros(1, 2, 3, 64), torch.zeros(1, 2, 3, 64)), dtype=torch.bfloat16)


@pytest.mark.parametrize("args", [(1, 2, 64, torch.float16), (0, 2, 64, torch.bfloat16), (1, 0, 64, torch.float32),
                                  (1, 2, 0, torch.float32)])
def test_bad_arguments_are_refused(args):
    with pytest.raises(OQError):
        PackedKVCache(*args, "cuda:0", capacity=4)


def test_tuple_shapes_are_checked():
    with pytest.raises(OQError):
        PackedKVCache.from_tuple((torch.zeros(1, 2, 3, 64),))
    with pytest.raises(OQError):
        PackedKVCache.from_tuple((torch.zeros(1, 2, 3, 64), torch.zeros(1, 2, 4, 64)))
