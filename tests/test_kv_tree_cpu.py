"""Host side of tree attention for speculative decoding: kvcache.TokenTree (depths, ancestor sets, paths, refusals, the
tensors it uploads) and the loud refusal of CPU tensors by ops.tree_attention / ops.kv_tree_commit.  No GPU needed."""
import pytest
import torch

from omniquant_amd import OQError, ops
from omniquant_amd.kvcache import TokenTree


def _bits(*nodes):
    return sum(1 << n for n in nodes)


def test_chain():
    t = TokenTree([-1, 0, 1, 2, 3])
    assert (t.Tq, t.bs, t.height) == (5, None, 5)
    assert t.depth == [0, 1, 2, 3, 4]
    assert t.ancestors == [_bits(*range(n + 1)) for n in range(5)]
    assert t.path(3) == [0, 1, 2, 3] and t.path(0) == [0]


def test_star():
    t = TokenTree([-1, 0, 0, 0, 0])
    assert t.height == 2 and t.depth == [0, 1, 1, 1, 1]
    assert t.ancestors == [_bits(0)] + [_bits(0, n) for n in range(1, 5)]
    assert t.path(4) == [0, 4]
    assert t.is_root_path([]) and t.is_root_path([0, 3]) and not t.is_root_path([3]) and not t.is_root_path([0, 3, 4])


def test_two_level_branching_tree():
    parents = [-1] + [(n - 1) // 3 for n in range(1, 13)]            # 0 -> 1, 2, 3 -> three children each
    t = TokenTree(parents)
    assert t.height == 3 and t.depth == [0] + [1] * 3 + [2] * 9
    assert t.ancestors[7] == _bits(0, 2, 7) and t.path(7) == [0, 2, 7]
    assert t.ancestors[12] == _bits(0, 3, 12) and t.path(12) == [0, 3, 12]
    for n, a in enumerate(t.ancestors):
        assert a >> (n + 1) == 0 and a >> n & 1                     # only bits <= n, the node's own among them
    assert t.is_root_path([0, 2, 7]) and not t.is_root_path([0, 1, 7]) and not t.is_root_path([2, 7])


def test_forest():
    t = TokenTree([-1, -1, 0, 1, 1, -1, 5, 6])
    assert t.depth == [0, 0, 1, 1, 1, 0, 1, 2] and t.height == 3
    assert t.ancestors == [_bits(0), _bits(1), _bits(0, 2), _bits(1, 3), _bits(1, 4), _bits(5), _bits(5, 6), _bits(5, 6, 7)]
    assert t.path(7) == [5, 6, 7] and t.path(4) == [1, 4]
    assert t.is_root_path([5, 6, 7]) and t.is_root_path([1]) and not t.is_root_path([0, 3])


def test_per_sequence_trees():
    t = TokenTree([[-1, 0, 1, 2], [-1, 0, 0, 0], (-1, -1, 1, 1)])
    assert (t.Tq, t.bs, t.height) == (4, 3, 4)
    assert t.depth == [[0, 1, 2, 3], [0, 1, 1, 1], [0, 0, 1, 1]]
    assert t.ancestors[2] == [_bits(0), _bits(1), _bits(1, 2), _bits(1, 3)]
    assert t.path(3, 0) == [0, 1, 2, 3] and t.path(3, 1) == [0, 3] and t.path(3, 2) == [1, 3]
    assert t.is_root_path([1, 3], 2) and not t.is_root_path([1, 3], 1)
    on = t.to("cpu")
    assert on.anc.shape == (3, 4, 2) and on.anc.dtype == torch.int32 and on.depth.shape == (3, 4) and on.depth.dtype == torch.int64
    assert on.depth.tolist() == t.depth and on.anc[:, :, 0].tolist() == t.ancestors and not on.anc[:, :, 1].any()


def test_device_tensors_of_the_full_mask():
    t = TokenTree([-1] + list(range(63)))                            # a chain of 64: every bit of the last node's set
    assert t.Tq == 64 and t.height == 64 and t.ancestors[63] == (1 << 64) - 1
    on = t.to("cpu")
    assert on is t.to("cpu")                                         # uploaded once per device
    assert on.anc.shape == (1, 64, 2) and on.depth.shape == (1, 64)
    words = on.anc[0].to(torch.int64) & 0xFFFFFFFF                   # (int32 words: bit 31 sits in the sign)
    assert [int(lo) | int(hi) << 32 for lo, hi in words.tolist()] == t.ancestors
    assert on.anc[0, 31].tolist() == [-1, 0] and on.anc[0, 32].tolist() == [-1, 1] and on.anc[0, 63].tolist() == [-1, -1]


@pytest.mark.parametrize("parents", [[-1, 1], [-1, 0, 2], [-1, 0, 3], [0], [-2], [-1, -2], [], [-1] * 65, [[-1, 0], [-1]],
                                     [[-1, 0], [-1, 0, 1]], [[]], 3, [-1, 0.5], [[-1, 0], [-1, 1]]])
def test_refusals(parents):
    with pytest.raises(OQError):
        TokenTree(parents)


def test_the_ops_refuse_cpu_tensors():
    tree = TokenTree([-1, 0, 0])
    q = torch.zeros(2, 3, 4, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 16, 64, dtype=torch.bfloat16)
    lens = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(OQError, match="GPU"):
        ops.tree_attention(q, (k, k.clone()), 8, 0.125, lens, tree)
    with pytest.raises(OQError, match="GPU"):
        ops.kv_tree_commit(k, lens, torch.full((2, 3), -1, dtype=torch.int32))
