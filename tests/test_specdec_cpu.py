"""Host side of greedy verification: kvcache.TokenTree.greedy_accept (the rule of ops.tree_verify_greedy in pure Python, the
oracle of tests/test_hip_specdec.py) on hand-written cases, its invariants on random ones, and the loud refusal of CPU tensors
by ops.lm_head_argmax / ops.tree_verify_greedy / specdec.GreedyVerifier.  No GPU needed."""
import random

import pytest
import torch

from omniquant_amd import OQError, ops
from omniquant_amd.kvcache import TokenTree
from omniquant_amd.specdec import GreedyVerifier

FOREST = [-1, -1, 0, 1, 1, -1, 5, 6]
#   0    1      5
#   2   3 4     6
#               7


def test_chain_full_accept_and_breaks():
    t = TokenTree([-1, 0, 1, 2])
    target = [[11, 12, 13, 14]]                                      # after node i the model says 11 + i
    # full accept: root = expect, every child = its parent's target
    assert t.greedy_accept([[10, 11, 12, 13]], target, [10]) == ([[0, 1, 2, 3]], [14])
    # a break in the middle: node 2 drafts 99 instead of 12, node 3 matches its parent's target but hangs below the break
    assert t.greedy_accept([[10, 11, 99, 13]], target, [10]) == ([[0, 1]], [12])
    # a break at the root: nothing accepted, the next token is expect
    assert t.greedy_accept([[7, 11, 12, 13]], target, [10]) == ([[]], [10])
    assert t.greedy_accept([[7, 11, 12, 13]], target, None) == ([[0, 1, 2, 3]], [14])


def test_star():
    t = TokenTree([-1, 0, 0, 0, 0])
    target = [[5, 1, 2, 3, 4]]
    assert t.greedy_accept([[9, 6, 5, 7, 5]], target, [9]) == ([[0, 2]], [2])          # two leaves match: the lower id
    assert t.greedy_accept([[9, 6, 7, 8, 5]], target, [9]) == ([[0, 4]], [4])
    assert t.greedy_accept([[9, 6, 7, 8, 3]], target, [9]) == ([[0]], [5])             # no leaf matches: the root alone


def test_forest_expect_chooses_between_roots():
    t = TokenTree(FOREST)
    draft = [[20, 21, 30, 31, 32, 22, 33, 34]]
    target = [[30, 32, 40, 41, 42, 33, 34, 43]]
    assert t.greedy_accept(draft, target, [20]) == ([[0, 2]], [40])
    assert t.greedy_accept(draft, target, [21]) == ([[1, 4]], [42])
    assert t.greedy_accept(draft, target, [22]) == ([[5, 6, 7]], [43])
    assert t.greedy_accept(draft, target, [23]) == ([[]], [23])
    # expect=None admits every root: the deepest accepted node wins
    assert t.greedy_accept(draft, target, None) == ([[5, 6, 7]], [43])


def test_a_depth_tie_goes_to_the_lowest_id():
    t = TokenTree(FOREST[:5])
    draft = [[20, 21, 30, 31, 32]]
    target = [[30, 32, 40, 41, 42]]
    assert t.greedy_accept(draft, target, None) == ([[0, 2]], [40])                   # nodes 2 and 4 both at depth 1
    t2 = TokenTree([-1, 0, 0, 1, 2])
    assert t2.greedy_accept([[1, 5, 5, 6, 6]], [[5, 6, 6, 7, 8]], [1]) == ([[0, 1, 3]], [7])


def test_per_sequence_trees():
    t = TokenTree([[-1, 0, 1], [-1, 0, 0], [-1, -1, 1]])
    draft = [[1, 2, 3], [1, 9, 2], [8, 1, 2]]
    target = [[2, 3, 4], [2, 5, 6], [7, 2, 9]]
    assert t.greedy_accept(draft, target, [1, 1, 1]) == ([[0, 1, 2], [0, 2], [1, 2]], [4, 6, 9])
    with pytest.raises(OQError, match="batch of 2"):
        t.greedy_accept(draft[:2], target[:2], [1, 1])


def test_padding_leaves_and_an_inactive_sequence():
    t = TokenTree([-1, 0, 0, 1])
    target = [[5, -1, 6, 7], [5, 5, 6, 7]]
    # sequence 0: node 1 is padding although its parent's target is -1 too; sequence 1: all padding
    draft = [[9, -1, 5, -1], [-1, -1, -1, -1]]
    assert t.greedy_accept(draft, target, [9, 4]) == ([[0, 2], []], [6, 4])
    assert t.greedy_accept(draft, target, None) == ([[0, 2], []], [6, -1])
    target[0][0] = -1
    assert t.greedy_accept(draft, target, None) == ([[0], []], [-1, -1])               # -1 never matches a target of -1


def test_invariants_on_random_trees():
    rng = random.Random(0)
    for trial in range(200):
        Tq, bs = rng.randint(1, 64), rng.randint(1, 3)
        per_seq = rng.random() < 0.5
        make = lambda: [rng.randint(-1, n - 1) if rng.random() < 0.9 else -1 for n in range(Tq)]
        tree = TokenTree([make() for _ in range(bs)] if per_seq else make())
        draft = [[rng.randint(-1, 2) for _ in range(Tq)] for _ in range(bs)]
        target = [[rng.randint(0, 2) for _ in range(Tq)] for _ in range(bs)]
        expect = None if rng.random() < 0.3 else [rng.randint(0, 2) for _ in range(bs)]
        paths, nexts = tree.greedy_accept(draft, target, expect)
        assert len(paths) == len(nexts) == bs
        for b, (path, nxt) in enumerate(zip(paths, nexts)):
            assert tree.is_root_path(path, b) and len(path) <= tree.height
            par = tree.parents[b] if per_seq else tree.parents
            depth = tree.depth[b] if per_seq else tree.depth

            def accepted(n):
                if draft[b][n] < 0:
                    return False
                if par[n] < 0:
                    return expect is None or draft[b][n] == expect[b]
                return accepted(par[n]) and draft[b][n] == target[b][par[n]]
            acc = [n for n in range(Tq) if accepted(n)]
            if not acc:
                assert path == [] and nxt == (-1 if expect is None else expect[b])
            else:
                best = min(acc, key=lambda n: (-depth[n], n))
                assert path == tree.path(best, b) and nxt == target[b][best]


def test_greedy_accept_refuses_bad_shapes():
    t = TokenTree([-1, 0])
    with pytest.raises(OQError, match="rows of 2"):
        t.greedy_accept([[1]], [[1, 2]])
    with pytest.raises(OQError, match="rows of 2"):
        t.greedy_accept([[1, 2]], [[1, 2]], [1, 2])
    with pytest.raises(OQError, match="lists"):
        t.greedy_accept([[1.5, 2]], [[1, 2]])


def test_cpu_tensors_are_refused():
    h, w = torch.zeros(2, 3, 64, dtype=torch.bfloat16), torch.zeros(10, 64, dtype=torch.bfloat16)
    tree = TokenTree([-1, 0, 0])
    draft = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(OQError, match="GPU"):
        ops.lm_head_argmax(h, w)
    with pytest.raises(OQError, match="GPU"):
        ops.tree_verify_greedy(h, w, tree, draft)
    with pytest.raises(OQError, match="GPU"):
        GreedyVerifier(w)
    with pytest.raises(OQError):
        ops.lm_head_argmax([1, 2], w)
    with pytest.raises(OQError):
        ops.tree_verify_greedy(h[0], w, tree, draft)
