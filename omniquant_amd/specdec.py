"""Greedy verification for decoding with the packed blocks: the final norm, then the LM head reduced to one token id per row
on the device (ops.lm_head_argmax) and, for a speculative tree step, the accepted root path (ops.tree_verify_greedy).  Nothing
is read by the host: verify()'s `accept` goes straight into cache.commit_tree(tree, accept) and its `next_token` into the next
step's `expect`.  Stochastic acceptance, top-k / top-p, temperature and drafting itself are not built."""
import torch

from . import ops
from ._capi import OQError


class Verified:
    """What GreedyVerifier.verify returns, all on the device: accept int32 [bs, Tq] (node ids in path order, padded with -1),
    counts int32 [bs], next_token int32 [bs], target int32 [bs, Tq] and target_val float32 [bs, Tq]."""

    __slots__ = ("accept", "counts", "next_token", "target", "target_val")

    def __init__(self, accept, counts, next_token, target, target_val):
        self.accept, self.counts, self.next_token, self.target, self.target_val = accept, counts, next_token, target, target_val

    def __repr__(self):
        return f"Verified(bs={self.accept.shape[0]}, Tq={self.accept.shape[1]})"


class GreedyVerifier:
    """head_weight: the LM head [V, H] (bfloat16 or float16, on the device; kept by reference, never copied); norm: any callable
    applied to the hidden rows first, e.g. the model's final RMSNorm module, or None.  The workspace of the kernels is owned
    here and reused from call to call."""

    def __init__(self, head_weight, norm=None):
        if not torch.is_tensor(head_weight) or head_weight.dim() != 2:
            raise OQError("GreedyVerifier: head_weight must be a [V, H] tensor")
        if not head_weight.is_cuda:
            raise OQError(f"GreedyVerifier: head_weight on {head_weight.device}: the verification needs GPU tensors; there is no "
                          "CPU fallback")
        if norm is not None and not callable(norm):
            raise OQError(f"GreedyVerifier: norm must be callable or None, got {type(norm).__name__}")
        self.weight = head_weight.detach()
        self.norm = norm
        self._workspace = None

    def _rows(self, h):
        with torch.no_grad():
            h = h if self.norm is None else self.norm(h)
        if h.dtype != self.weight.dtype:
            raise OQError(f"GreedyVerifier: hidden rows are {h.dtype}, the head {self.weight.dtype}")
        M = h.numel() // h.shape[-1]
        need = ops.lm_head_workspace(M, self.weight.shape[0])
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != h.device:
            self._workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=h.device)
        return h

    def argmax(self, h):
        """(idx int32, val float32) of h [..., H]: the greedy token of every row and its logit."""
        h = self._rows(h)
        return ops.lm_head_argmax(h, self.weight, workspace=self._workspace)

    def verify(self, h, tree, draft, expect=None):
        """h [bs, Tq, H]: the output rows of a tree step; tree, draft, expect: ops.tree_verify_greedy's.  Returns a Verified."""
        h = self._rows(h)
        return Verified(*ops.tree_verify_greedy(h, self.weight, tree, draft, expect, workspace=self._workspace))
