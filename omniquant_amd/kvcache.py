"""Per-layer KV cache of the packed (real-quant) blocks.

K and V live in preallocated [bs, nkv, cap, hd] buffers in the block's compute dtype (bfloat16 or float32); a forward with a
past appends its rows in place (ops.kv_append, csrc/oq_decode.hip) and attends over rows [0, length) (ops.decode_attention).
The object stands in for the reference's `past_key_value` 2-tuple (models/int_llama_layer.py:121-135,177, transformers 4.31):
len() == 2, iteration and indexing give the [bs, nkv, length, hd] views, so `past[0].shape[2]` is the past length and
`k, v = cache` works.  Unlike a tuple it is appended to IN PLACE, as later transformers' DynamicCache is: the block returns
the same object as `present`.

code_bits=4 (W4A4 blocks, whose k / v rows pass a 4-bit per-(token, head) quantiser before they reach the cache) stores the
quantiser's codes instead of its fake-quant values: k_codes / v_codes uint8 [bs, nkv, cap, hd // 2], byte i of a row holding dim
2i in its low and dim 2i + 1 in its high nibble, and k_meta / v_meta float32 [bs, nkv, cap, 2] = (scale, rounded zero-point)
per row.  A stored element's value is fp32((float(code) - zp) * scale) -- bit for bit what the float32 cache of the same block
holds -- and dequantize() / unpack_codes() are that contract in plain torch.  72 bytes per head row of 128 instead of 256
(bfloat16) or 512 (float32).

code_bits=8 (weight-only blocks, whose k / v sit on no grid) stores one byte per dim: k_codes / v_codes uint8 [bs, nkv, cap, hd],
byte d of a row holding dim d, with the same meta and the same value expression.  The appending kernel quantises the post-RoPE
k and v per (token, head) over hd on the asymmetric 255-level grid, the row range first widened to contain zero (zero-point in
[0, 255]); an all-zero row is codes 0 under meta (0, 0) and reads back as exact zeros.  136 bytes per head row of 128.  The
cache's rows ARE the dequantised values: the block's prefill attends them too, so a row has one value wherever it is used.

ragged=True (either kind): every sequence of the batch has its own length.  `lengths` is an int32 [bs] tensor ON THE DEVICE,
which the append and the attention kernels read themselves (ops.kv_append(..., lengths=), ops.decode_attention(..., lengths=)):
sequence b's valid rows are [0, lengths[b]), a step needs no padding mask and no position tensor, and nothing about its
launches depends on a length the host would have to read back.  `length` stays a host int, now an UPPER BOUND of
lengths.max(): it sizes the buffers and the attention's split plan.  Rows of a sequence at or beyond its own length are
scratch.  There is no common length, so the (k, v) tuple surface is refused; sequence(b) gives one sequence's rows.

PagedKVCache (always ragged) drops the slab: rows live in pages of page_size rows per kv head, taken from one pool
[num_pages, nkv, page_size, ...] per buffer by a PageAllocator and found through a per-sequence page table on the device
(ops.*(..., page_table=)).  A sequence holds the pages its own rows need, a recycled slot returns its pages, and fork() lets
two sequences share the full pages of a common prefix.

PagedKVPool is the paged cache of a whole model: one allocator, one page table and one set of lengths for all layers, the
pools carrying a leading layer dimension; pool.layer(l) is the PagedKVCache view layer l's block steps on, and swap_out /
swap_in move a sequence's pages of every layer to pinned host memory and back (ops.kv_pages_*, csrc/oq_kvpool.hip).

TokenTree is the host description of a tree of draft tokens (speculative decoding).  A block forward with tree= appends the
tree's Tq nodes at rows lengths[b] + t of a ragged cache and attends them under the tree's mask (ops.tree_attention) without
moving any length: the cache only remembers that a tree step is pending.  commit_tree(tree, accept) then compacts the accepted
root path's rows to lengths[b] + 0, 1, ... in every buffer (ops.kv_tree_commit) and grows the lengths by the accepted counts.
Any other change of state (a normal step, set_lengths, fork, swap_*, abort_step) drops a pending tree: its rows are scratch.
"""
import heapq
import operator

import torch

from ._capi import OQError

_DTYPES = (torch.bfloat16, torch.float32)


def unpack_codes(codes, meta, bits=4):
    """float32 [..., hd] values of code rows uint8 [..., hd // 2] under meta float32 [..., 2] = (scale, zero-point): dim 2i is
    the low nibble of byte i, dim 2i + 1 its high nibble, value = (code - zp) * scale with the subtraction and the multiply in
    float32.  bits=8: code rows uint8 [..., hd], byte d holding dim d, the same expression.
    Pure torch (any device): the value contract of the code cache, as PackedLinear.dequantize() is of the weights."""
    if bits == 8:
        c = codes.to(torch.float32)
    elif bits == 4:
        c = torch.stack((codes & 0xF, codes >> 4), dim=-1).reshape(*codes.shape[:-1], 2 * codes.shape[-1]).to(torch.float32)
    else:
        raise OQError(f"unpack_codes: bits {bits} (4 or 8)")
    return (c - meta[..., 1:2]) * meta[..., 0:1]


class _TreeOnDevice:
    """TokenTree.to(device): anc int32 [1 | bs, Tq, 2] (low word = nodes 0..31, high word = 32..63 of each node's ancestor
    set) and depth int64 [1 | bs, Tq]."""

    def __init__(self, anc, depth):
        self.anc, self.depth = anc, depth


class TokenTree:
    """A tree of Tq draft tokens for one speculative step, or one such tree per sequence.  parents: a sequence of Tq ints, or bs
    sequences of Tq ints each; parents[t] in [-1, t) names node t's parent (so the order is topological), -1 hangs the node off
    the committed past, and several roots are allowed.  1 <= Tq <= 64.  Pure Python: no device is needed to build one.

    Tq, bs (None: one tree for the whole batch), height = largest depth + 1; depth (roots 0) and ancestors (one 64-bit int per
    node, bit u set iff u is the node or one of its ancestors: only bits <= t) are lists over the nodes, or with per-sequence
    trees lists of such lists; path(t, b=0) gives the node ids from a root down to t, ascending.  to(device) uploads the masks
    and depths once per device and caches them."""

    MAX_NODES = 64

    def __init__(self, parents):
        try:
            outer = list(parents)
            per_seq = len(outer) > 0 and not hasattr(outer[0], "__index__")
            trees = [[operator.index(p) for p in t] for t in outer] if per_seq else [[operator.index(p) for p in outer]]
        except TypeError:
            raise OQError(f"TokenTree: parents must be Tq ints or bs sequences of Tq ints, got {parents!r}") from None
        Tq = len(trees[0])
        if not 1 <= Tq <= self.MAX_NODES:
            raise OQError(f"TokenTree: {Tq} nodes (1 to {self.MAX_NODES})")
        if any(len(t) != Tq for t in trees):
            raise OQError(f"TokenTree: per-sequence trees of {[len(t) for t in trees]} nodes (one Tq for the batch; pad with leaves)")
        for t in trees:
            for node, par in enumerate(t):
                if not -1 <= par < node:
                    raise OQError(f"TokenTree: parents[{node}] = {par} outside [-1, {node}) (a parent precedes its children; -1: "
                                  "a root)")
        self.Tq, self.bs = Tq, len(trees) if per_seq else None
        self.parents = trees if per_seq else trees[0]
        depth, anc = [], []
        for t in trees:
            d, a = [], []
            for node, par in enumerate(t):
                d.append(0 if par < 0 else d[par] + 1)
                a.append((1 << node) | (0 if par < 0 else a[par]))
            depth.append(d)
            anc.append(a)
        self.height = max(max(d) for d in depth) + 1
        self.depth, self.ancestors = (depth, anc) if per_seq else (depth[0], anc[0])
        self._trees, self._depth, self._anc = trees, depth, anc
        self._on = {}

    def _tree(self, b):
        return 0 if self.bs is None else operator.index(b)

    def path(self, t, b=0):
        """The node ids from a root to node t (of sequence b's tree), ascending."""
        t = operator.index(t)
        if not 0 <= t < self.Tq:
            raise IndexError(f"node {t} of a tree of {self.Tq}")
        anc = self._anc[self._tree(b)][t]
        return [u for u in range(t + 1) if anc >> u & 1]

    def is_root_path(self, nodes, b=0):
        """Whether `nodes` is empty or a path from a root downwards (of sequence b's tree): each node the child of the one before."""
        par = self._trees[self._tree(b)]
        prev = -1
        for n in nodes:
            if not 0 <= n < self.Tq or par[n] != prev:
                return False
            prev = n
        return True

    def greedy_accept(self, draft, target, expect=None):
        """Greedy acceptance on the host, the rule of ops.tree_verify_greedy (csrc/oq_lmhead.hip) on lists.  draft[b][t]: the
        drafted token of node t (-1: a padding node), target[b][t]: the model's greedy token after node t, expect[b] (or None):
        the token the model chose after the committed past.  A node matches iff its draft is >= 0 and equals its parent's target
        (a root: expect[b], or anything when expect is None); it is accepted iff it and all its ancestors match.  The accepted
        node of largest depth wins, the lowest id among equals.  Returns (paths, next_tokens): per sequence the winner's root
        path (ascending node ids; [] if no node is accepted) and target[b][winner] (expect[b], or -1 without expect, if none)."""
        try:
            draft = [[operator.index(x) for x in row] for row in draft]
            target = [[operator.index(x) for x in row] for row in target]
            expect = None if expect is None else [operator.index(x) for x in expect]
        except TypeError:
            raise OQError("TokenTree.greedy_accept: draft and target are bs lists of Tq ints, expect bs ints or None") from None
        bs = len(draft)
        if self.bs not in (None, bs):
            raise OQError(f"TokenTree.greedy_accept: {self!r} for a batch of {bs}")
        if len(target) != bs or (expect is not None and len(expect) != bs) or any(len(r) != self.Tq for r in draft + target):
            raise OQError(f"TokenTree.greedy_accept: draft and target must be {bs} rows of {self.Tq} tokens, expect {bs} tokens")
        paths, nexts = [], []
        for b in range(bs):
            i = self._tree(b)
            par, depth = self._trees[i], self._depth[i]
            accepted, best = [], -1
            for t in range(self.Tq):
                if par[t] < 0:
                    ok = draft[b][t] >= 0 and (expect is None or draft[b][t] == expect[b])
                else:
                    ok = draft[b][t] >= 0 and accepted[par[t]] and draft[b][t] == target[b][par[t]]
                accepted.append(ok)
                if ok and (best < 0 or depth[t] > depth[best]):
                    best = t
            paths.append(self.path(best, b) if best >= 0 else [])
            nexts.append(target[b][best] if best >= 0 else (-1 if expect is None else expect[b]))
        return paths, nexts

    def to(self, device):
        """The tree on `device` (uploaded once, then cached): an object with anc int32 [1 | bs, Tq, 2] and depth int64
        [1 | bs, Tq]."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        on = self._on.get(device)
        if on is None:
            words = [[[a & 0xFFFFFFFF, a >> 32] for a in tree] for tree in self._anc]
            anc = torch.tensor(words, dtype=torch.int64).to(torch.int32)         # (wraps bit 31 into the sign)
            on = _TreeOnDevice(anc.to(device), torch.tensor(self._depth, dtype=torch.int64).to(device))
            self._on[device] = on
        return on

    def __repr__(self):
        return f"TokenTree(Tq={self.Tq}, height={self.height}" + ("" if self.bs is None else f", bs={self.bs}") + ")"


def _accept_in(who, cache, tree, accept):
    """commit_tree's arguments, checked before anything changes: (accept int32 [bs, Tq] on the device, counts int32 [bs] on the
    device, the counts as Python ints or None for the device form)."""
    if not isinstance(tree, TokenTree):
        raise OQError(f"{who}: expected a TokenTree, got {type(tree).__name__}")
    Tq, bs = tree.Tq, cache.bs
    if cache._tree_pending is None:
        raise OQError(f"{who}: {cache!r} has no pending tree step (a forward with tree= books one; any other change of state "
                      "drops it)")
    if cache._tree_pending != Tq:
        raise OQError(f"{who}: {tree!r}, the pending tree step has {cache._tree_pending} nodes")
    if tree.bs not in (None, bs):
        raise OQError(f"{who}: {tree!r} for a batch of {bs}")
    if torch.is_tensor(accept):
        if accept.dtype != torch.int32 or tuple(accept.shape) != (bs, Tq) or accept.device != cache.device:
            raise OQError(f"{who}: accept must be an int32 [{bs}, {Tq}] tensor on {cache.device} (node ids in path order, padded "
                          f"with -1), got {tuple(accept.shape)} {accept.dtype} on {accept.device}")
        accept = accept.contiguous()
        counts = (accept >= 0).to(torch.int32).cummin(dim=1).values.sum(dim=1, dtype=torch.int32)
        return accept, counts, None
    try:
        paths = [[operator.index(n) for n in path] for path in accept]
    except TypeError:
        raise OQError(f"{who}: accept must be {bs} lists of node ids or an int32 [{bs}, {Tq}] device tensor") from None
    if len(paths) != bs:
        raise OQError(f"{who}: {len(paths)} paths for a batch of {bs}")
    for b, path in enumerate(paths):
        if not tree.is_root_path(path, b):
            raise OQError(f"{who}: sequence {b}'s path {path} is not a root path of {tree!r} (empty, or a root followed by a "
                          "child of each previous node)")
    rows = [path + [-1] * (Tq - len(path)) for path in paths]
    host = [len(path) for path in paths]
    return (torch.tensor(rows, dtype=torch.int32).to(cache.device, non_blocking=True),
            torch.tensor(host, dtype=torch.int32).to(cache.device, non_blocking=True), host)


class PackedKVCache:
    _tree_pending = None                # the node count of a tree step whose rows wait for commit_tree (ragged caches)

    def __init__(self, bs, nkv, hd, dtype, device, capacity=0, code_bits=None, ragged=False):
        device = torch.device(device)
        if device.type != "cuda":
            raise OQError(f"PackedKVCache needs a GPU device (got {device}); there is no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if dtype not in _DTYPES:
            raise OQError(f"PackedKVCache: dtype {dtype} (the packed blocks compute in bfloat16 or float32)")
        if min(int(bs), int(nkv), int(hd)) <= 0 or int(capacity) < 0:
            raise OQError(f"PackedKVCache: bs {bs}, nkv {nkv}, hd {hd}, capacity {capacity}")
        self.bs, self.nkv, self.hd, self.dtype, self.device = int(bs), int(nkv), int(hd), dtype, device
        if code_bits is not None and code_bits not in (4, 8):
            raise OQError(f"PackedKVCache: code_bits {code_bits} (None: float rows, 4 or 8)")
        if code_bits is not None and self.hd not in (64, 128):
            raise OQError(f"PackedKVCache: a code cache covers head_dim 64 and 128, not {self.hd}")
        self.code_bits = code_bits
        self.length = 0
        self.ragged = bool(ragged)
        self.lengths = torch.zeros(self.bs, dtype=torch.int32, device=device) if self.ragged else None
        self._allocate(int(capacity))

    def _buffers(self):
        """Names of the storage tensors of this kind (each [bs, nkv, cap, ...])."""
        return ("k", "v") if self.code_bits is None else ("k_codes", "v_codes", "k_meta", "v_meta")

    def _allocate(self, cap, keep=None):
        """Fresh buffers of `cap` rows; keep: a cache of this kind whose rows [0, keep.length) are copied in."""
        shape = (self.bs, self.nkv, cap)
        for name in self._buffers():
            if self.code_bits is None:
                t = torch.empty(shape + (self.hd,), dtype=self.dtype, device=self.device)
            elif name.endswith("codes"):
                t = torch.empty(shape + (self.hd * self.code_bits // 8,), dtype=torch.uint8, device=self.device)
            else:
                t = torch.empty(shape + (2,), dtype=torch.float32, device=self.device)
            if keep is not None and keep.length:
                t[:, :, :keep.length].copy_(getattr(keep, name)[:, :, :keep.length])
            setattr(self, name, t)

    @property
    def capacity(self):
        return getattr(self, self._buffers()[0]).shape[2]

    def nbytes(self):
        """Bytes of device memory the cache's buffers hold (the whole capacity)."""
        return sum(getattr(self, n).numel() * getattr(self, n).element_size() for n in self._buffers())

    def _no_tuple(self, what):
        if self.ragged:
            raise OQError(f"{what}: a ragged cache has no common length, hence no [bs, nkv, length, hd] tensors; "
                          "sequence(b) gives one sequence's rows")

    def set_lengths(self, lengths, bound=None):
        """Set the per-sequence lengths of a ragged cache: rows at or beyond a sequence's length become scratch, so
        set_lengths([n0, 0, n2]) hands slot 1 to a new prompt while the others keep theirs.  A Python sequence of ints gives
        length = max(lengths) (or `bound`, if larger) with no device read; an int32 [bs] device tensor is copied as it is and
        needs the explicit host `bound` >= its maximum that `length` becomes."""
        if not self.ragged:
            raise OQError("set_lengths: not a ragged cache (PackedKVCache(..., ragged=True))")
        if torch.is_tensor(lengths):
            if lengths.dtype != torch.int32 or tuple(lengths.shape) != (self.bs,) or lengths.device != self.device:
                raise OQError(f"set_lengths: expected an int32 [{self.bs}] tensor on {self.device}, got {tuple(lengths.shape)} "
                              f"{lengths.dtype} on {lengths.device}")
            if bound is None:
                raise OQError("set_lengths: a device tensor needs bound= (the host never reads the lengths back)")
            top = int(bound)
        else:
            seq = [operator.index(n) for n in lengths]
            if len(seq) != self.bs or min(seq) < 0:
                raise OQError(f"set_lengths: {seq} for a batch of {self.bs} (one length >= 0 per sequence)")
            top = max(seq) if bound is None else int(bound)
            if top < max(seq):
                raise OQError(f"set_lengths: bound {top} below the longest sequence ({max(seq)})")
            lengths = torch.tensor(seq, dtype=torch.int32)
        if not 0 <= top <= self.capacity:
            raise OQError(f"set_lengths: bound {top} outside the capacity {self.capacity}")
        self._tree_pending = None
        self.lengths.copy_(lengths)
        self.length = top

    def sequence(self, b):
        """(k, v) of sequence b of a ragged cache as [nkv, lengths[b], hd] copies in `dtype` (a code cache's are dequantised by
        unpack_codes).  The one call that reads a length back from the device: for tests and debugging, not for the step."""
        if not self.ragged:
            raise OQError("sequence: not a ragged cache (index a uniform cache as (k, v))")
        b = operator.index(b)
        if not 0 <= b < self.bs:
            raise IndexError(f"sequence {b} of a batch of {self.bs}")
        n = min(max(int(self.lengths[b]), 0), self.capacity)
        if self.code_bits is None:
            return self.k[b, :, :n].clone(), self.v[b, :, :n].clone()
        return tuple(unpack_codes(c[b, :, :n], m[b, :, :n], self.code_bits).to(self.dtype)
                     for c, m in ((self.k_codes, self.k_meta), (self.v_codes, self.v_meta)))

    def dequantize(self):
        """(k, v) as [bs, nkv, length, hd] tensors in `dtype`.  On a code cache these are fresh copies computed by
        unpack_codes (the value contract; one rounding to bfloat16 when that is the dtype); on a float cache, the views."""
        self._no_tuple("dequantize")
        if self.code_bits is None:
            return self.k[:, :, :self.length], self.v[:, :, :self.length]
        n = self.length
        return tuple(unpack_codes(c[:, :, :n], m[:, :, :n], self.code_bits).to(self.dtype)
                     for c, m in ((self.k_codes, self.k_meta), (self.v_codes, self.v_meta)))

    def book_step(self, Tq, new_tokens):
        """Book a step of Tq rows on a ragged cache, after the step's attention (which reads the pre-step lengths; the stream
        orders the launches): new_tokens = (counts or None for all Tq, growth of the bound, the counts on the host or None) as
        block_common._new_tokens_in returns it.  The block forwards call this."""
        counts, grow, _ = new_tokens
        self._tree_pending = None
        self.lengths.add_(Tq if counts is None else counts)
        self.length = self.length + (Tq if grow is None else grow)

    def book_tree_step(self, Tq):
        """Book a TREE step of Tq nodes (a block forward with tree=): lengths and length do not move; the cache remembers that
        Tq tree rows at lengths[b] + t wait for commit_tree.  The block forwards call this."""
        self._tree_pending = int(Tq)

    def commit_tree(self, tree, accept):
        """Make the accepted root path of the pending tree step each sequence's next rows.  accept: bs lists of node ids, each
        empty or a root path of `tree` (checked; `length` grows by the longest), or an int32 [bs, Tq] device tensor of node ids
        in path order padded with -1 (not validated, the caller guarantees root paths; the counts are computed on the device,
        nothing is read back, and `length` grows by tree.height).  One ops.kv_tree_commit launch per buffer, then lengths +=
        counts.  Without a pending tree step, or with a tree of another Tq, OQError and nothing changes."""
        from . import ops
        if not self.ragged:
            raise OQError("commit_tree: not a ragged cache (PackedKVCache(..., ragged=True))")
        acc, counts, host = _accept_in("commit_tree", self, tree, accept)
        for name in self._buffers():
            ops.kv_tree_commit(getattr(self, name), self.lengths, acc)
        self._tree_pending = None
        self.lengths.add_(counts)
        self.length = min(self.length + (tree.height if host is None else max(host)), self.capacity)

    def reserve(self, n):
        """Room for n more rows: the capacity grows geometrically (at least doubling) and the valid rows move to the new
        buffers.  A cache sized to prompt + max_new_tokens up front never reallocates."""
        need = self.length + int(n)
        self._tree_pending = None       # (a new step begins: the rows of an uncommitted tree are scratch)
        if need <= self.capacity:
            return
        self._allocate(max(need, 2 * self.capacity, 16), keep=self)

    # ---- the reference's (k, v) tuple surface ------------------------------------------------------------------------------
    def __len__(self):
        return 2

    def __getitem__(self, i):
        """0 = keys, 1 = values, [bs, nkv, length, hd]: views of a float cache; of a code cache, dequantised COPIES, not views
        (writing to them does not change the cache)."""
        self._no_tuple("indexing")
        if isinstance(i, slice):
            return (self[0], self[1])[i]
        i = operator.index(i)
        if i < 0:
            i += 2
        if i not in (0, 1):
            raise IndexError("PackedKVCache index out of range (0 = keys, 1 = values)")
        if self.code_bits is not None:
            return self.dequantize()[i]
        return (self.k if i == 0 else self.v)[:, :, :self.length]

    def __iter__(self):
        self._no_tuple("iteration")
        yield from self.dequantize()

    def __repr__(self):
        return (f"PackedKVCache(bs={self.bs}, nkv={self.nkv}, hd={self.hd}, dtype={self.dtype}, length={self.length}, "
                f"capacity={self.capacity}" + ("" if self.code_bits is None else f", code_bits={self.code_bits}")
                + (", ragged (length bounds the per-sequence lengths)" if self.ragged else "") + ")")

    @classmethod
    def from_tuple(cls, kv, dtype=None, capacity=None, head_bits=None, code_bits=None, ragged=False):
        """A cache holding copies of the reference-layout (k, v), each [bs, nkv, T, hd] (any float dtype, converted once);
        the tensors passed in are never modified.  head_bits (W4A4 blocks): the rows are quantised per (token, head) over hd on
        that grid as they are imported (ops.kv_append_quant without rotation), which is what the block's own appends store.
        code_bits=4 (with head_bits=4): the same quantisation, once, into a code cache.
        code_bits=8 (head_bits must be None: the weight-only blocks): the raw rows pass the 8-bit code cache's own quantiser
        (ops.kv_append_codes without rotation), once.
        ragged: refused -- a tuple has one length for the whole batch."""
        if ragged:
            raise OQError("past_key_value: a (k, v) tuple has one length for the batch and cannot fill a ragged cache")
        if len(kv) != 2:
            raise OQError(f"past_key_value: expected (k, v), got {len(kv)} tensors")
        k, v = kv
        if not (torch.is_tensor(k) and torch.is_tensor(v)) or k.dim() != 4 or tuple(k.shape) != tuple(v.shape):
            raise OQError("past_key_value: k and v must be [bs, nkv, T, hd] tensors of one shape")
        if not (k.is_cuda and v.is_cuda):
            raise OQError("past_key_value: GPU tensors expected (no CPU fallback)")
        bs, nkv, T, hd = k.shape
        if code_bits == 8:
            if head_bits is not None:
                raise OQError(f"past_key_value: an 8-bit code cache holds a weight-only block's rows (head_bits {head_bits} given)")
        elif code_bits is not None and head_bits != code_bits:
            raise OQError(f"past_key_value: a {code_bits}-bit code cache holds rows quantised on that grid (head_bits {head_bits})")
        c = cls(bs, nkv, hd, dtype or k.dtype, k.device, max(int(capacity or 0), T), code_bits=code_bits)
        if T and code_bits == 8:
            from . import ops
            src = c.dtype if k.dtype == c.dtype else torch.float32
            kt, vt = (t.transpose(1, 2).to(src).contiguous() for t in (k, v))         # [bs, T, nkv, hd], fresh copies
            ops.kv_append_codes(kt, vt, c.dtype, c.k_codes, c.v_codes, c.k_meta, c.v_meta, past=0)
        elif T and head_bits is not None:
            from . import ops
            src = c.dtype if k.dtype == c.dtype else torch.float32
            kt, vt = (t.transpose(1, 2).to(src).contiguous() for t in (k, v))         # [bs, T, nkv, hd], fresh copies
            if code_bits is not None:
                ops.kv_append_codes(kt, vt, c.dtype, c.k_codes, c.v_codes, c.k_meta, c.v_meta, past=0)
            else:
                ops.kv_append_quant(kt, vt, head_bits, c.dtype, k_cache=c.k, v_cache=c.v, past=0)
        elif T:
            c.k[:, :, :T].copy_(k)
            c.v[:, :, :T].copy_(v)
        c.length = T
        return c

    def to_tuple(self):
        """(k, v) as contiguous [bs, nkv, length, hd] copies (the reference's layout; a code cache's are dequantised)."""
        self._no_tuple("to_tuple")
        return tuple(t.clone(memory_format=torch.contiguous_format) for t in self)

    def clone(self):
        c = PackedKVCache(self.bs, self.nkv, self.hd, self.dtype, self.device, 0, code_bits=self.code_bits, ragged=self.ragged)
        c._allocate(self.capacity, keep=self)
        c.length = self.length
        if self.ragged:
            c.lengths.copy_(self.lengths)
        return c


class PageAllocator:
    """Host bookkeeping of a pool of `num_pages` pages: a free list handed out in ascending page order and one reference count
    per page (a page is free exactly when its count is 0).  Pure Python, no device; the same sequence of calls gives the same
    page ids."""

    def __init__(self, num_pages):
        num_pages = operator.index(num_pages)
        if num_pages <= 0:
            raise OQError(f"PageAllocator: num_pages {num_pages}")
        self.num_pages = num_pages
        self._free = list(range(num_pages))         # a heap: ascending ids
        self._refs = [0] * num_pages

    @property
    def n_free(self):
        return len(self._free)

    def refcount(self, page):
        return self._refs[operator.index(page)]

    def _held(self, what, pages):
        pages = [operator.index(p) for p in pages]
        for p in pages:
            if not 0 <= p < self.num_pages or self._refs[p] <= 0:
                raise OQError(f"PageAllocator.{what}: page {p} is not allocated")
        return pages

    def alloc(self, n):
        """n fresh pages (reference count 1), the lowest free ids in ascending order; all or nothing."""
        n = operator.index(n)
        if n < 0 or n > len(self._free):
            raise OQError(f"PageAllocator.alloc: {n} pages wanted, {len(self._free)} of {self.num_pages} free")
        pages = [heapq.heappop(self._free) for _ in range(n)]
        for p in pages:
            self._refs[p] = 1
        return pages

    def retain(self, pages):
        """One more reference to each of `pages` (allocated ones only)."""
        pages = self._held("retain", pages)
        for p in pages:
            self._refs[p] += 1

    def release(self, pages):
        """Drop one reference to each of `pages`; a page whose count reaches 0 returns to the free list.  Releasing a page more
        often than it is held is refused, and then nothing is released."""
        pages = self._held("release", pages)
        for p in set(pages):
            if pages.count(p) > self._refs[p]:
                raise OQError(f"PageAllocator.release: page {p} released {pages.count(p)} times, held {self._refs[p]} times")
        for p in pages:
            self._refs[p] -= 1
            if self._refs[p] == 0:
                heapq.heappush(self._free, p)

    def clone(self):
        c = PageAllocator(self.num_pages)
        c._free, c._refs = list(self._free), list(self._refs)
        return c

    def __repr__(self):
        return f"PageAllocator({self.n_free} of {self.num_pages} pages free)"


class PagedKVCache:
    """One layer's paged, ragged KV cache.  Pools k / v [num_pages, nkv, page_size, hd] in `dtype` -- or, with code_bits=4 / 8,
    k_codes / v_codes uint8 [num_pages, nkv, page_size, hd // 2 resp. hd] and k_meta / v_meta float32 [num_pages, nkv, page_size, 2] --
    and page_table int32 [bs, max_pages] on the device: logical row j of sequence b lives in page page_table[b, j // page_size]
    (entries of pages a sequence does not hold are -1, which the kernels neither store to nor load).  `lengths` (device) and
    `length` (host upper bound) are a ragged PackedKVCache's; capacity = max_pages * page_size rows per sequence.

    The host keeps a mirror of the table and, per sequence, an upper bound of its length: exact where lengths arrive as Python
    ints (set_lengths, the block forwards' new_tokens), grown by the step's rows where they arrive as device tensors.  reserve()
    allocates pages from the bounds and uploads the table only when it changed; no call of the step path reads the device.

    Sharing invariant (fork): a page with more than one reference is never written.  Appends only write rows at or beyond a
    sequence's own length; fork shares only pages that lie wholly below the forked length and copies the partial last page, and
    set_lengths gives a sequence a private copy of a shared page before its length may point into it.  So every row at or
    beyond a sequence's length lies in a page that sequence owns alone, and no copy-on-write is needed in the step."""

    ragged = True
    paged = True
    _tree_pending = None                # as PackedKVCache's

    def __init__(self, bs, nkv, hd, dtype, device, num_pages, page_size=16, max_pages=None, code_bits=None, _lead=()):
        who = type(self).__name__
        device = torch.device(device)
        if device.type != "cuda":
            raise OQError(f"{who} needs a GPU device (got {device}); there is no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if dtype not in _DTYPES:
            raise OQError(f"{who}: dtype {dtype} (the packed blocks compute in bfloat16 or float32)")
        max_pages = num_pages if max_pages is None else max_pages
        if min(int(bs), int(nkv), int(hd), int(num_pages), int(max_pages)) <= 0:
            raise OQError(f"{who}: bs {bs}, nkv {nkv}, hd {hd}, num_pages {num_pages}, max_pages {max_pages}")
        if page_size not in (16, 32, 64, 128):
            raise OQError(f"{who}: page_size {page_size} (16, 32, 64 or 128)")
        if int(hd) not in (64, 128):
            raise OQError(f"{who}: head_dim {hd} (the decode kernels cover 64 and 128)")
        if code_bits is not None and code_bits not in (4, 8):
            raise OQError(f"{who}: code_bits {code_bits} (None: float rows, 4 or 8)")
        self.bs, self.nkv, self.hd, self.dtype, self.device = int(bs), int(nkv), int(hd), dtype, device
        self.num_pages, self.page_size, self.max_pages, self.code_bits = int(num_pages), int(page_size), int(max_pages), code_bits
        self.length = 0
        self.lengths = torch.zeros(self.bs, dtype=torch.int32, device=device)
        self.allocator = PageAllocator(self.num_pages)
        self._pages = [[] for _ in range(self.bs)]          # host mirror of the table: the pages each sequence holds, in order
        self._bound = [0] * self.bs                         # host upper bound of each length
        self._exact = [True] * self.bs                      # ... which is the length itself (it came as a Python int)
        self.page_table = torch.full((self.bs, self.max_pages), -1, dtype=torch.int32, device=device)
        shape = tuple(_lead) + (self.num_pages, self.nkv, self.page_size)      # (_lead: PagedKVPool's layer dimension)
        for name in self._buffers():
            if code_bits is None:
                t = torch.empty(shape + (self.hd,), dtype=dtype, device=device)
            elif name.endswith("codes"):
                t = torch.empty(shape + (self.hd * code_bits // 8,), dtype=torch.uint8, device=device)
            else:
                t = torch.empty(shape + (2,), dtype=torch.float32, device=device)
            setattr(self, name, t)

    def _buffers(self):
        """Names of the pool tensors of this kind (each [num_pages, nkv, page_size, ...])."""
        return ("k", "v") if self.code_bits is None else ("k_codes", "v_codes", "k_meta", "v_meta")

    @property
    def capacity(self):
        return self.max_pages * self.page_size

    @property
    def n_free(self):
        return self.allocator.n_free

    def nbytes(self):
        """Bytes of device memory the pools and the page table hold."""
        return sum(t.numel() * t.element_size() for t in [getattr(self, n) for n in self._buffers()] + [self.page_table])

    def pages(self, b):
        """The page ids sequence b holds, in row order (the host mirror of its table row)."""
        return list(self._pages[operator.index(b)])

    def _need(self, rows):
        return -(-rows // self.page_size)

    def _upload(self):
        """The host mirror to the device: one non-blocking copy, ordered on the current stream behind the launches that read the
        table it replaces."""
        rows = [p + [-1] * (self.max_pages - len(p)) for p in self._pages]
        self.page_table.copy_(torch.tensor(rows, dtype=torch.int32), non_blocking=True)

    def _copy_page(self, src, dst):
        for name in self._buffers():
            t = getattr(self, name)
            t[dst].copy_(t[src])

    def reserve(self, n):
        """Pages for n more rows of every sequence, counted from its host bound.  All or nothing: a sequence that would exceed
        max_pages, or a pool without enough free pages, raises OQError before anything changes.  The table is uploaded only if
        a page was added; a step inside the pages already held uploads nothing."""
        n = int(n)
        want = [max(self._need(bd + n) - len(p), 0) for bd, p in zip(self._bound, self._pages)]
        for b, (w, p) in enumerate(zip(want, self._pages)):
            if len(p) + w > self.max_pages or self.length + n > self.capacity:
                raise OQError(f"{self!r}: {n} more rows take sequence {b} beyond max_pages = {self.max_pages} "
                              f"({self.capacity} rows)")
        if sum(want) > self.allocator.n_free:
            raise OQError(f"{self!r}: {n} more rows per sequence need {sum(want)} pages, {self.allocator.n_free} are free")
        self._tree_pending = None       # (a new step begins: the rows of an uncommitted tree are scratch; a refusal keeps them)
        if not any(want):
            return
        for w, p in zip(want, self._pages):
            p.extend(self.allocator.alloc(w))
        self._upload()

    def book_step(self, Tq, new_tokens):
        """PackedKVCache.book_step, and advance() books the step in the host bounds.  The block forwards call this."""
        counts, grow, host_counts = new_tokens
        self._tree_pending = None
        self.lengths.add_(Tq if counts is None else counts)
        self.length = self.length + (Tq if grow is None else grow)
        self.advance(Tq, host_counts, exact=counts is None or host_counts is not None)

    def book_tree_step(self, Tq):
        """PackedKVCache.book_tree_step: nothing moves, no page is trimmed; the pages reserve() took for the tree's rows stay
        with their sequences until commit_tree (or a later step's trim)."""
        self._tree_pending = int(Tq)

    def _commit_buffers(self, acc):
        from . import ops
        for name in self._buffers():        # (a pool's buffers carry the layer dimension: one launch serves all layers)
            ops.kv_tree_commit(getattr(self, name), self.lengths, acc, page_table=self.page_table)

    def commit_tree(self, tree, accept):
        """PackedKVCache.commit_tree on paged storage.  Host form: the host bounds grow by the exact counts and the pages
        beyond them return to the pool (a table upload only if one did).  Device form: the bounds grow by tree.height and
        become upper bounds, as with a device new_tokens.  The commit writes only rows at or beyond a sequence's length, which
        lie in pages it owns alone (the sharing invariant)."""
        acc, counts, host = _accept_in("commit_tree", self, tree, accept)
        self._commit_buffers(acc)
        self._tree_pending = None
        self.lengths.add_(counts)
        if host is None:
            self.length = min(self.length + tree.height, self.capacity)
            PagedKVCache.advance(self, tree.height, None, exact=False)
        else:
            self.length = self.length + max(host)
            PagedKVCache.advance(self, 0, host)

    def advance(self, rows, counts=None, exact=True):
        """Book a step of `rows` rows per sequence that the kernels have appended: the host bounds grow by `counts` (the valid
        rows of each sequence as Python ints) or by `rows` -- exact=False: only an upper bound of what the sequences grew by,
        their counts being a device tensor.  With counts, the pages that only the pad rows of a right-padded step made
        reserve() take are returned to the pool.  book_step() calls this after it has updated `lengths` and `length`."""
        if counts is None:
            self._bound = [bd + int(rows) for bd in self._bound]
            if not exact:
                self._exact = [False] * self.bs
            return
        self._bound = [bd + int(c) for bd, c in zip(self._bound, counts)]
        if self._trim():
            self._upload()

    def _trim(self):
        """Release the pages beyond each sequence's bound; says whether the table changed."""
        changed = False
        for bd, p in zip(self._bound, self._pages):
            keep = self._need(bd)
            if len(p) > keep:
                self.allocator.release(p[keep:])
                del p[keep:]
                changed = True
        return changed

    def set_lengths(self, lengths, bound=None):
        """Set the per-sequence lengths, in the two forms of PackedKVCache.set_lengths.  Python ints: each sequence keeps the
        pages its rows need and releases the rest -- set_lengths([n0, 0, n2]) returns all of slot 1's pages to the pool -- and
        a sequence cut back into a page it shares first gets a private copy of that page (the sharing invariant).  A length
        beyond the pages held takes fresh pages (their rows are scratch).  An int32 [bs] device tensor needs the host `bound`:
        every sequence then holds pages for `bound` rows, none of them shared.  All or nothing; no device read."""
        ps = self.page_size
        if torch.is_tensor(lengths):
            if lengths.dtype != torch.int32 or tuple(lengths.shape) != (self.bs,) or lengths.device != self.device:
                raise OQError(f"set_lengths: expected an int32 [{self.bs}] tensor on {self.device}, got {tuple(lengths.shape)} "
                              f"{lengths.dtype} on {lengths.device}")
            if bound is None:
                raise OQError("set_lengths: a device tensor needs bound= (the host never reads the lengths back)")
            top = int(bound)
            bounds, exact, dev = [top] * self.bs, False, lengths
        else:
            seq = [operator.index(n) for n in lengths]
            if len(seq) != self.bs or min(seq) < 0:
                raise OQError(f"set_lengths: {seq} for a batch of {self.bs} (one length >= 0 per sequence)")
            top = max(seq) if bound is None else int(bound)
            if top < max(seq):
                raise OQError(f"set_lengths: bound {top} below the longest sequence ({max(seq)})")
            bounds, exact, dev = seq, True, torch.tensor(seq, dtype=torch.int32)
        if not 0 <= top <= self.capacity:
            raise OQError(f"set_lengths: bound {top} outside the capacity {self.capacity}")
        # the plan: pages kept, pages whose private copy is needed (shared ones the sequence may now write), fresh pages
        refs = self.allocator.refcount
        keep = [min(self._need(bd), len(p)) if exact else len(p) for bd, p in zip(bounds, self._pages)]
        fresh = [max(self._need(bd) - len(p), 0) for bd, p in zip(bounds, self._pages)]
        copies = []
        for b, (bd, p) in enumerate(zip(bounds, self._pages)):
            first = bd // ps if exact else 0                # the first page the sequence may write from now on
            copies += [(b, i) for i in range(first, keep[b]) if refs(p[i]) > 1]
        dropped = [pg for b, p in enumerate(self._pages) for pg in p[keep[b]:]]
        freed = sum(1 for pg in set(dropped) if dropped.count(pg) == refs(pg))
        if len(copies) + sum(fresh) > self.allocator.n_free + freed:
            raise OQError(f"{self!r}: set_lengths needs {len(copies) + sum(fresh)} pages, {self.allocator.n_free + freed} are free")
        self._tree_pending = None
        self.allocator.release(dropped)
        for b, p in enumerate(self._pages):
            del p[keep[b]:]
        for b, i in copies:
            (new,) = self.allocator.alloc(1)
            self._copy_page(self._pages[b][i], new)
            self.allocator.release([self._pages[b][i]])
            self._pages[b][i] = new
        for b, w in enumerate(fresh):
            self._pages[b].extend(self.allocator.alloc(w))
        if dropped or copies or any(fresh):
            self._upload()
        self.lengths.copy_(dev, non_blocking=True)
        self._bound, self._exact, self.length = list(bounds), [exact] * self.bs, top

    def fork(self, src, dst):
        """Sequence dst, which must be empty, becomes a copy of sequence src: the pages that lie wholly below src's length are
        shared by reference, a partial last page is copied into a fresh page (one device-side page copy per buffer), and dst's
        length and bound become src's.  Both then append into pages of their own (the sharing invariant of the class).  src's
        length must be known to the host exactly (set as Python ints / grown by new_tokens counts or whole steps from there)."""
        src, dst = operator.index(src), operator.index(dst)
        if not (0 <= src < self.bs and 0 <= dst < self.bs) or src == dst:
            raise OQError(f"fork: sequences {src} -> {dst} of a batch of {self.bs}")
        if self._bound[dst] != 0 or not self._exact[dst]:
            raise OQError(f"fork: sequence {dst} is not empty (set_lengths with 0 for it first)")
        if not self._exact[src]:
            raise OQError(f"fork: the host holds only an upper bound of sequence {src}'s length (set_lengths with Python ints)")
        n = self._bound[src]
        full, part = n // self.page_size, 1 if n % self.page_size else 0
        own = [pg for pg in self._pages[dst] if self.allocator.refcount(pg) == 1]
        if part > self.allocator.n_free + len(own):
            raise OQError(f"{self!r}: fork needs a page for the partial last page, none is free")
        self._tree_pending = None
        self.allocator.release(self._pages[dst])
        shared = self._pages[src][:full]
        self.allocator.retain(shared)
        self._pages[dst] = list(shared)
        if part:
            (new,) = self.allocator.alloc(1)
            self._copy_page(self._pages[src][full], new)
            self._pages[dst].append(new)
        self._upload()
        self.lengths[dst:dst + 1].copy_(self.lengths[src:src + 1])
        self._bound[dst] = n

    def sequence(self, b):
        """(k, v) of sequence b as [nkv, lengths[b], hd] copies in `dtype`, gathered from its pages (a code cache's are
        dequantised by unpack_codes).  The one call that reads a length back from the device: for tests and debugging."""
        b = operator.index(b)
        if not 0 <= b < self.bs:
            raise IndexError(f"sequence {b} of a batch of {self.bs}")
        n = min(max(int(self.lengths[b]), 0), len(self._pages[b]) * self.page_size)
        idx = torch.tensor(self._pages[b][:self._need(n)], dtype=torch.int64, device=self.device)

        def rows(t):                                        # [pages, nkv, PS, x] -> [nkv, n, x]
            return t[idx].transpose(0, 1).reshape(self.nkv, -1, t.shape[3])[:, :n]
        if self.code_bits is None:
            return rows(self.k).clone(), rows(self.v).clone()
        return tuple(unpack_codes(rows(c), rows(m), self.code_bits).to(self.dtype)
                     for c, m in ((self.k_codes, self.k_meta), (self.v_codes, self.v_meta)))

    # ---- the (k, v) tuple surface: refused, as for every ragged cache ------------------------------------------------------------
    def _no_tuple(self, what):
        raise OQError(f"{what}: a ragged cache has no common length, hence no [bs, nkv, length, hd] tensors; "
                      "sequence(b) gives one sequence's rows")

    def __len__(self):
        return 2

    def __getitem__(self, i):
        self._no_tuple("indexing")

    def __iter__(self):
        self._no_tuple("iteration")

    def dequantize(self):
        self._no_tuple("dequantize")

    def to_tuple(self):
        self._no_tuple("to_tuple")

    def clone(self):
        c = PagedKVCache(self.bs, self.nkv, self.hd, self.dtype, self.device, self.num_pages, self.page_size, self.max_pages,
                         code_bits=self.code_bits)
        for name in self._buffers():
            getattr(c, name).copy_(getattr(self, name))
        c.allocator = self.allocator.clone()
        c._pages, c._bound, c._exact, c.length = [list(p) for p in self._pages], list(self._bound), list(self._exact), self.length
        c.page_table.copy_(self.page_table)
        c.lengths.copy_(self.lengths)
        return c

    def __repr__(self):
        return (f"PagedKVCache(bs={self.bs}, nkv={self.nkv}, hd={self.hd}, dtype={self.dtype}, length={self.length}, paged: "
                f"page_size={self.page_size}, {self.allocator.n_free} of {self.num_pages} pages free, max_pages={self.max_pages}"
                + ("" if self.code_bits is None else f", code_bits={self.code_bits}") + ")")


class SwappedSequence:
    """One sequence of a PagedKVPool in host memory (PagedKVPool.swap_out): `length` rows in `n_pages` pages, the pool's
    geometry (layers, nkv, hd, page_size, dtype, code_bits) and, per buffer kind of the pool ("k", "v" or "k_codes", "v_codes",
    "k_meta", "v_meta"), `buffers[kind]`: one PINNED uint8 host tensor [layers, n_pages, page_bytes] holding the raw bytes of
    the sequence's pages in row order -- page_bytes = nkv * page_size * bytes of one row of that kind.  `event` is recorded
    behind the last device-to-host copy on `stream`: the bytes are complete once it has passed (swap_in waits for it on another
    stream; a host reader calls event.synchronize()).  The handle is never consumed: it can be swapped into any empty slot of
    any pool of the same geometry, any number of times."""

    def __init__(self, length, n_pages, geometry, buffers, event, stream):
        self.length, self.n_pages, self.geometry, self.buffers, self.event, self.stream = length, n_pages, geometry, buffers, event, stream

    @property
    def nbytes(self):
        return sum(t.numel() for t in self.buffers.values())

    def __repr__(self):
        return f"SwappedSequence(length={self.length}, n_pages={self.n_pages}, nbytes={self.nbytes}, geometry={self.geometry})"


class _PoolLayer(PagedKVCache):
    """Layer l of a PagedKVPool, what layer l's block receives as past_key_value: a PagedKVCache that allocates nothing.  Its
    pools are pool.<buffer>[l] (contiguous, so the kernels are the per-layer cache's), its page_table and lengths the pool's
    shared tensors, and length, the pages and the allocator are read through to the pool.  reserve() and book_step(), which
    the block forward calls, take part in the pool's step protocol; everything that changes the sequences (set_lengths, fork,
    swap) is called on the pool."""

    def __init__(self, pool, l):
        self.pool, self.index = pool, l
        self.bs, self.nkv, self.hd, self.dtype, self.device = pool.bs, pool.nkv, pool.hd, pool.dtype, pool.device
        self.num_pages, self.page_size, self.max_pages, self.code_bits = pool.num_pages, pool.page_size, pool.max_pages, pool.code_bits
        self.lengths, self.page_table = pool.lengths, pool.page_table
        for name in pool._buffers():
            setattr(self, name, getattr(pool, name)[l])

    length = property(lambda self: self.pool.length)
    allocator = property(lambda self: self.pool.allocator)
    _pages = property(lambda self: self.pool._pages)

    def reserve(self, n):
        self.pool._layer_reserve(self.index, int(n))

    def book_step(self, Tq, new_tokens):
        self.pool._layer_book(self.index, int(Tq), new_tokens)

    def book_tree_step(self, Tq):
        self.pool._layer_book(self.index, int(Tq), (None, None, None), tree=True)

    def commit_tree(self, tree, accept):
        self._on_the_pool("commit_tree")

    _tree_pending = property(lambda self: self.pool._tree_pending)

    def _on_the_pool(self, what):
        raise OQError(f"{what}: layer {self.index} is a view of {self.pool!r}; call it on the pool, for all layers at once")

    def advance(self, rows, counts=None, exact=True):
        self._on_the_pool("advance")

    def set_lengths(self, lengths, bound=None):
        self._on_the_pool("set_lengths")

    def fork(self, src, dst):
        self._on_the_pool("fork")

    def clone(self):
        self._on_the_pool("clone")

    def __repr__(self):
        return f"layer {self.index} of {self.pool!r}"


class PagedKVPool(PagedKVCache):
    """The paged KV cache of a whole model: `layers` layers share ONE PageAllocator, one host mirror, one page_table int32
    [bs, max_pages], one `lengths` int32 [bs] on the device and one host bound `length`.  Storage per buffer kind is one tensor
    with a leading layer dimension -- k / v [layers, num_pages, nkv, page_size, hd], with code_bits 4 / 8 k_codes / v_codes /
    k_meta / v_meta in PagedKVCache's shapes behind `layers` -- and a page id names the same slot in every layer.  The
    arguments are PagedKVCache's, checked and refused as it does.  The host side IS PagedKVCache's (reserve, advance,
    set_lengths, fork, pages, n_free, nbytes and the sharing invariant), applied to every layer at once: a shared page has
    reference count 2 once, and the page copies of set_lengths and fork are one ops.kv_pages_copy launch per buffer kind for all
    layers.

    layer(l) is the view layer l's block receives as past_key_value.  Step protocol: in a model step every layer's block forward
    runs exactly once, in any order, with the same step rows Tq and the same new_tokens.  The first view whose reserve(Tq) is
    called does the pool's reserve -- one host loop over the batch, at most one table upload -- and the others only check their
    Tq.  After its attention a view books its step; when the last of the `layers` views has, the pool applies the step once
    (lengths, length, the host bounds, the pad-row trim of PagedKVCache.advance).  Until then every view reads the pre-step
    length and lengths; all launches are on one stream, which orders them.  A view that steps twice before the others, a Tq
    or new_tokens that differs from the step's first layer, a tree step (tree=) in one layer and a normal one in another, and set_lengths / fork / swap_* in mid-step raise OQError and leave
    the pool unchanged; abort_step() discards the bookings of an unfinished step.  new_tokens given as a device tensor must be
    the same tensor object for every layer (its values are never read).

    swap_out(b) moves a sequence to pinned host memory and frees its pages, swap_in(b, handle) brings one back into fresh
    private pages: a gather / scatter launch per buffer kind (ops.kv_pages_gather / kv_pages_scatter) through a device staging
    buffer of swap_staging_bytes, allocated at the first swap and kept, and non-blocking copies between it and the host; the
    kernels touch device memory only.  No call of the step path, and neither swap, reads the device (a swap may block in the
    host allocator, see swap_out).  reserve() and advance() are the step protocol's own (the views call them through the
    pool) and are refused in mid-step when called directly."""

    def __init__(self, layers, bs, nkv, hd, dtype, device, num_pages, page_size=16, max_pages=None, code_bits=None,
                 swap_staging_bytes=64 << 20):
        layers = operator.index(layers)
        if layers <= 0:
            raise OQError(f"PagedKVPool: layers {layers}")
        super().__init__(bs, nkv, hd, dtype, device, num_pages, page_size, max_pages, code_bits, _lead=(layers,))
        self.layers = layers
        biggest = max(self._page_bytes(n) for n in self._buffers())
        if int(swap_staging_bytes) < biggest:
            raise OQError(f"PagedKVPool: swap_staging_bytes {swap_staging_bytes} below one page of one layer ({biggest} bytes)")
        self.swap_staging_bytes = int(swap_staging_bytes)
        self._staging = None
        self._step = None                   # an unfinished model step: Tq, the layers that reserved / booked, its new_tokens
        self._copies = []                   # (src, dst) page copies queued by set_lengths / fork for one launch
        self._views = [_PoolLayer(self, l) for l in range(layers)]

    def layer(self, l):
        """The view of layer l (created once): what layer l's block receives as past_key_value."""
        l = operator.index(l)
        if not 0 <= l < self.layers:
            raise IndexError(f"layer {l} of {self.layers}")
        return self._views[l]

    def _page_bytes(self, name):
        t = getattr(self, name)
        return t[0, 0].numel() * t.element_size()

    # ---- the step protocol ---------------------------------------------------------------------------------------------------
    def _layer_reserve(self, l, Tq):
        st = self._step
        if st is None:
            self.reserve(Tq)                # all or nothing: a refusal opens no step
            self._step = {"Tq": Tq, "reserved": {l}, "booked": set(), "tokens": None, "tree": None}
            return
        if l in st["reserved"]:
            raise OQError(f"{self!r}: layer {l} steps twice in one model step ({len(st['booked'])} of {self.layers} layers have "
                          "booked it; abort_step() discards an unfinished step)")
        if Tq != st["Tq"]:
            raise OQError(f"{self!r}: layer {l} steps {Tq} rows, the step's first layer {st['Tq']}")
        st["reserved"].add(l)

    @staticmethod
    def _same_tokens(a, b):
        (ca, ga, ha), (cb, gb, hb) = a, b
        if ha is not None or hb is not None:
            return ha == hb and ga == gb
        return ca is cb and ga == gb

    def _layer_book(self, l, Tq, new_tokens, tree=False):
        st = self._step
        if st is None or l not in st["reserved"] or l in st["booked"] or Tq != st["Tq"]:
            raise OQError(f"{self!r}: layer {l} books a step of {Tq} rows it has not reserved")
        if st["tree"] is not None and st["tree"] != tree:
            raise OQError(f"{self!r}: layer {l} books a {'tree' if tree else 'normal'} step, the step's first layer a "
                          f"{'tree' if st['tree'] else 'normal'} one")
        st["tree"] = tree
        if st["tokens"] is not None and not self._same_tokens(st["tokens"], new_tokens):
            raise OQError(f"{self!r}: layer {l}'s new_tokens differ from the step's first layer's")
        if st["tokens"] is None:
            st["tokens"] = tuple(new_tokens)
        st["booked"].add(l)
        if len(st["booked"]) == self.layers:
            self._step = None
            if st["tree"]:
                self._tree_pending = Tq     # a tree step: nothing advances, commit_tree does
            else:
                PagedKVCache.book_step(self, Tq, st["tokens"])

    def abort_step(self):
        """Discard the bookings of an unfinished model step: lengths, length and the host bounds stay the pre-step ones (pages
        its reserve took stay with their sequences, as after PagedKVCache.reserve).  A pending tree step is dropped too."""
        self._step = None
        self._tree_pending = None

    def commit_tree(self, tree, accept):
        """PagedKVCache.commit_tree for every layer at once, after the tree step of all layers: one ops.kv_tree_commit launch
        per buffer kind.  Refused in mid-step."""
        self._idle("commit_tree")
        super().commit_tree(tree, accept)

    def _idle(self, what):
        if self._step is not None:
            st = self._step
            raise OQError(f"{self!r}: {what} in mid-step ({len(st['booked'])} of {self.layers} layers have booked a step of "
                          f"{st['Tq']} rows; abort_step() discards it)")

    def book_step(self, Tq, new_tokens):
        raise OQError(f"{self!r}: the layers' views step (pool.layer(l) as past_key_value), not the pool")

    def reserve(self, n):
        """PagedKVCache.reserve for every layer at once.  The first view of a model step calls it; called directly it is refused
        in mid-step, like every other call that moves the host state behind the step protocol."""
        self._idle("reserve")
        super().reserve(n)

    def advance(self, rows, counts=None, exact=True):
        """PagedKVCache.advance on the pool's host bounds.  The pool calls it when the last layer has booked a step; called
        directly it is refused in mid-step."""
        self._idle("advance")
        super().advance(rows, counts, exact)

    # ---- model-wide set_lengths / fork: PagedKVCache's, the page copies batched into one launch per buffer kind ----------------
    def _copy_page(self, src, dst):
        # a queued copy must not write a page that an earlier queued copy still reads (a source both sharers have left is free
        # again and may be handed out as a destination): launch what is queued first
        if any(dst == s for s, _ in self._copies):
            self._flush_copies()
        self._copies.append((src, dst))

    def _flush_copies(self):
        from . import ops
        pairs, self._copies = self._copies, []
        if not pairs:
            return
        ids = torch.tensor(pairs, dtype=torch.int32).t().contiguous().to(self.device, non_blocking=True)
        for name in self._buffers():
            ops.kv_pages_copy(getattr(self, name), ids[0], ids[1])

    def set_lengths(self, lengths, bound=None):
        """PagedKVCache.set_lengths for every layer at once."""
        self._idle("set_lengths")
        try:
            super().set_lengths(lengths, bound)
            self._flush_copies()
        finally:
            self._copies = []               # (after an exception: never launch stale pairs on pages that changed owner)

    def fork(self, src, dst):
        """PagedKVCache.fork for every layer at once: the shared pages gain one reference, not one per layer."""
        self._idle("fork")
        try:
            super().fork(src, dst)
            self._flush_copies()
        finally:
            self._copies = []

    # ---- swap to host --------------------------------------------------------------------------------------------------------
    @property
    def geometry(self):
        return (self.layers, self.nkv, self.hd, self.page_size, self.dtype, self.code_bits)

    def _chunks(self, name, n):
        """The (layer range, page range) pieces of a transfer of n pages of every layer that fit the staging buffer: whole
        layers while a layer's pages fit, else page ranges of one layer."""
        pb = self._page_bytes(name)
        if n * pb <= self.swap_staging_bytes:
            step = self.swap_staging_bytes // (n * pb)
            return [(l, min(l + step, self.layers), 0, n) for l in range(0, self.layers, step)]
        step = self.swap_staging_bytes // pb
        return [(l, l + 1, p, min(p + step, n)) for l in range(self.layers) for p in range(0, n, step)]

    def _stage(self):
        if self._staging is None:
            self._staging = torch.empty(self.swap_staging_bytes, dtype=torch.uint8, device=self.device)
        return self._staging

    def _slot(self, what, b):
        b = operator.index(b)
        if not 0 <= b < self.bs:
            raise OQError(f"{what}: sequence {b} of a batch of {self.bs}")
        return b

    def swap_out(self, b):
        """Move sequence b to host memory: all ceil(length / page_size) pages of every layer, shared ones included, are gathered
        into the staging buffer and copied to a SwappedSequence's pinned tensors (in chunks when they exceed the staging buffer;
        stream order makes its reuse safe); then b's references are released, lengths[b] and its host bound become 0 and the
        table is uploaded.  The host must know b's length exactly (as fork needs it).  Nothing here reads the device, and the
        handle's event tells when the bytes have arrived.  The call can still block on the host: the page ids go up from
        pageable memory (the runtime stages such a copy, as for the table upload), and the first handle of a size allocates
        pinned host memory, which later ones of that size find in torch's pinned-memory cache."""
        from . import ops
        self._idle("swap_out")
        b = self._slot("swap_out", b)
        if not self._exact[b]:
            raise OQError(f"swap_out: the host holds only an upper bound of sequence {b}'s length (set_lengths with Python ints)")
        length = self._bound[b]
        n = self._need(length)
        ids = torch.tensor(self._pages[b][:n], dtype=torch.int32).to(self.device, non_blocking=True)
        buffers = {}
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream()
            for name in self._buffers():
                pool, pb = getattr(self, name), self._page_bytes(name)
                host = torch.empty((self.layers, n, pb), dtype=torch.uint8, pin_memory=True)
                for l0, l1, p0, p1 in (self._chunks(name, n) if n else ()):
                    stage = self._stage()[:(l1 - l0) * (p1 - p0) * pb]
                    ops.kv_pages_gather(pool[l0:l1], ids[p0:p1], stage)
                    host[l0:l1, p0:p1].copy_(stage.view(l1 - l0, p1 - p0, pb), non_blocking=True)
                buffers[name] = host
            event = torch.cuda.Event()
            event.record(stream)
        self._tree_pending = None
        self.allocator.release(self._pages[b])
        self._pages[b] = []
        self._bound[b] = 0
        self.lengths[b:b + 1].zero_()
        self._upload()
        return SwappedSequence(length, n, self.geometry, buffers, event, stream)

    def swap_in(self, b, handle):
        """Bring a swapped-out sequence into slot b, which must be empty with its length known to the host: n_pages fresh
        private pages (all or nothing), the handle's bytes copied host -> staging and scattered into the pages of every layer,
        lengths[b] and the host bound set to the handle's length (`length` grows to it if it is below), the table uploaded.
        Sharing is not restored: the sequence owns all its pages.  The handle stays valid.  A geometry that differs, a slot
        that is not empty and a pool without the pages raise OQError before anything changes."""
        from . import ops
        self._idle("swap_in")
        b = self._slot("swap_in", b)
        if not isinstance(handle, SwappedSequence):
            raise OQError(f"swap_in: expected a SwappedSequence, got {type(handle).__name__}")
        if handle.geometry != self.geometry:
            raise OQError(f"swap_in: {handle!r} does not fit the geometry {self.geometry} of {self!r}")
        if self._bound[b] != 0 or not self._exact[b]:
            raise OQError(f"swap_in: sequence {b} is not empty (set_lengths with 0 for it first)")
        n = handle.n_pages
        if n > self.max_pages:
            raise OQError(f"{self!r}: swap_in of {handle.length} rows takes sequence {b} beyond max_pages = {self.max_pages}")
        own = [pg for pg in self._pages[b] if self.allocator.refcount(pg) == 1]
        if n > self.allocator.n_free + len(own):
            raise OQError(f"{self!r}: swap_in needs {n} pages, {self.allocator.n_free + len(own)} are free")
        self._tree_pending = None
        self.allocator.release(self._pages[b])
        self._pages[b] = self.allocator.alloc(n)
        ids = torch.tensor(self._pages[b], dtype=torch.int32).to(self.device, non_blocking=True)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream()
            if stream != handle.stream:
                stream.wait_event(handle.event)
            for name in self._buffers():
                pool, pb, host = getattr(self, name), self._page_bytes(name), handle.buffers[name]
                for l0, l1, p0, p1 in (self._chunks(name, n) if n else ()):
                    stage = self._stage()[:(l1 - l0) * (p1 - p0) * pb]
                    stage.view(l1 - l0, p1 - p0, pb).copy_(host[l0:l1, p0:p1], non_blocking=True)
                    ops.kv_pages_scatter(stage, pool[l0:l1], ids[p0:p1])
        self.lengths[b:b + 1].copy_(torch.tensor([handle.length], dtype=torch.int32), non_blocking=True)
        self._bound[b] = handle.length
        self.length = max(self.length, handle.length)
        self._upload()

    # ---- the rest of the surface ---------------------------------------------------------------------------------------------
    def sequence(self, b):
        raise OQError(f"{self!r}: sequence(b) is a layer's (pool.layer(l).sequence(b))")

    def clone(self):
        self._idle("clone")
        c = PagedKVPool(self.layers, self.bs, self.nkv, self.hd, self.dtype, self.device, self.num_pages, self.page_size,
                        self.max_pages, code_bits=self.code_bits, swap_staging_bytes=self.swap_staging_bytes)
        for name in self._buffers():
            getattr(c, name).copy_(getattr(self, name))
        c.allocator = self.allocator.clone()
        c._pages, c._bound, c._exact, c.length = [list(p) for p in self._pages], list(self._bound), list(self._exact), self.length
        c.page_table.copy_(self.page_table)
        c.lengths.copy_(self.lengths)
        return c

    def __repr__(self):
        return (f"PagedKVPool(layers={self.layers}, bs={self.bs}, nkv={self.nkv}, hd={self.hd}, dtype={self.dtype}, "
                f"length={self.length}, paged: page_size={self.page_size}, {self.allocator.n_free} of {self.num_pages} pages free, "
                f"max_pages={self.max_pages}" + ("" if self.code_bits is None else f", code_bits={self.code_bits}") + ")")
