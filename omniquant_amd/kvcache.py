"""Per-layer KV cache of the packed (real-quant) blocks.

K and V live in preallocated [bs, nkv, cap, hd] buffers in the block's compute dtype (bfloat16 or float32); a forward with a
past appends its rows in place (ops.kv_append, csrc/oq_decode.hip) and attends over rows [0, length) (ops.decode_attention).
The object stands in for the reference's `past_key_value` 2-tuple (models/int_llama_layer.py:121-135,177, transformers 4.31):
len() == 2, iteration and indexing give the [bs, nkv, length, hd] views, so `past[0].shape[2]` is the past length and
`k, v = cache` works.  Unlike a tuple it is appended to IN PLACE, as later transformers' DynamicCache is: the block returns
the same object as `present`.
"""
import operator

import torch

from ._capi import OQError

_DTYPES = (torch.bfloat16, torch.float32)


class PackedKVCache:
    def __init__(self, bs, nkv, hd, dtype, device, capacity=0):
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
        self.length = 0
        self.k = torch.empty((self.bs, self.nkv, int(capacity), self.hd), dtype=dtype, device=device)
        self.v = torch.empty_like(self.k)

    @property
    def capacity(self):
        return self.k.shape[2]

    def reserve(self, n):
        """Room for n more rows: the capacity grows geometrically (at least doubling) and the valid rows move to the new
        buffers.  A cache sized to prompt + max_new_tokens up front never reallocates."""
        need = self.length + int(n)
        if need <= self.capacity:
            return
        cap = max(need, 2 * self.capacity, 16)
        k = torch.empty((self.bs, self.nkv, cap, self.hd), dtype=self.dtype, device=self.device)
        v = torch.empty_like(k)
        if self.length:
            k[:, :, :self.length].copy_(self.k[:, :, :self.length])
            v[:, :, :self.length].copy_(self.v[:, :, :self.length])
        self.k, self.v = k, v

    # ---- the reference's (k, v) tuple surface ------------------------------------------------------------------------------
    def __len__(self):
        return 2

    def __getitem__(self, i):
        if isinstance(i, slice):
            return (self[0], self[1])[i]
        i = operator.index(i)
        if i < 0:
            i += 2
        if i not in (0, 1):
            raise IndexError("PackedKVCache index out of range (0 = keys, 1 = values)")
        return (self.k if i == 0 else self.v)[:, :, :self.length]

    def __iter__(self):
        yield self[0]
        yield self[1]

    def __repr__(self):
        return (f"PackedKVCache(bs={self.bs}, nkv={self.nkv}, hd={self.hd}, dtype={self.dtype}, length={self.length}, "
                f"capacity={self.capacity})")

    @classmethod
    def from_tuple(cls, kv, dtype=None, capacity=None, head_bits=None):
        """A cache holding copies of the reference-layout (k, v), each [bs, nkv, T, hd] (any float dtype, converted once);
        the tensors passed in are never modified.  head_bits (W4A4 blocks): the rows are quantised per (token, head) over hd on
        that grid as they are imported (ops.kv_append_quant without rotation), which is what the block's own appends store."""
        if len(kv) != 2:
            raise OQError(f"past_key_value: expected (k, v), got {len(kv)} tensors")
        k, v = kv
        if not (torch.is_tensor(k) and torch.is_tensor(v)) or k.dim() != 4 or tuple(k.shape) != tuple(v.shape):
            raise OQError("past_key_value: k and v must be [bs, nkv, T, hd] tensors of one shape")
        if not (k.is_cuda and v.is_cuda):
            raise OQError("past_key_value: GPU tensors expected (no CPU fallback)")
        bs, nkv, T, hd = k.shape
        c = cls(bs, nkv, hd, dtype or k.dtype, k.device, max(int(capacity or 0), T))
        if T and head_bits is not None:
            from . import ops
            src = c.dtype if k.dtype == c.dtype else torch.float32
            kt, vt = (t.transpose(1, 2).to(src).contiguous() for t in (k, v))         # [bs, T, nkv, hd], fresh copies
            ops.kv_append_quant(kt, vt, head_bits, c.dtype, k_cache=c.k, v_cache=c.v, past=0)
        elif T:
            c.k[:, :, :T].copy_(k)
            c.v[:, :, :T].copy_(v)
        c.length = T
        return c

    def to_tuple(self):
        """(k, v) as contiguous [bs, nkv, length, hd] copies (the reference's layout)."""
        return tuple(t.clone(memory_format=torch.contiguous_format) for t in self)

    def clone(self):
        c = PackedKVCache(self.bs, self.nkv, self.hd, self.dtype, self.device, self.capacity)
        if self.length:
            c.k[:, :, :self.length].copy_(self.k[:, :, :self.length])
            c.v[:, :, :self.length].copy_(self.v[:, :, :self.length])
        c.length = self.length
        return c
