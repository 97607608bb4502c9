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

ragged=True (either kind): every sequence of the batch has its own length.  `lengths` is an int32 [bs] tensor ON THE DEVICE,
which the append and the attention kernels read themselves (ops.kv_append(..., lengths=), ops.decode_attention(..., lengths=)):
sequence b's valid rows are [0, lengths[b]), a step needs no padding mask and no position tensor, and nothing about its
launches depends on a length the host would have to read back.  `length` stays a host int, now an UPPER BOUND of
lengths.max(): it sizes the buffers and the attention's split plan.  Rows of a sequence at or beyond its own length are
scratch.  There is no common length, so the (k, v) tuple surface is refused; sequence(b) gives one sequence's rows.
"""
import operator

import torch

from ._capi import OQError

_DTYPES = (torch.bfloat16, torch.float32)


def unpack_codes(codes, meta):
    """float32 [..., hd] values of code rows uint8 [..., hd // 2] under meta float32 [..., 2] = (scale, zero-point): dim 2i is
    the low nibble of byte i, dim 2i + 1 its high nibble, value = (code - zp) * scale with the subtraction and the multiply in
    float32.  Pure torch (any device): the value contract of the code cache, as PackedLinear.dequantize() is of the weights."""
    c = torch.stack((codes & 0xF, codes >> 4), dim=-1).reshape(*codes.shape[:-1], 2 * codes.shape[-1]).to(torch.float32)
    return (c - meta[..., 1:2]) * meta[..., 0:1]


class PackedKVCache:
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
        if code_bits is not None and code_bits != 4:
            raise OQError(f"PackedKVCache: code_bits {code_bits} (None: float rows, or 4)")
        if code_bits == 4 and self.hd not in (64, 128):
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
                t = torch.empty(shape + (self.hd // 2,), dtype=torch.uint8, device=self.device)
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
        return tuple(unpack_codes(c[b, :, :n], m[b, :, :n]).to(self.dtype)
                     for c, m in ((self.k_codes, self.k_meta), (self.v_codes, self.v_meta)))

    def dequantize(self):
        """(k, v) as [bs, nkv, length, hd] tensors in `dtype`.  On a code cache these are fresh copies computed by
        unpack_codes (the value contract; one rounding to bfloat16 when that is the dtype); on a float cache, the views."""
        self._no_tuple("dequantize")
        if self.code_bits is None:
            return self.k[:, :, :self.length], self.v[:, :, :self.length]
        n = self.length
        return tuple(unpack_codes(c[:, :, :n], m[:, :, :n]).to(self.dtype)
                     for c, m in ((self.k_codes, self.k_meta), (self.v_codes, self.v_meta)))

    def reserve(self, n):
        """Room for n more rows: the capacity grows geometrically (at least doubling) and the valid rows move to the new
        buffers.  A cache sized to prompt + max_new_tokens up front never reallocates."""
        need = self.length + int(n)
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
        if code_bits is not None and head_bits != code_bits:
            raise OQError(f"past_key_value: a {code_bits}-bit code cache holds rows quantised on that grid (head_bits {head_bits})")
        c = cls(bs, nkv, hd, dtype or k.dtype, k.device, max(int(capacity or 0), T), code_bits=code_bits)
        if T and head_bits is not None:
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
