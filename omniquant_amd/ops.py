"""torch.autograd.Function wrappers around the C ABI (include/oq_hip.h).

Each Function's forward AND backward are hand-written HIP kernels; PyTorch only allocates the outputs and keeps
the graph.  Activations are float32 (parity mode: exact-f32 MFMA) or bfloat16 (production: bf16 MFMA).
"""
import math
import ctypes
import os

import torch

from . import _capi as C


def _empty_like(t, dtype=None):
    return torch.empty(t.shape, dtype=dtype or t.dtype, device=t.device)


def _f32(t):
    """float32 contiguous view/copy of a small parameter vector (plumbing)."""
    if t is None:
        return None
    t = t.detach() if not t.requires_grad else t
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


# ------------------------------------------------------------------------------------------------------
# UniformAffineQuantizer core (+ LET weight re-parameterisation)
# ------------------------------------------------------------------------------------------------------
class WgradQueue:
    """Deferred weight-gradient GEMMs of one backward pass.  The four wgrads of a block (q | k | v, o, gate | up, down) are
    independent of the rest of the backward chain -- only the weight quantisers' backward reads them -- so, when `enabled` (the
    calibration step sets it), the Linear nodes park them here and they run as ONE grouped launch when the backward pass ends
    (oq_wgrad_group: the tiles of all of them fill whole rounds of the CUs instead of four ragged last rounds).  A consumer that
    meets a parked gradient (`pending(t)`) either parks its own launch behind the group (`after`) or calls `flush()` first.
    Only weights that come out of FakeQuantFn (`_oq_fq_out`) are parked: its backward knows the protocol.
    OFF by default (OQ_WGRAD_GROUP=1 switches it on): measured same-box, LLaMA-2-13B gains 0.55 % (gate | up + o_proj = exactly
    10 rounds instead of 9 + 2) and LLaMA-7B loses 0.7 % -- its 2064 tiles of down_proj + gate | up are 8 rounds + 16 tiles, the
    peeled strip costs 31 us of the 53 us round it saves, the mixed launch runs 4 % slower per round, and a parked gradient
    reaches its weight quantiser's backward from HBM instead of the Infinity Cache."""
    enabled = False
    items = []        # (gy2, x2, gw, N, K, T, ld_gy, ld_x, ld_gw, gy_off)
    ranges = []       # [lo, hi) device addresses of the parked outputs
    after = []        # (entry point, args, keep-alive) launches that read parked outputs

    @staticmethod
    def on():
        return WgradQueue.enabled and os.environ.get("OQ_WGRAD_GROUP", "0") != "0"

    @staticmethod
    def park(gy2, x2, gw, N, K, T, ld_gy, ld_x, ld_gw, gy_off=0):
        if not WgradQueue.items and not WgradQueue.after:
            torch.autograd.Variable._execution_engine.queue_callback(WgradQueue.flush)
        WgradQueue.items.append((gy2, x2, gw, int(N), int(K), int(T), int(ld_gy), int(ld_x), int(ld_gw), int(gy_off)))
        WgradQueue.ranges.append((gw.data_ptr(), gw.data_ptr() + gw.numel() * gw.element_size()))
        # Launch as soon as the parked tiles make (nearly) whole rounds of the CUs: a gradient that waits longer than it must
        # is read by its weight quantiser's backward from HBM instead of from the Infinity Cache (measured: parking all four
        # until the pass ends loses what the fuller rounds gain).  LLaMA-7B: down_proj (688 tiles) waits for gate | up (1376):
        # 2064 = 8 rounds + one tile column; o_proj (256) and q | k | v (768) are whole rounds and go at once.
        tiles = sum(-(-it[3] // 256) * -(-it[4] // 256) for it in WgradQueue.items)
        rem = tiles % _n_cus()
        if rem == 0 or rem <= _n_cus() // 4:
            WgradQueue.flush()

    @staticmethod
    def pending(t):
        if t is None or not WgradQueue.ranges:
            return False
        p = t.data_ptr()
        return any(lo <= p < hi for lo, hi in WgradQueue.ranges)

    @staticmethod
    def flush():
        items, after = WgradQueue.items, WgradQueue.after
        WgradQueue.items, WgradQueue.after, WgradQueue.ranges = [], [], []
        if items:
            arr = (C.WgradItem * len(items))()
            for i, (gy2, x2, gw, N, K, T, ld_gy, ld_x, ld_gw, off) in enumerate(items):
                arr[i] = C.WgradItem(gy2.data_ptr() + off * gy2.element_size(), x2.data_ptr(), gw.data_ptr(), N, K, T, ld_gy, ld_x, ld_gw)
            ws_bytes = C.size_call("oq_wgrad_group_workspace", ctypes.addressof(arr), len(items))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=items[0][2].device)
            C.call("oq_wgrad_group", ctypes.addressof(arr), len(items), ws.data_ptr(), ws_bytes, C.stream())
        for name, args, _keep in after:
            C.call(name, *args, C.stream())

    @staticmethod
    def drop():
        WgradQueue.items, WgradQueue.after, WgradQueue.ranges = [], [], []


_N_CUS = [0]


def _n_cus():
    if not _N_CUS[0]:
        _N_CUS[0] = int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count) or 256
    return _N_CUS[0]


def wgrad(gy2, x2, gw, N, K, T, ld_gy, ld_x, ld_gw, gy_off=0, park=False):
    """gw[N, K] = gy2[T, gy_off : gy_off + N]^T @ x2[T, K] (both operands k-strided); parked in the WgradQueue when the caller
    allows it (the weight came out of FakeQuantFn) and a calibration step is collecting them."""
    if park and WgradQueue.on() and gw.dtype == torch.bfloat16 and gy2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16:
        WgradQueue.park(gy2, x2, gw, N, K, T, ld_gy, ld_x, ld_gw, gy_off)
    else:
        gemm(gy2, x2, gw, N, K, T, ld_gy, ld_x, ld_gw, False, False, a_off=gy_off)


class WeightQuantBatch:
    """`with WeightQuantBatch():` -- the FakeQuantFn calls made inside (the LET weights of one shape: q, k, v, o) are launched
    as ONE multi-matrix kernel when the block ends (oq_fakequant_fwd_multi), and their backward calls as one launch plus one
    launch for all column reductions (oq_fakequant_bwd_multi) once the last of them has arrived -- or when
    `flush_pending()` is called (optim.GradCollector.flush does, before anything reads the gradients).  Same kernels'
    arithmetic, same values; four 67 MB problems stop paying ramp-up, tail and launch gap four times.  OQ_WQ_BATCH=0: off."""
    active = None
    pending = []          # batches whose backward has started but is not launched yet

    def __init__(self):
        self.fwd, self.bwd, self.keep = [], [], []
        self.shape = None
        self.enabled = os.environ.get("OQ_WQ_BATCH", "1") != "0"

    def takes(self, w, cols, seg, col_mul, row_div, row_mul, shift):
        if not self.enabled or seg != cols or w.dim() != 2 or len(self.fwd) >= 4:
            return False
        if col_mul is None and row_div is None and row_mul is None and shift is None:
            return False
        key = (tuple(w.shape), w.dtype, w.device)
        if self.shape is None:
            self.shape = key
        return self.shape == key

    def add_forward(self, args, keep):
        self.fwd.append(args)
        self.keep.append(keep)

    def __enter__(self):
        if WeightQuantBatch.active is not None:
            raise C.OQError("WeightQuantBatch does not nest")
        WeightQuantBatch.active = self
        return self

    def __exit__(self, *exc):
        WeightQuantBatch.active = None
        if self.fwd and exc[0] is None:
            arr = (C.FakeQuantFwdArgs * len(self.fwd))()
            for i, a in enumerate(self.fwd):
                arr[i] = C.FakeQuantFwdArgs(*a)
            C.call("oq_fakequant_fwd_multi", ctypes.addressof(arr), len(self.fwd), C.stream())
        self.n = len(self.fwd)
        self.fwd, self.keep = [], []
        return False

    def add_backward(self, args, keep):
        if not self.bwd:
            WeightQuantBatch.pending.append(self)
            # the deferred launch goes to the stream the siblings' buffers were produced on (with OQ_WEIGHT_STREAM=1 that is the
            # block's side stream, not the stream of whoever flushes): the caching allocator then cannot hand `keep`'s buffers,
            # released right after the launch, to work that is ordered before it
            self.stream = torch.cuda.current_stream()
            # a sibling that needs no gradient never arrives: whatever is still queued goes out when this backward pass ends
            torch.autograd.Variable._execution_engine.queue_callback(WeightQuantBatch.flush_pending)
        self.bwd.append(args)
        self.keep.append(keep)
        if len(self.bwd) == self.n and not WgradQueue.items:      # (parked weight gradients: wait for flush_pending)
            self.flush_backward()

    def flush_backward(self):
        if self in WeightQuantBatch.pending:
            WeightQuantBatch.pending.remove(self)
        if self.bwd:
            arr = (C.FakeQuantBwdArgs * len(self.bwd))()
            for i, a in enumerate(self.bwd):
                arr[i] = C.FakeQuantBwdArgs(*a)
            st = getattr(self, "stream", None) or torch.cuda.current_stream()
            cur = torch.cuda.current_stream()
            if st != cur:
                st.wait_stream(cur)           # the last sibling's gradient may have been produced on the flusher's stream
            C.call("oq_fakequant_bwd_multi", ctypes.addressof(arr), len(self.bwd), st.cuda_stream)
            if st != cur:
                cur.wait_stream(st)           # the outputs feed the optimiser arena, read on the flusher's stream
        self.bwd, self.keep = [], []

    @staticmethod
    def flush_pending():
        WgradQueue.flush()              # parked weight gradients first: the launches below read them
        for b in list(WeightQuantBatch.pending):
            b.flush_backward()

    @staticmethod
    def drop_stale():
        """Start of a new step: a backward pass that raised may have left batches queued whose buffers are gone -- forget
        them instead of launching them with the next flush."""
        for b in WeightQuantBatch.pending:
            b.bwd, b.keep = [], []
        WeightQuantBatch.pending = []
        WeightQuantBatch.active = None
        WgradQueue.drop()


class FakeQuantFn(torch.autograd.Function):
    """y = fake_quant(((w*col_mul)/row_div)*row_mul) over segments of `seg`; wshift = w @ shift.

    Reference: quantize/quantizer.py:84-147 and models/transformation.py:24-69.  `stash` (dict) receives the
    non-differentiable side outputs 'scale' and 'zp' ([rows*cols/seg, 1] f32)."""

    @staticmethod
    def forward(ctx, w, col_mul, row_div, row_mul, shift, up, low, nbits, seg, symmetric, out_dtype, stash, out=None, src=None):
        """src: float32 tensor of w's shape holding the same values un-rounded (`_oq_wide`): the kernels read it in place of w;
        the gradient returned for w keeps w's dtype."""
        ctx.in_dtype = w.dtype
        if src is not None:
            if src.dtype != torch.float32 or src.shape != w.shape or src.device != w.device:
                raise C.OQError("FakeQuantFn: `src` must be a float32 tensor of the input's shape")
            w = src
        w = w.contiguous()
        cols = w.shape[-1]
        rows = w.numel() // cols
        nseg = rows * ((cols + seg - 1) // seg)          # a ragged last segment is zero-padded inside the kernel
        ws_out = None
        dest = None
        if isinstance(out, WeightDest):
            dest, ws_out, out = out, out.wshift, out.y
        elif isinstance(out, (tuple, list)):
            out, ws_out = out
        if out is not None:
            # caller-provided destination (a row block of a buffer that stacks sibling weights, see stacked_rows)
            if out.shape != w.shape or out.dtype != out_dtype or out.device != w.device or not out.is_contiguous():
                raise C.OQError("FakeQuantFn: `out` must be a contiguous tensor of the weight's shape and the output dtype")
            y = out
        else:
            y = torch.empty(w.shape, dtype=out_dtype, device=w.device)
        if dest is not None and dest.scale is not None:
            scale, zp = dest.scale, dest.zp              # row blocks of vectors that stack the siblings' (block_common._weight_slabs)
            if tuple(scale.shape) != (nseg, 1) or tuple(zp.shape) != (nseg, 1) or scale.dtype != torch.float32:
                raise C.OQError("FakeQuantFn: scale / zp destinations must be float32 [segments, 1]")
        else:
            scale = torch.empty((nseg, 1), dtype=torch.float32, device=w.device)
            zp = torch.empty((nseg, 1), dtype=torch.float32, device=w.device)
        # integer side channel (IntCodes): asked for through stash["want_int"], produced when the kernels that take this
        # problem can (whole-row segments, grids of at most 8 bits)
        codes = csum = None
        if stash is not None and stash.get("want_int") and int_codes_supported(cols, seg, nbits, not (
                col_mul is None and row_div is None and row_mul is None and shift is None)):
            if dest is not None and dest.codes is not None:
                codes, csum = dest.codes, dest.csum
                if tuple(codes.shape) != (rows, cols) or codes.dtype != torch.int8 or tuple(csum.shape) != (rows,):
                    raise C.OQError("FakeQuantFn: codes / csum destinations must be int8 [rows, cols] / float32 [rows]")
            else:
                codes = torch.empty((rows, cols), dtype=torch.int8, device=w.device)
                csum = torch.empty((rows,), dtype=torch.float32, device=w.device)
        xmin = torch.empty((nseg,), dtype=torch.float32, device=w.device)     # consumed by the backward kernel
        xmax = torch.empty((nseg,), dtype=torch.float32, device=w.device)
        wshift = None
        if shift is not None:
            if ws_out is not None and (ws_out.shape != (rows,) or ws_out.dtype != torch.float32 or not ws_out.is_contiguous()):
                raise C.OQError("FakeQuantFn: the w @ shift destination must be a contiguous float32 vector of `rows` elements")
            wshift = ws_out if ws_out is not None else torch.empty((rows,), dtype=torch.float32, device=w.device)
        cm, rd, rm, sh, u, l = (_f32(t) for t in (col_mul, row_div, row_mul, shift, up, low))
        fargs = (C.ptr(w), C.dt(w), rows, cols, seg, nbits, int(symmetric),
                 C.fptr(cm), C.fptr(rd), C.fptr(rm), C.fptr(sh), C.fptr(u), C.fptr(l),
                 C.ptr(y), C._DT[out_dtype], C.fptr(scale), C.fptr(zp), C.fptr(xmin), C.fptr(xmax), C.fptr(wshift),
                 C.ptr(codes), C.fptr(csum))
        batch = WeightQuantBatch.active
        ctx.batch = None
        if batch is not None and batch.takes(w, cols, seg, col_mul, row_div, row_mul, shift):
            # launched with its siblings when the `with` block ends (one multi-matrix launch); the outputs are not read before
            batch.add_forward(fargs, (w, cm, rd, rm, sh, u, l, y, scale, zp, xmin, xmax, wshift, codes, csum))
            ctx.batch = batch
        else:
            C.call("oq_fakequant_fwd", *fargs, C.stream())
        if stash is not None:
            stash["scale"], stash["zp"] = scale, zp
            if codes is not None:
                stash["int"] = IntCodes(codes, scale.view(-1), zp.view(-1), csum, nbits)
        ctx.save_for_backward(w, cm, rd, rm, sh, u, l, xmin, xmax)
        ctx.cfg = (rows, cols, seg, nbits, int(symmetric))
        # gradient routing set up by optim.BlockOptimizer: single-use learnables (LWC bounds) get their gradient
        # written straight into the arena, shared ones (LET vectors) go through the GradCollector
        ctx.route = [t if (t is not None and getattr(t, "_oq_grad_sink", None) is not None and _gradient_routing_on())
                     else None for t in (col_mul, row_div, row_mul, shift, up, low)]
        if wshift is None:
            wshift = torch.empty((0,), device=w.device)   # placeholder output, never used (no kernel launched)
            ctx.has_wshift = False
        else:
            ctx.has_wshift = True
        ctx.mark_non_differentiable(*([] if ctx.has_wshift else [wshift]))
        return y, wshift

    @staticmethod
    def backward(ctx, gy, gwshift):
        w, cm, rd, rm, sh, u, l, xmin, xmax = ctx.saved_tensors
        rows, cols, seg, nbits, symmetric = ctx.cfg
        need = ctx.needs_input_grad   # w, col_mul, row_div, row_mul, shift, up, low
        dev = w.device
        if gy is None:
            gy = torch.zeros(w.shape, dtype=torch.float32, device=dev)
        gy = gy.contiguous()
        nseg = rows * ((cols + seg - 1) // seg)
        r_cm, r_rd, r_rm, r_sh, r_up, r_low = ctx.route
        g_up = (r_up._oq_grad_sink.view(nseg, 1) if r_up is not None else
                torch.empty((nseg, 1), dtype=torch.float32, device=dev)) if need[5] else None
        g_low = (r_low._oq_grad_sink.view(nseg, 1) if r_low is not None else
                 torch.empty((nseg, 1), dtype=torch.float32, device=dev)) if need[6] else None
        gx = torch.empty(w.shape, dtype=gy.dtype, device=dev) if need[0] else None
        g_cm = torch.empty((cols,), dtype=torch.float32, device=dev) if need[1] else None
        g_rd = torch.empty((rows,), dtype=torch.float32, device=dev) if need[2] else None
        g_rm = torch.empty((rows,), dtype=torch.float32, device=dev) if need[3] else None
        g_sh = None
        gws = None
        if need[4] and ctx.has_wshift:
            g_sh = torch.empty((cols,), dtype=torch.float32, device=dev)
            gws = gwshift.contiguous().float() if gwshift is not None else torch.zeros((rows,), device=dev)
        ws, ws_n = None, 0
        if g_cm is not None or g_sh is not None:
            ws_n = C.size_call("oq_fakequant_bwd_workspace", rows, cols)
            ws = torch.empty((ws_n,), dtype=torch.float32, device=dev)
        bargs = (C.ptr(w), C.dt(w), rows, cols, seg, nbits, symmetric,
                 C.fptr(cm), C.fptr(rd), C.fptr(rm), C.fptr(sh), C.fptr(u), C.fptr(l), C.fptr(xmin), C.fptr(xmax),
                 C.ptr(gy), C.dt(gy), C.fptr(gws), C.fptr(g_up), C.fptr(g_low), C.ptr(gx), C.dt(gy),
                 C.fptr(g_cm), C.fptr(g_sh), C.fptr(g_rd), C.fptr(g_rm), C.fptr(ws), ws_n)
        routed = all(r is not None for r, t in zip((r_cm, r_rd, r_rm, r_sh, r_up, r_low), (g_cm, g_rd, g_rm, g_sh, g_up, g_low))
                     if t is not None)
        keep = (w, cm, rd, rm, sh, u, l, xmin, xmax, gy, gws, g_up, g_low, g_cm, g_sh, g_rd, g_rm, ws)
        if ctx.batch is not None and gx is None and routed:
            # deferred only when no gradient goes back to autograd (AccumulateGrad would copy a buffer that is not filled yet):
            # every consumer (the optimiser arena, optim.GradCollector.flush) runs after the batch is flushed
            ctx.batch.add_backward(bargs, keep)
        elif WgradQueue.pending(gy) and gx is None and routed:
            WgradQueue.after.append(("oq_fakequant_bwd", bargs, keep))      # dW is parked: this launch goes right behind the group
        else:
            if WgradQueue.pending(gy):
                WgradQueue.flush()
            C.call("oq_fakequant_bwd", *bargs, C.stream())
        if gx is not None and gx.dtype != ctx.in_dtype:
            gx = gx.to(ctx.in_dtype)
        if r_up is not None:
            g_up = None               # already in the arena
        if r_low is not None:
            g_low = None
        outs = [g_cm, g_rd, g_rm, g_sh]
        for i, (par, g) in enumerate(zip((r_cm, r_rd, r_rm, r_sh), outs)):
            if par is not None and g is not None:
                par._oq_collector.add(par, g)
                outs[i] = None
        g_cm, g_rd, g_rm, g_sh = outs
        return gx, g_cm, g_rd, g_rm, g_sh, g_up, g_low, None, None, None, None, None, None, None


def _gradient_routing_on():
    return not os.environ.get("OQ_NO_GRAD_ROUTING")       # A/B switch: plain autograd accumulation


def fake_quant(x, nbits, seg=None, up=None, low=None, symmetric=False, out_dtype=None, stash=None,
               col_mul=None, row_div=None, row_mul=None, shift=None, out=None, src=None):
    """Functional entry: returns y (and wshift when `shift` is given).  out: destination of y; src: float32 source of the
    same values (see FakeQuantFn)."""
    seg = seg or x.shape[-1]
    if (seg == x.shape[-1] and seg <= 512 and col_mul is None and row_div is None and row_mul is None
            and shift is None and up is None and out is None and src is None):
        # short rows (per-head quantisation over head_dim): pack several segments into one kernel row so a
        # workgroup streams 2-8 KB instead of 256 B; segments never straddle rows, results are identical.
        nrows = x.numel() // seg
        m = 1
        while seg * m * 2 <= 4096 and nrows % (m * 2) == 0:
            m *= 2
        if m > 1:
            y, _ = FakeQuantFn.apply(x.contiguous().view(nrows // m, seg * m), None, None, None, None, None, None,
                                     nbits, seg, symmetric, out_dtype or x.dtype, stash)
            return y.view(x.shape)
    y, wshift = FakeQuantFn.apply(x, col_mul, row_div, row_mul, shift, up, low, nbits, seg, symmetric,
                                  out_dtype or x.dtype, stash, out, src)
    return (y, wshift) if shift is not None else y


def stacked_rows(ts):
    """The 2-D tensors `ts` (same row length, dtype) lie back to back in ONE buffer -> that buffer as one [sum rows, cols]
    tensor, else None.  Sibling projections whose fake-quant weights were written into such a buffer
    (block_common: q | k | v and gate | up) run as ONE GEMM per direction: y = x @ [W_0; W_1; ..].T gives the outputs as
    column blocks, dX = dY @ [W_0; W_1; ..] sums the siblings' input gradients inside the GEMM's fp32 accumulators, and
    dW = dY.T @ x gives the weight gradients as row blocks."""
    if os.environ.get("OQ_STACKED_GEMM", "1") == "0" or len(ts) < 2:
        return None
    t0 = ts[0]
    if any(t is None or t.dim() != 2 or not t.is_contiguous() or t.dtype != t0.dtype or t.shape[1] != t0.shape[1]
           or t.device != t0.device for t in ts):
        return None
    es = t0.element_size()
    base = t0.untyped_storage().data_ptr()
    for a, b in zip(ts, ts[1:]):
        if b.untyped_storage().data_ptr() != base or a.data_ptr() + a.numel() * es != b.data_ptr():
            return None
    rows = sum(t.shape[0] for t in ts)
    return torch.empty(0, dtype=t0.dtype, device=t0.device).set_(t0.untyped_storage(), t0.storage_offset(),
                                                                 (rows, t0.shape[1]), (t0.shape[1], 1))


def stacked_vectors(vs):
    """None (all absent) or the 1-D float32 tensors `vs` as one contiguous vector when they lie back to back; False when
    they cannot be addressed as one."""
    if all(v is None for v in vs):
        return None
    if any(v is None or v.dim() != 1 or v.dtype != torch.float32 or not v.is_contiguous() for v in vs):
        return False
    base = vs[0].untyped_storage().data_ptr()
    for a, b in zip(vs, vs[1:]):
        if b.untyped_storage().data_ptr() != base or a.data_ptr() + a.numel() * 4 != b.data_ptr():
            return False
    n = sum(v.numel() for v in vs)
    return torch.empty(0, dtype=torch.float32, device=vs[0].device).set_(vs[0].untyped_storage(), vs[0].storage_offset(), (n,), (1,))


# ------------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------------
def gemm(a, b, c, M, N, K, lda, ldb, ldc, a_kc, b_kc, bias=None, alpha=1.0, batch_o=1, batch_i=1,
         sa=(0, 0), sb=(0, 0), sc=(0, 0), a_off=0, b_off=0, c_off=0, tri=0, addend=None):
    """Raw strided-batched GEMM on device buffers (element offsets/strides).  addend: tensor with c's dtype / layout
    that is added in the epilogue (may be c itself: accumulate)."""
    if addend is not None and (addend.dtype != c.dtype or not addend.is_cuda or not addend.is_contiguous()):
        raise C.OQError("gemm: addend must be a contiguous GPU tensor of the output dtype")
    for t in (a, b, c):
        if not t.is_cuda:
            raise C.OQError("gemm: the HIP path needs GPU tensors; there is no CPU fallback")
        if not t.is_contiguous():
            raise C.OQError("gemm: non-contiguous buffer")
    es_in, es_out = a.element_size(), c.element_size()
    args = (a.data_ptr() + a_off * es_in, b.data_ptr() + b_off * es_in, c.data_ptr() + c_off * es_out,
            C.fptr(bias), None if addend is None else addend.data_ptr() + c_off * es_out, M, N, K, lda, ldb, ldc, int(a_kc), int(b_kc),
            C.dt(a), C.dt(c), float(alpha), batch_o, batch_i, sa[0], sa[1], sb[0], sb[1], sc[0], sc[1], int(tri))
    ws_bytes = C.size_call("oq_gemm_workspace", M, N, K, C.dt(a), batch_o * batch_i, int(tri))
    if ws_bytes:
        # a ragged round of long tiles (LLaMA-2-13B's N = 5120 launches): the kernel splits the contraction into S parts and a
        # second launch adds the fp32 partial outputs it parks in this workspace
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device)
        C.call("oq_gemm_ws", *args, ws.data_ptr(), ws_bytes, C.stream())
    else:
        C.call("oq_gemm", *args, C.stream())


class IntCodes:
    """Integer side of a fake-quantised tensor, written by the quantiser kernels next to their bf16 / f32 output:
    codes [rows, cols] int8 = the grid codes 0 .. 2^nbits - 1 (8-bit grids: code - 128); scale, zp [rows] (the quantiser's
    scale / rounded zero-point); csum [rows] = sum of the stored codes of the row (float, exact).  With it
    dequant[r][k] = (code[r][k] - zp[r]) * scale[r]  exactly, and a Linear whose two operands carry IntCodes runs its fprop
    on the int8 MFMA (gemm_i8)."""
    __slots__ = ("codes", "scale", "zp", "csum", "nbits")

    def __init__(self, codes, scale, zp, csum, nbits):
        self.codes, self.scale, self.zp, self.csum, self.nbits = codes, scale, zp, csum, int(nbits)

    def rows(self, lo, hi):
        """The same for the row block [lo, hi) (sibling weights stacked in one buffer)."""
        return IntCodes(self.codes[lo:hi], self.scale[lo:hi], self.zp[lo:hi], self.csum[lo:hi], self.nbits)


class WeightDest:
    """Caller-provided destinations of a weight quantiser's outputs: row blocks of buffers that stack sibling weights
    (block_common._weight_slabs), so that q | k | v and gate | up -- values, integer codes and per-row vectors -- are one
    operand of ONE GEMM per direction.  Any field may be None (allocated by the quantiser then)."""
    __slots__ = ("y", "wshift", "codes", "scale", "zp", "csum")

    def __init__(self, y=None, wshift=None, codes=None, scale=None, zp=None, csum=None):
        self.y, self.wshift, self.codes, self.scale, self.zp, self.csum = y, wshift, codes, scale, zp, csum


def int_fprop_on():
    """Integer-exact fprop of the fake-quant Linears (oq_gemm_i8) in the bf16 production mode.  OQ_INT_FPROP=0: A/B switch
    back to bf16 operands."""
    return os.environ.get("OQ_INT_FPROP", "1") != "0"


def int_pre_dtype(act_dtype, site="qkv"):
    """dtype of a projection output that feeds a fused producer -> quantiser kernel (site "qkv": q | k | v -> RoPE -> head
    quantisers; site "mlp": gate | up -> silu * up -> down_proj input quantiser) on the integer path: float32 by default, so
    that the exact GEMM result is not rounded to bf16 in front of the next 4-bit rounding decision.
    OQ_INT_PRE_F32=0 / OQ_INT_PRE_F32_QKV=0 / OQ_INT_PRE_F32_MLP=0: the activation dtype (A/B switches)."""
    dflt = {"qkv": "1", "mlp": "0"}[site]
    on = os.environ.get("OQ_INT_PRE_F32", "1") != "0" and os.environ.get("OQ_INT_PRE_F32_" + site.upper(), dflt) != "0"
    return torch.float32 if on else act_dtype


def wide_on():
    """Un-rounded float32 side channel (`_oq_wide` on a bf16 tensor) for the activations that reach a 4-bit rounding decision
    in the bf16 production mode: the fused attention's output in front of the o_proj input quantiser, the two hidden states
    (o_proj / down_proj output + residual) in front of the second norm's quantiser and of the loss.  The bf16 tensor stays the
    autograd value (gradients keep flowing in bf16); kernels that know the channel read it instead.  OQ_WIDE=0: A/B switch."""
    return os.environ.get("OQ_WIDE", "1") != "0"


def grid_attention_on():
    """Fused attention on the head quantisers' integer grid (oq_attn_*_grid): q, k, v are never rounded to 16 bits.
    OQ_GRID_ATTN=0: A/B switch back to bf16 values."""
    return os.environ.get("OQ_GRID_ATTN", "1") != "0"


def wide_of(t):
    """The float32 side channel of `t` (same shape), or None."""
    w = getattr(t, "_oq_wide", None)
    if w is None or w.dtype != torch.float32 or w.numel() != t.numel() or w.device != t.device or not wide_on():
        return None
    return w.view(t.shape)


def int_codes_supported(cols, seg, nbits, let):
    return bool(C.size_call("oq_fakequant_codes_supported", int(cols), int(seg), int(nbits), int(bool(let))))


def stacked_int(ints):
    """IntCodes of sibling weights whose codes and per-row vectors lie back to back (block_common._weight_slabs) -> the
    IntCodes of the stacked operand, else None."""
    if any(i is None for i in ints) or len({i.nbits for i in ints}) != 1:
        return None
    codes = stacked_rows([i.codes for i in ints])
    if codes is None:
        return None
    vecs = [stacked_vectors([getattr(i, f) for i in ints]) for f in ("scale", "zp", "csum")]
    if any(v is None or v is False for v in vecs):
        return None
    return IntCodes(codes, vecs[0], vecs[1], vecs[2], ints[0].nbits)


def gemm_i8(a, b, c, bias=None, addend=None, c_off=0, wide=None):
    """c[M, N] = dequant(a)[M, K] @ dequant(b)[N, K]^T + bias (+ addend), contracted exactly on the int8 MFMA (oq_gemm_i8).
    a, b: IntCodes; c: preallocated float32 / bfloat16 GPU tensor -- [M, N], or [M, ldc] with the result written to the
    column block [c_off, c_off + N) (sibling projections sharing one output buffer).  addend: float32 or bfloat16 [M, N].
    wide: float32 [M, N] that receives the un-rounded result as well (dense output only)."""
    M, K = a.codes.shape
    N = b.codes.shape[0]
    ldc = c.shape[-1]
    if b.codes.shape[1] != K or c.dim() != 2 or c.shape[0] != M or c_off < 0 or c_off + N > ldc or not c.is_contiguous():
        raise C.OQError(f"gemm_i8: shapes a {tuple(a.codes.shape)} b {tuple(b.codes.shape)} c {tuple(c.shape)} offset {c_off}")
    if addend is not None and (ldc != N or c_off):
        raise C.OQError("gemm_i8: addend only with a dense [M, N] output")
    for t in (a.codes, b.codes):
        if t.dtype != torch.int8 or not t.is_cuda or not t.is_contiguous():
            raise C.OQError("gemm_i8: codes must be contiguous int8 GPU tensors; there is no CPU fallback")
    for v, n in ((a.scale, M), (a.zp, M), (a.csum, M), (b.scale, N), (b.zp, N), (b.csum, N)):
        if v.numel() != n or v.dtype != torch.float32:
            raise C.OQError("gemm_i8: per-row vectors must be float32 with one entry per row")
    if addend is not None and (addend.dtype not in (torch.float32, torch.bfloat16) or tuple(addend.shape) != (M, N)
                               or not addend.is_contiguous()):
        raise C.OQError("gemm_i8: addend must be a contiguous float32 / bfloat16 tensor of the output's shape")
    if wide is not None and (wide.dtype != torch.float32 or tuple(wide.shape) != (M, N) or not wide.is_contiguous()
                             or ldc != N or c_off):
        raise C.OQError("gemm_i8: the wide copy is a contiguous float32 [M, N] tensor next to a dense output")
    C.call("oq_gemm_i8", C.ptr(a.codes), C.ptr(b.codes), c.data_ptr() + c_off * c.element_size(), C.fptr(wide), C.fptr(bias),
           C.ptr(addend), C.dt(addend) if addend is not None else 0, C.fptr(a.scale), C.fptr(a.zp), C.fptr(a.csum), C.fptr(b.scale), C.fptr(b.zp), C.fptr(b.csum),
           M, N, K, K, K, ldc, a.nbits, b.nbits, C.dt(c), C.stream())


class SiblingGrads:
    """Side channel for the input gradient of SIBLING consumers of one tensor (q/k/v projections; gate/up): the first
    consumer whose backward runs returns its dL/dx to autograd as usual, the others park theirs here and return None, and
    the producer's backward kernel (oq_norm_quant_bwd) adds the parked pieces while it loads the gradient -- instead of
    autograd materialising the sum with one `add` launch per extra consumer (3 launches, 100 MB of traffic per step)."""

    def __init__(self):
        self.primary = False
        self.parts = []

    def offer(self, gx):
        if not self.primary:
            self.primary = True
            return gx
        self.parts.append(gx)
        return None

    def take(self):
        parts, self.parts, self.primary = self.parts, [], False
        return parts


class LinearFn(torch.autograd.Function):
    """y = x @ wq.T + bias (+ residual)  (quantize/int_linear.py:62; the residual add of
    models/int_llama_layer.py:246,264 is folded into the GEMM's store) with dgrad / wgrad / bias-grad kernels."""

    @staticmethod
    def forward(ctx, x, wq, bias, residual=None, sib=None, xint=None, wint=None, stash=None):
        """stash (dict): with "want_wide" the integer fprop also writes its un-rounded float32 result into stash["wide"] (the
        returned bf16 tensor is its rounded copy), and the residual is read from stash["res_wide"] (float32) when given."""
        ctx.sib = sib
        ctx.park_wgrad = bool(getattr(wq, "_oq_fq_out", False))       # the weight's producer knows the WgradQueue protocol
        x2 = x.contiguous().view(-1, x.shape[-1])
        wq = wq.contiguous()
        T, K = x2.shape
        N = wq.shape[0]
        if wq.dtype != x2.dtype:
            raise C.OQError(f"LinearFn: weight dtype {wq.dtype} != activation dtype {x2.dtype}")
        y = torch.empty((T, N), dtype=x2.dtype, device=x2.device)
        b32 = _f32(bias)
        res2 = None
        if residual is not None:
            if residual.dtype != x2.dtype or residual.numel() != T * N:
                raise C.OQError("LinearFn: residual must have the output's dtype and size")
            res2 = residual.contiguous().view(T, N)
        if xint is not None and wint is not None and tuple(xint.codes.shape) == (T, K) and tuple(wint.codes.shape) == (N, K):
            # both operands are on quantiser grids: the fprop contracts their integer codes exactly (int8 MFMA); x2 / wq -- the
            # same values rounded to bf16 -- are only the backward's operands
            wide = None
            if stash is not None and stash.get("want_wide") and y.dtype == torch.bfloat16:
                wide = stash["wide"] = torch.empty((T, N), dtype=torch.float32, device=x2.device)
                rw = stash.get("res_wide")
                if rw is not None and res2 is not None and rw.numel() == T * N:
                    res2 = rw.contiguous().view(T, N)
            gemm_i8(xint, wint, y, bias=b32, addend=res2, wide=wide)
        else:
            gemm(x2, wq, y, T, N, K, K, K, N, True, True, bias=b32, addend=res2)
        ctx.save_for_backward(x2, wq)
        ctx.has_bias = bias is not None
        ctx.has_res = residual is not None
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, gy):
        x2, wq = ctx.saved_tensors
        T, K = x2.shape
        N = wq.shape[0]
        gy2 = gy.contiguous().view(T, N)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty((T, K), dtype=x2.dtype, device=x2.device)
            # dX[t,k] = sum_n dY[t,n] * W[n,k]   (B is k-strided: B(k_out, n) = W[n*K + k_out])
            gemm(gy2, wq, gx, T, K, N, N, K, K, True, False)
            gx = gx.view(ctx.xshape)
            if ctx.sib is not None:
                gx = ctx.sib.offer(gx)
        if ctx.needs_input_grad[1]:
            gw = torch.empty((N, K), dtype=wq.dtype, device=x2.device)
            # dW[n,k] = sum_t dY[t,n] * X[t,k]   (both operands k-strided)
            wgrad(gy2, x2, gw, N, K, T, N, K, K, park=ctx.park_wgrad)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = torch.empty((N,), dtype=torch.float32, device=x2.device)
            ws_n = C.size_call("oq_colsum_workspace", T, N)
            ws = torch.empty(ws_n, dtype=torch.float32, device=gy2.device)
            C.call("oq_colsum", C.ptr(gy2), C.dt(gy2), T, N, C.fptr(gb), C.fptr(ws), ws_n, C.stream())
        gres = gy if (ctx.has_res and ctx.needs_input_grad[3]) else None
        return gx, gw, gb, gres, None, None, None, None


def rope_quant_supported(dtype, hd):
    """Fused projection -> RoPE -> head-wise fake quant (bf16 / f32, head_dim 128).  OQ_NO_FUSED_ROPEQ=1: A/B switch."""
    if os.environ.get("OQ_NO_FUSED_ROPEQ") or dtype not in C._DT:
        return False
    return bool(C.size_call("oq_rope_quant_supported", C._DT[dtype], int(hd)))


class LinearRopeQuantFn(torch.autograd.Function):
    """y = fake_quant_head(rope(x @ wq.T + bias)) for one of q / k (cos, sin given) or fake_quant_head(x @ wq.T + bias)
    for v (cos = sin = None): quantize/int_linear.py:62 -> models/int_llama_layer.py:124-125 -> quant_x1 / quant_x2
    (:140-143,161) as ONE autograd node: the rotated tensor is never stored (two 16.8 MB round trips per direction at
    LLaMA-7B) and is not rounded to bf16 in front of the 4-bit rounding decision.  The projection's output lives only
    inside this node; OQ_QKV_F32=1 keeps it in fp32 as well (measured: 1 % slower, and the gradients of the q / k path
    agree no better with an fp32 run -- their rounding flips come from the shared 4-bit INPUT of the projections).
    x [bs, T, K]; returns y [bs, T, nh, hd]."""

    @staticmethod
    def forward(ctx, x, wq, bias, cos, sin, nbits, hd, stash, sib=None):
        ctx.sib = sib
        x2 = x.contiguous().view(-1, x.shape[-1])
        wq = wq.contiguous()
        rows, K = x2.shape
        N = wq.shape[0]
        nh = N // hd
        if wq.dtype != x2.dtype:
            raise C.OQError(f"LinearRopeQuantFn: weight dtype {wq.dtype} != activation dtype {x2.dtype}")
        pre_dtype = torch.float32 if os.environ.get("OQ_QKV_F32") else x2.dtype
        pre = torch.empty((rows, N), dtype=pre_dtype, device=x2.device)
        gemm(x2, wq, pre, rows, N, K, K, K, N, True, True, bias=_f32(bias))
        y = torch.empty((rows, N), dtype=x2.dtype, device=x2.device)
        scale, zp, xmin, xmax = (torch.empty((rows * nh, 1), dtype=torch.float32, device=x2.device) for _ in range(4))
        T = x.shape[-2]
        C.call("oq_rope_quant_fwd", C.ptr(pre), C.dt(pre), rows, T, nh, hd, C.fptr(cos), C.fptr(sin), int(nbits),
               C.ptr(y), C.dt(y), C.fptr(scale), C.fptr(zp), C.fptr(xmin), C.fptr(xmax), C.stream())
        if stash is not None:
            stash["scale"], stash["zp"] = scale, zp
        ctx.save_for_backward(x2, wq, pre, xmin, xmax, cos, sin)
        ctx.cfg = (T, nh, hd, int(nbits), bias is not None, x.shape)
        return y.view(*x.shape[:-1], nh, hd)

    @staticmethod
    def backward(ctx, gy):
        x2, wq, pre, xmin, xmax, cos, sin = ctx.saved_tensors
        T, nh, hd, nbits, has_bias, xshape = ctx.cfg
        rows, K = x2.shape
        N = wq.shape[0]
        gy = gy.contiguous()
        if gy.dtype != x2.dtype:
            gy = gy.to(x2.dtype)
        gpre = torch.empty((rows, N), dtype=x2.dtype, device=x2.device)
        C.call("oq_rope_quant_bwd", C.ptr(pre), C.dt(pre), rows, T, nh, hd, C.fptr(cos), C.fptr(sin), nbits,
               C.fptr(xmin), C.fptr(xmax), C.ptr(gy), C.dt(gy), C.ptr(gpre), C.stream())
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty((rows, K), dtype=x2.dtype, device=x2.device)
            gemm(gpre, wq, gx, rows, K, N, N, K, K, True, False)
            gx = gx.view(xshape)
            if ctx.sib is not None:
                gx = ctx.sib.offer(gx)
        if ctx.needs_input_grad[1]:
            gw = torch.empty((N, K), dtype=wq.dtype, device=x2.device)
            gemm(gpre, x2, gw, N, K, rows, N, K, K, False, False)
        if has_bias and ctx.needs_input_grad[2]:
            gb = torch.empty((N,), dtype=torch.float32, device=x2.device)
            ws_n = C.size_call("oq_colsum_workspace", rows, N)
            ws = torch.empty(ws_n, dtype=torch.float32, device=x2.device)
            C.call("oq_colsum", C.ptr(gpre), C.dt(gpre), rows, N, C.fptr(gb), C.fptr(ws), ws_n, C.stream())
        return gx, gw, gb, None, None, None, None, None, None


class QKVRopeQuantFn(torch.autograd.Function):
    """q, k, v = LinearRopeQuantFn three times, as ONE autograd node: the projections write column blocks of one
    [rows, Nq + Nk + Nv] buffer, RoPE + head-wise fake quant of all heads is one launch per direction
    (oq_qkv_rope_quant_*), the bias gradients one column sum.  When the three fake-quant weights (and biases) lie back to back
    in one buffer (stacked_rows: block_common._weight_slabs hands such destinations to the weight quantisers) the projections
    are ONE GEMM per direction: N = Nq + Nk + Nv forward, K = that sum for dX (the three input gradients are added in the
    fp32 accumulators), M = that sum for dW; otherwise one GEMM per matrix into / out of the shared buffer, bit-identical to
    three separate nodes.  nbits >= 16 is the identity grid (quantize/quantizer.py:109-110): rotate and split only -- the
    weight-only configurations' path (models/int_llama_layer.py:116-125).
    x [bs, T, K]; returns q [bs, T, nhq, hd], k, v [bs, T, nhk|nhv, hd]."""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, wv, bv, cos, sin, nbits, hd, stashes, sib=None, xint=None, wints=None, grid=False):
        ctx.sib = sib
        x2 = x.contiguous().view(-1, x.shape[-1])
        ws = [w.contiguous() for w in (wq, wk, wv)]
        bs_ = [bq, bk, bv]
        rows, K = x2.shape
        Ns = [w.shape[0] for w in ws]
        Ntot = sum(Ns)
        for w in ws:
            if w.dtype != x2.dtype:
                raise C.OQError(f"QKVRopeQuantFn: weight dtype {w.dtype} != activation dtype {x2.dtype}")
        offs = [0, Ns[0], Ns[0] + Ns[1]]
        ctx.park_wgrad = all(getattr(w, "_oq_fq_out", False) for w in (wq, wk, wv))
        wall = stacked_rows(ws)
        ball = stacked_vectors(bs_) if wall is not None else False
        ctx.stacked = wall is not None and ball is not False
        wint = stacked_int(list(wints)) if (ctx.stacked and xint is not None and wints is not None) else None
        if wint is not None and (tuple(xint.codes.shape) != (rows, K) or tuple(wint.codes.shape) != (Ntot, K)):
            wint = None
        each_int = (wint is None and xint is not None and wints is not None and tuple(xint.codes.shape) == (rows, K)
                    and all(tuple(wi.codes.shape) == (N, K) for wi, N in zip(wints, Ns)))
        pre = torch.empty((rows, Ntot), dtype=int_pre_dtype(x2.dtype) if (wint is not None or each_int) else x2.dtype,
                          device=x2.device)
        if wint is not None:
            # integer-exact projections (oq_gemm_i8); the result reaches RoPE and the head quantisers in fp32
            gemm_i8(xint, wint, pre, bias=ball)
        elif each_int:
            # the same per matrix (weights not stacked): identical integer accumulators, identical results
            for wi, b, off in zip(wints, bs_, offs):
                gemm_i8(xint, wi, pre, bias=_f32(b), c_off=off)
        elif ctx.stacked:
            # the three fake-quant weights are row blocks of one buffer: ONE GEMM with N = Nq + Nk + Nv
            gemm(x2, wall, pre, rows, Ntot, K, K, K, Ntot, True, True, bias=ball)
        else:
            for w, b, N, off in zip(ws, bs_, Ns, offs):
                gemm(x2, w, pre, rows, N, K, K, K, Ntot, True, True, bias=_f32(b), c_off=off)
        nhs = [N // hd for N in Ns]
        nht = sum(nhs)
        ys = [torch.empty((rows, N), dtype=x2.dtype, device=x2.device) for N in Ns]
        ident = int(nbits) >= 16          # identity grid: rotate + split only (weight-only configurations)
        nbits = 16 if ident else int(nbits)
        scale, zp, xmin, xmax = ((None,) * 4 if ident else
                                 tuple(torch.empty((rows * nht, 1), dtype=torch.float32, device=x2.device) for _ in range(4)))
        T = x.shape[-2]
        C.call("oq_qkv_rope_quant_fwd", C.ptr(pre), C.dt(pre), rows, T, nhs[0], nhs[1], nhs[2], hd, C.fptr(cos), C.fptr(sin),
               int(nbits), C.ptr(ys[0]), C.ptr(ys[1]), C.ptr(ys[2]), C.dt(ys[0]), int(bool(grid) and not ident), C.fptr(scale),
               C.fptr(zp), C.fptr(xmin), C.fptr(xmax), C.stream())
        if stashes is not None and not ident:
            h0 = 0
            sv, zv = scale.view(rows, nht, 1), zp.view(rows, nht, 1)
            for st, n in zip(stashes, nhs):
                st["scale"], st["zp"] = sv[:, h0:h0 + n], zv[:, h0:h0 + n]       # views of the merged per-(token, head) vectors
                h0 += n
        if ident:
            ctx.save_for_backward(x2, *ws, cos, sin)        # the backward of rotate + split needs no forward values
        else:
            ctx.save_for_backward(x2, *ws, pre, xmin, xmax, cos, sin)
        ctx.cfg = (T, tuple(nhs), hd, int(nbits), tuple(b is not None for b in bs_), x.shape, tuple(offs))
        return tuple(y.view(*x.shape[:-1], n, hd) for y, n in zip(ys, nhs))

    @staticmethod
    def backward(ctx, gq, gk, gv):
        T, nhs, hd, nbits, has_bias, xshape, offs = ctx.cfg
        if nbits >= 16:
            x2, wq, wk, wv, cos, sin = ctx.saved_tensors
            pre = x2                                        # not read by the identity-grid backward; any valid pointer
            xmin = xmax = None
        else:
            x2, wq, wk, wv, pre, xmin, xmax, cos, sin = ctx.saved_tensors
        rows, K = x2.shape
        ws = (wq, wk, wv)
        Ns = [w.shape[0] for w in ws]
        Ntot = sum(Ns)
        gs = []
        for g, N in zip((gq, gk, gv), Ns):
            if g is None:
                g = torch.zeros((rows, N), dtype=x2.dtype, device=x2.device)
            g = g.contiguous()
            gs.append(g if g.dtype == x2.dtype else g.to(x2.dtype))
        gpre = torch.empty((rows, Ntot), dtype=x2.dtype, device=x2.device)
        C.call("oq_qkv_rope_quant_bwd", C.ptr(pre), C.dt(pre), rows, T, nhs[0], nhs[1], nhs[2], hd, C.fptr(cos), C.fptr(sin),
               nbits, C.fptr(xmin), C.fptr(xmax), C.ptr(gs[0]), C.ptr(gs[1]), C.ptr(gs[2]), C.dt(gs[0]), C.ptr(gpre), C.stream())
        need = ctx.needs_input_grad         # x, wq, bq, wk, bk, wv, bv, ...
        gx = None
        wall = stacked_rows(ws) if ctx.stacked else None
        if need[0] and wall is not None:
            # dX = dPre @ [Wq; Wk; Wv]: the three projections' input gradients are summed in the GEMM's fp32 accumulators
            gx2 = torch.empty((rows, K), dtype=x2.dtype, device=x2.device)
            gemm(gpre, wall, gx2, rows, K, Ntot, Ntot, K, K, True, False)
            gx = gx2.view(xshape)
            if ctx.sib is not None:
                gx = ctx.sib.offer(gx)
        elif need[0]:
            if ctx.sib is not None:
                # one dL/dx per projection: the first goes back to autograd, the others are summed inside oq_norm_quant_bwd
                for w, N, off in zip(ws, Ns, offs):
                    gxi = torch.empty((rows, K), dtype=x2.dtype, device=x2.device)
                    gemm(gpre, w, gxi, rows, K, N, Ntot, K, K, True, False, a_off=off)
                    r = ctx.sib.offer(gxi.view(xshape))
                    if r is not None:
                        gx = r
            else:
                gx2 = torch.empty((rows, K), dtype=x2.dtype, device=x2.device)
                for i, (w, N, off) in enumerate(zip(ws, Ns, offs)):
                    gemm(gpre, w, gx2, rows, K, N, Ntot, K, K, True, False, a_off=off, addend=None if i == 0 else gx2)
                gx = gx2.view(xshape)
        gws = [None, None, None]
        if wall is not None and need[1] and need[3] and need[5]:
            # dW of the three as row blocks of one buffer: ONE GEMM with M = Nq + Nk + Nv
            gwall = torch.empty((Ntot, K), dtype=wall.dtype, device=x2.device)
            wgrad(gpre, x2, gwall, Ntot, K, rows, Ntot, K, K, park=ctx.park_wgrad)
            gws = [gwall[off:off + N] for N, off in zip(Ns, offs)]
        else:
            for i, (w, N, off) in enumerate(zip(ws, Ns, offs)):
                if need[1 + 2 * i]:
                    gws[i] = torch.empty((N, K), dtype=w.dtype, device=x2.device)
                    wgrad(gpre, x2, gws[i], N, K, rows, Ntot, K, K, gy_off=off, park=ctx.park_wgrad)
        gbs = [None, None, None]
        if any(has_bias[i] and need[2 + 2 * i] for i in range(3)):
            gb = torch.empty((Ntot,), dtype=torch.float32, device=x2.device)
            ws_n = C.size_call("oq_colsum_workspace", rows, Ntot)
            wsb = torch.empty(ws_n, dtype=torch.float32, device=x2.device)
            C.call("oq_colsum", C.ptr(gpre), C.dt(gpre), rows, Ntot, C.fptr(gb), C.fptr(wsb), ws_n, C.stream())
            for i, (N, off) in enumerate(zip(Ns, offs)):
                if has_bias[i] and need[2 + 2 * i]:
                    gbs[i] = gb[off:off + N]
        return (gx, gws[0], gbs[0], gws[1], gbs[1], gws[2], gbs[2], None, None, None, None, None, None, None, None, None)


class SiblingLinearFn(torch.autograd.Function):
    """Projections that read the SAME input (q/k/v; gate/up): y_i = x @ w_i.T + b_i.  One autograd node, so the
    input gradient dX = sum_i dY_i @ W_i is ACCUMULATED by the dgrad GEMMs' epilogue (addend = the running sum) instead
    of materialising every term and adding them with separate launches.  Inputs: x, then (w_i, b_i) pairs."""

    @staticmethod
    def forward(ctx, x, *wb):
        x2 = x.contiguous().view(-1, x.shape[-1])
        T, K = x2.shape
        ws = [w.contiguous() for w in wb[0::2]]
        bs = list(wb[1::2])
        outs = []
        for w, b in zip(ws, bs):
            if w.dtype != x2.dtype:
                raise C.OQError(f"SiblingLinearFn: weight dtype {w.dtype} != activation dtype {x2.dtype}")
            N = w.shape[0]
            y = torch.empty((T, N), dtype=x2.dtype, device=x2.device)
            gemm(x2, w, y, T, N, K, K, K, N, True, True, bias=_f32(b))
            outs.append(y.view(*x.shape[:-1], N))
        ctx.save_for_backward(x2, *ws)
        ctx.has_bias = [b is not None for b in bs]
        ctx.xshape = x.shape
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gys):
        x2, *ws = ctx.saved_tensors
        T, K = x2.shape
        need = ctx.needs_input_grad
        gx = None
        grads = []
        first = True
        for i, (w, gy) in enumerate(zip(ws, gys)):
            N = w.shape[0]
            gw = gb = None
            if gy is not None:
                gy2 = gy.contiguous().view(T, N)
                if need[0]:
                    if gx is None:
                        gx = torch.empty((T, K), dtype=x2.dtype, device=x2.device)
                    gemm(gy2, w, gx, T, K, N, N, K, K, True, False, addend=None if first else gx)
                    first = False
                if need[1 + 2 * i]:
                    gw = torch.empty((N, K), dtype=w.dtype, device=x2.device)
                    gemm(gy2, x2, gw, N, K, T, N, K, K, False, False)
                if ctx.has_bias[i] and need[2 + 2 * i]:
                    gb = torch.empty((N,), dtype=torch.float32, device=x2.device)
                    ws_n = C.size_call("oq_colsum_workspace", T, N)
                    wsb = torch.empty(ws_n, dtype=torch.float32, device=gy2.device)
                    C.call("oq_colsum", C.ptr(gy2), C.dt(gy2), T, N, C.fptr(gb), C.fptr(wsb), ws_n, C.stream())
            grads += [gw, gb]
        if gx is not None:
            gx = gx.view(ctx.xshape)
        return (gx, *grads)


class AttnScoresFn(torch.autograd.Function):
    """S[b,h] = Q[b,:,h,:] @ K[b,:,h//rep,:]^T  (quantize/int_matmul.py:41-43 as used at
    models/int_llama_layer.py:143).  q [bs,T,nh,hd], k [bs,Tk,nkv,hd] -> S [bs,nh,T,Tk]."""

    @staticmethod
    def forward(ctx, q, k, causal=False):
        q, k = q.contiguous(), k.contiguous()
        bs, T, nh, hd = q.shape
        Tk, nkv = k.shape[1], k.shape[2]
        rep = nh // nkv
        causal = bool(causal) and T == Tk
        s = torch.empty((bs, nh, T, Tk), dtype=q.dtype, device=q.device)
        for b in range(bs):
            gemm(q, k, s, T, Tk, hd, nh * hd, nkv * hd, Tk, True, True, batch_o=nkv, batch_i=rep,
                 sa=(rep * hd, hd), sb=(hd, 0), sc=(rep * T * Tk, T * Tk),
                 a_off=b * T * nh * hd, b_off=b * Tk * nkv * hd, c_off=b * nh * T * Tk, tri=1 if causal else 0)
        ctx.save_for_backward(q, k)
        ctx.causal = causal
        return s

    @staticmethod
    def backward(ctx, gs):
        q, k = ctx.saved_tensors
        gs = gs.contiguous()
        bs, T, nh, hd = q.shape
        Tk, nkv = k.shape[1], k.shape[2]
        rep = nh // nkv
        gq = torch.empty_like(q)
        gk_full = torch.empty((bs, Tk, nh, hd), dtype=k.dtype, device=k.device)
        for b in range(bs):
            # dQ[t,d] = sum_t' dS[t,t'] K[t',d]          (causal: t' < m0 + tile)
            gemm(gs, k, gq, T, hd, Tk, Tk, nkv * hd, nh * hd, True, False, batch_o=nkv, batch_i=rep,
                 sa=(rep * T * Tk, T * Tk), sb=(hd, 0), sc=(rep * hd, hd),
                 a_off=b * nh * T * Tk, b_off=b * Tk * nkv * hd, c_off=b * T * nh * hd, tri=2 if ctx.causal else 0)
            # dK[t',d] = sum_t dS[t,t'] Q[t,d]    (per q-head, reduced over rep below; causal: t >= m0)
            gemm(gs, q, gk_full, Tk, hd, T, Tk, nh * hd, nh * hd, False, False, batch_o=nh, batch_i=1,
                 sa=(T * Tk, 0), sb=(hd, 0), sc=(hd, 0),
                 a_off=b * nh * T * Tk, b_off=b * T * nh * hd, c_off=b * Tk * nh * hd, tri=3 if ctx.causal else 0)
        gk = gk_full if rep == 1 else group_sum(gk_full, nkv, rep)[0]
        return gq, gk, None


class AttnPVFn(torch.autograd.Function):
    """O[b,:,h,:] = P[b,h] @ V[b,:,h//rep,:]  (models/int_llama_layer.py:163).  p [bs,nh,T,Tk],
    v [bs,Tk,nkv,hd] -> o [bs,T,nh,hd]."""

    @staticmethod
    def forward(ctx, p, v, causal=False):
        p, v = p.contiguous(), v.contiguous()
        bs, nh, T, Tk = p.shape
        nkv, hd = v.shape[2], v.shape[3]
        rep = nh // nkv
        causal = bool(causal) and T == Tk
        o = torch.empty((bs, T, nh, hd), dtype=p.dtype, device=p.device)
        for b in range(bs):
            gemm(p, v, o, T, hd, Tk, Tk, nkv * hd, nh * hd, True, False, batch_o=nkv, batch_i=rep,
                 sa=(rep * T * Tk, T * Tk), sb=(hd, 0), sc=(rep * hd, hd),
                 a_off=b * nh * T * Tk, b_off=b * Tk * nkv * hd, c_off=b * T * nh * hd, tri=2 if causal else 0)
        ctx.save_for_backward(p, v)
        ctx.causal = causal
        return o

    @staticmethod
    def backward(ctx, go):
        p, v = ctx.saved_tensors
        go = go.contiguous()
        bs, nh, T, Tk = p.shape
        nkv, hd = v.shape[2], v.shape[3]
        rep = nh // nkv
        gp = torch.empty_like(p)
        gv_full = torch.empty((bs, Tk, nh, hd), dtype=v.dtype, device=v.device)
        for b in range(bs):
            # dP[t,t'] = sum_d dO[t,d] V[t',d]          (causal: tiles above the diagonal are skipped)
            gemm(go, v, gp, T, Tk, hd, nh * hd, nkv * hd, Tk, True, True, batch_o=nkv, batch_i=rep,
                 sa=(rep * hd, hd), sb=(hd, 0), sc=(rep * T * Tk, T * Tk),
                 a_off=b * T * nh * hd, b_off=b * Tk * nkv * hd, c_off=b * nh * T * Tk, tri=1 if ctx.causal else 0)
            # dV[t',d] = sum_t P[t,t'] dO[t,d]           (causal: t >= m0)
            gemm(p, go, gv_full, Tk, hd, T, Tk, nh * hd, nh * hd, False, False, batch_o=nh, batch_i=1,
                 sa=(T * Tk, 0), sb=(hd, 0), sc=(hd, 0),
                 a_off=b * nh * T * Tk, b_off=b * T * nh * hd, c_off=b * Tk * nh * hd, tri=3 if ctx.causal else 0)
        gv = gv_full if rep == 1 else group_sum(gv_full, nkv, rep)[0]
        return gp, gv, None


# ------------------------------------------------------------------------------------------------------
# norms and glue
# ------------------------------------------------------------------------------------------------------
def _norm_forward(ctx, x, w, b, eps, is_ln):
    x = x.contiguous()
    cols = x.shape[-1]
    rows = x.numel() // cols
    w32, b32 = _f32(w), _f32(b)
    y = torch.empty_like(x)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device) if is_ln else None
    C.call("oq_norm_fwd", C.ptr(x), C.dt(x), rows, cols, C.fptr(w32), C.fptr(b32), float(eps), int(is_ln),
           C.ptr(y), C.fptr(rstd), C.fptr(mean), C.stream())
    ctx.save_for_backward(x, w32, rstd, mean)
    ctx.is_ln, ctx.has_b = is_ln, b is not None
    return x, y


def _norm_backward(ctx, gy, gpass):
    x, w32, rstd, mean = ctx.saved_tensors
    gy = gy.contiguous()
    cols = x.shape[-1]
    rows = x.numel() // cols
    gx = torch.empty_like(x)
    gw = torch.empty((cols,), dtype=torch.float32, device=x.device)
    gb = torch.empty((cols,), dtype=torch.float32, device=x.device) if (ctx.has_b and ctx.needs_input_grad[2]) else None
    ws_n = C.size_call("oq_norm_bwd_workspace", rows, cols)
    ws = torch.empty((ws_n,), dtype=torch.float32, device=x.device)
    if gpass is not None:
        gpass = gpass.contiguous()
        if gpass.dtype != x.dtype:
            gpass = gpass.to(x.dtype)
    C.call("oq_norm_bwd", C.ptr(x), C.ptr(gy), C.dt(x), rows, cols, C.fptr(w32), C.fptr(rstd), C.fptr(mean),
           int(ctx.is_ln), C.ptr(gx), C.fptr(gw), C.fptr(gb), C.ptr(gpass), C.fptr(ws), ws_n, C.stream())
    return gx, (gw if ctx.needs_input_grad[1] else None), gb, None, None


class NormFn(torch.autograd.Function):
    """OmniLlamaRMSNorm / OmniLayerNorm (quantize/omni_norm.py:26-34,52-63)."""

    @staticmethod
    def forward(ctx, x, w, b, eps, is_ln):
        return _norm_forward(ctx, x, w, b, eps, is_ln)[1]

    @staticmethod
    def backward(ctx, gy):
        return _norm_backward(ctx, gy, None)


class NormResidualFn(torch.autograd.Function):
    """(norm(x), x): the same norm, plus the input handed through for the block's residual path
    (models/int_llama_layer.py:248-264: residual = hidden; hidden = norm(hidden); ...; hidden = residual + mlp).
    One autograd node, so the gradient arriving on the residual path is added to the norm's input gradient inside
    the backward kernel (oq_norm_bwd gx_addend) instead of by a separate `add` launch."""

    @staticmethod
    def forward(ctx, x, w, b, eps, is_ln):
        xc, y = _norm_forward(ctx, x, w, b, eps, is_ln)
        return y, xc.view_as(xc)

    @staticmethod
    def backward(ctx, gy, gpass):
        if gy is None:          # only the residual path was used
            return gpass, None, None, None, None
        return _norm_backward(ctx, gy, gpass)


def norm_quant_supported(x, nbits):
    """Fused norm -> per-token fake quant (bf16 / f32, 512 .. 8192 columns).  OQ_NO_FUSED_NORMQ=1: A/B switch."""
    if os.environ.get("OQ_NO_FUSED_NORMQ") or not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float32):
        return False
    return 2 <= nbits < 16 and bool(C.size_call("oq_norm_quant_supported", C._DT[x.dtype], int(x.shape[-1])))


class NormQuantFn(torch.autograd.Function):
    """(fake_quant_per_token(norm(x)), x): OmniLlamaRMSNorm / OmniLayerNorm (quantize/omni_norm.py:26-34,52-63) fused
    with the act_quantizer of the QuantLinears that read its output (quantize/int_linear.py:59-60); the second output
    hands x through for the block's residual path exactly like NormResidualFn (its gradient is added inside the backward
    kernel).  The normalised row reaches the quantiser in fp32 and is never stored."""

    @staticmethod
    def forward(ctx, x, w, b, eps, is_ln, nbits, stash, src=None):
        """src: float32 tensor holding x's values un-rounded (`_oq_wide`); the kernels read it in place of x, y and the
        gradients keep x's dtype."""
        x = x.contiguous()
        xin = x
        if src is not None:
            if src.dtype != torch.float32 or src.numel() != x.numel() or x.dtype != torch.bfloat16:
                raise C.OQError("NormQuantFn: `src` must be a float32 tensor of the (bf16) input's shape")
            x = src.contiguous().view(x.shape)
        cols = x.shape[-1]
        rows = x.numel() // cols
        w32, b32 = _f32(w), _f32(b)
        y = torch.empty_like(xin)
        rstd, scale, zp, xmin, xmax = (torch.empty((rows, 1), dtype=torch.float32, device=x.device) for _ in range(5))
        mean = torch.empty((rows,), dtype=torch.float32, device=x.device) if is_ln else None
        codes = csum = None
        if stash is not None and stash.get("want_int") and int(nbits) <= 8:
            codes = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
            csum = torch.empty((rows,), dtype=torch.float32, device=x.device)
        C.call("oq_norm_quant_fwd", C.ptr(x), C.dt(x), rows, cols, C.fptr(w32), C.fptr(b32), float(eps), int(is_ln), int(nbits),
               C.ptr(y), C.dt(y), C.fptr(rstd), C.fptr(mean), C.fptr(scale), C.fptr(zp), C.fptr(xmin), C.fptr(xmax),
               C.ptr(codes), C.fptr(csum), C.stream())
        ctx.sib = None
        if stash is not None:
            stash["scale"], stash["zp"] = scale, zp
            if codes is not None:
                stash["int"] = IntCodes(codes, scale.view(-1), zp.view(-1), csum, int(nbits))
            if not os.environ.get("OQ_NO_SIBLING_GRADS"):
                ctx.sib = stash["sib"] = SiblingGrads()       # hand this to every consumer of y (see SiblingGrads)
        ctx.save_for_backward(x, w32, b32, rstd, mean, xmin, xmax)
        ctx.cfg = (bool(is_ln), int(nbits), b is not None, xin.dtype)
        return y, xin.view_as(xin)

    @staticmethod
    def backward(ctx, gy, gpass):
        x, w32, b32, rstd, mean, xmin, xmax = ctx.saved_tensors
        is_ln, nbits, has_b, gdt = ctx.cfg          # gdt: the autograd dtype of x (x itself may be its float32 source)
        if gy is None:
            return gpass, None, None, None, None, None, None, None
        cols = x.shape[-1]
        rows = x.numel() // cols
        gy = gy.contiguous()
        if gy.dtype != gdt:
            gy = gy.to(gdt)
        if gpass is not None:
            gpass = gpass.contiguous()
            if gpass.dtype != gdt:
                gpass = gpass.to(gdt)
        parts = ctx.sib.take() if ctx.sib is not None else []
        parts = [t.contiguous().view(rows, cols) for t in parts]
        if any(t.dtype != gdt for t in parts) or len(parts) > 2:
            gy = gy + sum(t.to(gdt) for t in parts)            # more pieces than the kernel takes: plain adds
            parts = []
        g2 = parts[0] if len(parts) > 0 else None
        g3 = parts[1] if len(parts) > 1 else None
        gx = torch.empty(x.shape, dtype=gdt, device=x.device)
        gw = torch.empty((cols,), dtype=torch.float32, device=x.device)
        gb = torch.empty((cols,), dtype=torch.float32, device=x.device) if (has_b and ctx.needs_input_grad[2]) else None
        ws_n = C.size_call("oq_norm_quant_bwd_workspace", rows, cols)
        ws = torch.empty((ws_n,), dtype=torch.float32, device=x.device)
        C.call("oq_norm_quant_bwd", C.ptr(x), C.ptr(gy), C.ptr(g2), C.ptr(g3), C.dt(x), C.dt(gy), rows, cols, C.fptr(w32), C.fptr(b32), C.fptr(rstd), C.fptr(mean),
               int(is_ln), nbits, C.fptr(xmin), C.fptr(xmax), C.ptr(gx), C.fptr(gw), C.fptr(gb), C.ptr(gpass), C.fptr(ws), ws_n,
               C.stream())
        return gx, (gw if ctx.needs_input_grad[1] else None), gb, None, None, None, None, None


class RopeFn(torch.autograd.Function):
    """x [bs,T,heads,hd] rotated with cos/sin [T,hd] (f32, already gathered by position_ids)."""

    @staticmethod
    def forward(ctx, x, cos, sin):
        x = x.contiguous()
        bs, T, nh, hd = x.shape
        y = torch.empty_like(x)
        for b in range(bs):
            C.call("oq_rope", x.data_ptr() + b * T * nh * hd * x.element_size(),
                   y.data_ptr() + b * T * nh * hd * x.element_size(), C.dt(x), T, nh, hd, C.fptr(cos), C.fptr(sin), 0,
                   C.stream())
        ctx.save_for_backward(cos, sin)
        return y

    @staticmethod
    def backward(ctx, gy):
        cos, sin = ctx.saved_tensors
        gy = gy.contiguous()
        bs, T, nh, hd = gy.shape
        gx = torch.empty_like(gy)
        for b in range(bs):
            C.call("oq_rope", gy.data_ptr() + b * T * nh * hd * gy.element_size(),
                   gx.data_ptr() + b * T * nh * hd * gy.element_size(), C.dt(gy), T, nh, hd, C.fptr(cos), C.fptr(sin), 1,
                   C.stream())
        return gx, None, None


class SiluMulFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):
        gate, up = gate.contiguous(), up.contiguous()
        y = torch.empty_like(gate)
        C.call("oq_silu_mul_fwd", C.ptr(gate), C.ptr(up), C.ptr(y), C.dt(gate), gate.numel(), C.stream())
        ctx.save_for_backward(gate, up)
        return y

    @staticmethod
    def backward(ctx, gy):
        gate, up = ctx.saved_tensors
        gy = gy.contiguous()
        gg, gu = torch.empty_like(gate), torch.empty_like(up)
        C.call("oq_silu_mul_bwd", C.ptr(gate), C.ptr(up), C.ptr(gy), C.ptr(gg), C.ptr(gu), C.dt(gate), gate.numel(),
               C.stream())
        return gg, gu


def silu_mul_quant_supported(gate, nbits):
    """The fused silu*up -> per-token fake-quant kernels take bf16 / f32 rows of 512 .. 32768 elements (multiple of 8).
    OQ_NO_FUSED_SILUQ=1 is an A/B switch."""
    if os.environ.get("OQ_NO_FUSED_SILUQ"):
        return False
    k = gate.shape[-1]
    return gate.is_cuda and gate.dtype in (torch.bfloat16, torch.float32) and 2 <= nbits < 16 and k % 8 == 0 and 512 <= k <= 32768


class StackedGateUpFn(torch.autograd.Function):
    """act = silu(x @ Wg.T + bg) * (x @ Wu.T + bu), optionally followed by the down_proj input quantiser (nbits in 2..15, as
    SiluMulQuantFn), for gate / up weights that are the two row blocks of ONE buffer (stacked_rows): the projections are one
    GEMM with N = 2*I whose output holds gate | up as column blocks, the silu*up (-> quant) kernels read those blocks through a
    row stride, and the backward is one kernel writing dgate | dup into one buffer, ONE dgrad GEMM (K = 2*I: the two input
    gradients are summed in the fp32 accumulators), ONE wgrad GEMM (M = 2*I) and one bias column sum.
    models/int_llama_layer.py:44-45 + quantize/int_linear.py:48-65."""

    @staticmethod
    def forward(ctx, x, wg, bg, wu, bu, nbits, stash, sib=None, xint=None, wints=None):
        ctx.sib = sib
        ctx.park_wgrad = bool(getattr(wg, "_oq_fq_out", False) and getattr(wu, "_oq_fq_out", False))
        x2 = x.contiguous().view(-1, x.shape[-1])
        rows, K = x2.shape
        wall = stacked_rows([wg, wu])
        ball = stacked_vectors([bg, bu])
        if wall is None or ball is False or wg.shape != wu.shape:
            raise C.OQError("StackedGateUpFn: gate / up weights (and biases) must lie back to back in one buffer")
        if wall.dtype != x2.dtype:
            raise C.OQError(f"StackedGateUpFn: weight dtype {wall.dtype} != activation dtype {x2.dtype}")
        I = wg.shape[0]
        nbits = int(nbits or 0)
        wint = stacked_int(list(wints)) if (xint is not None and wints is not None) else None
        if wint is not None and (tuple(xint.codes.shape) != (rows, K) or tuple(wint.codes.shape) != (2 * I, K)):
            wint = None
        # integer path: the exact projection result stays fp32 when a quantiser reads it next (silu * up -> down_proj input)
        pre_dtype = int_pre_dtype(x2.dtype, "mlp") if (wint is not None and nbits) else x2.dtype
        pre = torch.empty((rows, 2 * I), dtype=pre_dtype, device=x2.device)
        es = pre.element_size()
        if wint is not None:
            gemm_i8(xint, wint, pre, bias=ball)
        else:
            gemm(x2, wall, pre, rows, 2 * I, K, K, K, 2 * I, True, True, bias=ball)
        y = torch.empty((rows, I), dtype=x2.dtype, device=x2.device)
        if nbits:
            scale, zp, xmin, xmax = (torch.empty((rows, 1), dtype=torch.float32, device=x2.device) for _ in range(4))
            codes = csum = None
            if stash is not None and stash.get("want_int") and nbits <= 8:
                codes = torch.empty((rows, I), dtype=torch.int8, device=x2.device)
                csum = torch.empty((rows,), dtype=torch.float32, device=x2.device)
            C.call("oq_silu_mul_quant_fwd", pre.data_ptr(), pre.data_ptr() + I * es, C.dt(pre), rows, I, 2 * I, nbits, C.ptr(y),
                   C.dt(y), C.fptr(scale), C.fptr(zp), C.fptr(xmin), C.fptr(xmax), C.ptr(codes), C.fptr(csum), C.stream())
            if stash is not None:
                stash["scale"], stash["zp"] = scale, zp
                if codes is not None:
                    stash["int"] = IntCodes(codes, scale.view(-1), zp.view(-1), csum, nbits)
            ctx.save_for_backward(x2, wg, wu, pre, xmin, xmax)
        else:
            C.call("oq_silu_mul_fwd_2d", pre.data_ptr(), pre.data_ptr() + I * es, C.ptr(y), C.dt(pre), rows, I, 2 * I, C.stream())
            ctx.save_for_backward(x2, wg, wu, pre)
        ctx.cfg = (nbits, bg is not None, x.shape)
        return y.view(*x.shape[:-1], I)

    @staticmethod
    def backward(ctx, gy):
        nbits, has_bias, xshape = ctx.cfg
        if nbits:
            x2, wg, wu, pre, xmin, xmax = ctx.saved_tensors
        else:
            x2, wg, wu, pre = ctx.saved_tensors
        rows, K = x2.shape
        I = wg.shape[0]
        es = x2.element_size()
        gy = gy.contiguous()
        if gy.dtype != x2.dtype:
            gy = gy.to(x2.dtype)
        gpre = torch.empty((rows, 2 * I), dtype=x2.dtype, device=x2.device)
        if nbits:
            C.call("oq_silu_mul_quant_bwd", pre.data_ptr(), pre.data_ptr() + I * pre.element_size(), C.ptr(gy), C.dt(pre), C.dt(gy),
                   rows, I, 2 * I, nbits, C.fptr(xmin), C.fptr(xmax), gpre.data_ptr(), gpre.data_ptr() + I * es, C.stream())
        else:
            C.call("oq_silu_mul_bwd_2d", pre.data_ptr(), pre.data_ptr() + I * es, C.ptr(gy), gpre.data_ptr(),
                   gpre.data_ptr() + I * es, C.dt(pre), rows, I, 2 * I, C.stream())
        need = ctx.needs_input_grad          # x, wg, bg, wu, bu
        wall = stacked_rows([wg, wu])
        gx = gwg = gwu = gbg = gbu = None
        if need[0]:
            gx2 = torch.empty((rows, K), dtype=x2.dtype, device=x2.device)
            gemm(gpre, wall, gx2, rows, K, 2 * I, 2 * I, K, K, True, False)
            gx = gx2.view(xshape)
            if ctx.sib is not None:
                gx = ctx.sib.offer(gx)
        if need[1] or need[3]:
            gwall = torch.empty((2 * I, K), dtype=wall.dtype, device=x2.device)
            wgrad(gpre, x2, gwall, 2 * I, K, rows, 2 * I, K, K, park=ctx.park_wgrad)
            gwg, gwu = (gwall[:I] if need[1] else None), (gwall[I:] if need[3] else None)
        if has_bias and (need[2] or need[4]):
            gb = torch.empty((2 * I,), dtype=torch.float32, device=x2.device)
            ws_n = C.size_call("oq_colsum_workspace", rows, 2 * I)
            wsb = torch.empty(ws_n, dtype=torch.float32, device=x2.device)
            C.call("oq_colsum", C.ptr(gpre), C.dt(gpre), rows, 2 * I, C.fptr(gb), C.fptr(wsb), ws_n, C.stream())
            gbg, gbu = (gb[:I] if need[2] else None), (gb[I:] if need[4] else None)
        return gx, gwg, gbg, gwu, gbu, None, None, None, None, None


class SiluMulQuantFn(torch.autograd.Function):
    """y = per_token_fake_quant(silu(gate) * up): QuantLlamaMLP's act_fn(gate) * up (models/int_llama_layer.py:44-45)
    fused with the down_proj input quantiser (quantize/int_linear.py:59-60, quantize/quantizer.py:84-147).  One kernel per
    direction; the product stays in fp32 registers between the two reference steps."""

    @staticmethod
    def forward(ctx, gate, up, nbits, stash):
        gate, up = gate.contiguous(), up.contiguous()
        cols = gate.shape[-1]
        rows = gate.numel() // cols
        y = torch.empty_like(gate)
        scale, zp, xmin, xmax = (torch.empty((rows, 1), dtype=torch.float32, device=gate.device) for _ in range(4))
        codes = csum = None
        if stash is not None and stash.get("want_int") and int(nbits) <= 8:
            codes = torch.empty((rows, cols), dtype=torch.int8, device=gate.device)
            csum = torch.empty((rows,), dtype=torch.float32, device=gate.device)
        C.call("oq_silu_mul_quant_fwd", C.ptr(gate), C.ptr(up), C.dt(gate), rows, cols, 0, int(nbits), C.ptr(y), C.dt(y),
               C.fptr(scale), C.fptr(zp), C.fptr(xmin), C.fptr(xmax), C.ptr(codes), C.fptr(csum), C.stream())
        if stash is not None:
            stash["scale"], stash["zp"] = scale, zp
            if codes is not None:
                stash["int"] = IntCodes(codes, scale.view(-1), zp.view(-1), csum, int(nbits))
        ctx.save_for_backward(gate, up, xmin, xmax)
        ctx.nbits = int(nbits)
        return y

    @staticmethod
    def backward(ctx, gy):
        gate, up, xmin, xmax = ctx.saved_tensors
        gy = gy.contiguous()
        if gy.dtype != gate.dtype:
            gy = gy.to(gate.dtype)
        cols = gate.shape[-1]
        rows = gate.numel() // cols
        gg, gu = torch.empty_like(gate), torch.empty_like(up)
        C.call("oq_silu_mul_quant_bwd", C.ptr(gate), C.ptr(up), C.ptr(gy), C.dt(gate), C.dt(gy), rows, cols, 0, ctx.nbits,
               C.fptr(xmin), C.fptr(xmax), C.ptr(gg), C.ptr(gu), C.stream())
        return gg, gu, None, None


class ReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        C.call("oq_relu_fwd", C.ptr(x), C.ptr(y), C.dt(x), x.numel(), C.stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        C.call("oq_relu_bwd", C.ptr(x), C.ptr(gy), C.ptr(gx), C.dt(x), x.numel(), C.stream())
        return gx


class SoftmaxFn(torch.autograd.Function):
    """p = softmax(max(s*alpha + mask, finfo.min)) in f32 (models/int_llama_layer.py:143-160).

    s [bs, nh, T, Tk].  mask: None, one [T, Tk] mask shared by every sample and head, or the reference's
    [bs, 1, T, Tk] additive mask -- each sample then gets ITS mask (one launch per sample when they differ)."""

    @staticmethod
    def forward(ctx, s, mask, alpha, causal=False):
        s = s.contiguous()
        cols = s.shape[-1]
        rows = s.numel() // cols
        p = torch.empty_like(s)
        causal = bool(causal) and s.shape[-2] == cols
        per_sample = None
        m32, mrows = None, 0
        if mask is not None and not causal:
            m = mask.detach()
            if m.dim() == 4:
                if m.shape[1] != 1 or tuple(m.shape[-2:]) != tuple(s.shape[-2:]):
                    raise C.OQError(f"SoftmaxFn: mask {tuple(m.shape)} does not fit scores {tuple(s.shape)}")
                if m.shape[0] == 1 or m.stride(0) == 0:
                    m = m[0, 0]                                      # one mask broadcast over the batch
                elif s.dim() != 4 or m.shape[0] != s.shape[0]:
                    raise C.OQError(f"SoftmaxFn: mask batch {m.shape[0]} != scores batch {tuple(s.shape)}")
                else:
                    per_sample = m[:, 0].float().contiguous()         # [bs, T, Tk]
            if per_sample is None:
                if m.dim() != 2 or m.shape[-1] != cols:
                    raise C.OQError(f"SoftmaxFn: mask {tuple(m.shape)} does not fit scores {tuple(s.shape)}")
                m32 = m.float().contiguous().view(-1, cols)
                mrows = m32.shape[0]
        if per_sample is not None:
            bs = s.shape[0]
            rps = rows // bs
            es = s.element_size()
            for b in range(bs):
                C.call("oq_softmax_fwd", s.data_ptr() + b * rps * cols * es, p.data_ptr() + b * rps * cols * es, C.dt(s),
                       rps, cols, float(alpha), C.fptr(per_sample[b]), per_sample.shape[1], 0, C.stream())
        else:
            C.call("oq_softmax_fwd", C.ptr(s), C.ptr(p), C.dt(s), rows, cols, float(alpha), C.fptr(m32), mrows,
                   int(causal), C.stream())
        ctx.save_for_backward(p)
        ctx.alpha = float(alpha)
        ctx.causal = causal
        return p

    @staticmethod
    def backward(ctx, gp):
        (p,) = ctx.saved_tensors
        gp = gp.contiguous()
        cols = p.shape[-1]
        rows = p.numel() // cols
        gs = torch.empty_like(p)
        C.call("oq_softmax_bwd", C.ptr(p), C.ptr(gp), C.ptr(gs), C.dt(p), rows, cols, ctx.alpha, int(ctx.causal),
               C.stream())
        return gs, None, None, None


def fused_attention_supported(q, causal):
    """The fused causal-attention kernels cover bf16, head_dim 128, T == 128 or T % 256 == 0 and the exact causal mask; anything
    else runs the unfused HIP kernels (oq_gemm + oq_softmax_*).  OQ_NO_FLASH=1 is an A/B switch."""
    if os.environ.get("OQ_NO_FLASH") or not causal or q.dim() != 4:
        return False
    return bool(C.size_call("oq_attn_supported", C.dt(q), q.shape[1], q.shape[3], 1))


def fused_attention_shape_supported(dtype, T, hd):
    """fused_attention_supported for a problem whose q does not exist yet (exact causal mask assumed)."""
    if os.environ.get("OQ_NO_FLASH") or dtype not in C._DT:
        return False
    return bool(C.size_call("oq_attn_supported", C._DT[dtype], int(T), int(hd), 1))


class FusedCausalAttnFn(torch.autograd.Function):
    """o = softmax(scale * q k^T + causal mask) v without materialising scores / probabilities
    (models/int_llama_layer.py:143-163 with the p-quantiser at its 16-bit identity).  q [bs,T,nh,hd];
    k, v [bs,T,nkv,hd] -> o [bs,T,nh,hd].  Backward: oq_attn_bwd (dK, dV, dS^T) + one causal oq_gemm for dQ.
    grid = (sq, sk, sv): q / k / v hold the head quantisers' grid coordinates (QKVRopeQuantFn(grid=True)) and sq / sk / sv
    [rows, heads, 1] are views of their merged per-(token, head) scale vector: the products contract the coordinates exactly
    (oq_attn_*_grid) and the incoming / outgoing gradients are still those of the fake-quantised VALUES.  stash (dict):
    receives "wide" = the output in float32 (side channel for the o_proj input quantiser; the returned tensor is its bf16 copy)."""

    @staticmethod
    def forward(ctx, q, k, v, scale, grid=None, stash=None):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        bs, T, nh, hd = q.shape
        nkv = k.shape[2]
        o = torch.empty_like(q)
        lse = torch.empty((bs, nh, T), dtype=torch.float32, device=q.device)
        ctx.grid = grid is not None
        if grid is not None:
            sq, sk, sv = grid
            ld_s = sq.stride(0)
            for s_, n in ((sq, nh), (sk, nkv), (sv, nkv)):
                if (s_.dtype != torch.float32 or tuple(s_.shape[:2]) != (bs * T, n) or s_.stride(0) != ld_s or s_.stride(1) != 1
                        or q.dtype != torch.bfloat16):
                    raise C.OQError("FusedCausalAttnFn: grid scales must be float32 [rows, heads(, 1)] views of one merged vector")
            o32 = torch.empty(q.shape, dtype=torch.float32, device=q.device) if stash is not None else None
            C.call("oq_attn_fwd_grid", C.ptr(q), C.ptr(k), C.ptr(v), sq.data_ptr(), sk.data_ptr(), sv.data_ptr(), ld_s, C.ptr(o),
                   C.fptr(o32), C.fptr(lse), bs, T, nh, nkv, hd, float(scale), 1, C.stream())
            if stash is not None:
                stash["wide"] = o32
            ctx.has_o32 = o32 is not None
            ctx.save_for_backward(q, k, v, o, lse, sq, sk, sv, *([o32] if o32 is not None else []))
        else:
            C.call("oq_attn_fwd", C.ptr(q), C.ptr(k), C.ptr(v), C.ptr(o), C.fptr(lse), C.dt(q), bs, T, nh, nkv, hd,
                   float(scale), 1, C.stream())
            ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = float(scale)
        return o

    @staticmethod
    def backward(ctx, go):
        o32 = None
        if ctx.grid:
            q, k, v, o, lse, sq, sk, sv = ctx.saved_tensors[:8]
            o32 = ctx.saved_tensors[8] if ctx.has_o32 else None
        else:
            q, k, v, o, lse = ctx.saved_tensors
        go = go.contiguous()
        bs, T, nh, hd = q.shape
        nkv = k.shape[2]
        rep = nh // nkv
        dsum = torch.empty_like(lse)
        ds_t = torch.empty((bs, nh, T, T), dtype=q.dtype, device=q.device)
        gk_full = torch.empty_like(q)
        gv_full = torch.empty_like(q)
        if ctx.grid:
            # (ds_t comes back scaled by sk[key]: the dQ GEMM below contracts it with the K coordinates)
            C.call("oq_attn_bwd_grid", C.ptr(q), C.ptr(k), C.ptr(v), sq.data_ptr(), sk.data_ptr(), sv.data_ptr(), sq.stride(0),
                   C.ptr(o), C.fptr(o32), C.ptr(go), C.fptr(lse), C.fptr(dsum), C.ptr(ds_t), C.ptr(gk_full), C.ptr(gv_full), bs, T,
                   nh, nkv, hd, ctx.scale, 1, C.stream())
        else:
            C.call("oq_attn_bwd", C.ptr(q), C.ptr(k), C.ptr(v), C.ptr(o), C.ptr(go), C.fptr(lse), C.fptr(dsum), C.ptr(ds_t),
                   C.ptr(gk_full), C.ptr(gv_full), C.dt(q), bs, T, nh, nkv, hd, ctx.scale, 1, C.stream())
        gq = torch.empty_like(q)
        for b in range(bs):
            # dQ[t,d] = sum_t' dS^T[t',t] K[t',d]   (contraction limited to t' < m0 + tile)
            gemm(ds_t, k, gq, T, hd, T, T, nkv * hd, nh * hd, False, False, batch_o=nkv, batch_i=rep,
                 sa=(rep * T * T, T * T), sb=(hd, 0), sc=(rep * hd, hd),
                 a_off=b * nh * T * T, b_off=b * T * nkv * hd, c_off=b * T * nh * hd, tri=2)
        if rep == 1:
            gk, gv = gk_full, gv_full
        else:
            gk, gv = group_sum(gk_full, nkv, rep, gv_full)       # dK and dV of the shared heads: one launch of ours
        return gq, gk, gv, None, None, None


def group_sum(x, nkv, rep, x2=None):
    """Backward of repeat_kv for grouped-query attention: x [bs, T, nkv * rep, hd] (query-head order: head h belongs to
    key-value head h // rep) -> [bs, T, nkv, hd], summed over the rep query heads of each group (oq_group_sum).  With x2 the
    same for a second tensor in the same launch.  Returns (y, y2)."""
    bs, T, nh, hd = x.shape
    if nh != nkv * rep or (x2 is not None and (x2.shape != x.shape or x2.dtype != x.dtype)):
        raise C.OQError(f"group_sum: shape {tuple(x.shape)} for nkv {nkv} rep {rep}")
    if x.dtype not in (torch.bfloat16, torch.float32) or hd % 8 != 0 or not x.is_cuda:
        y = x.view(bs, T, nkv, rep, hd).sum(dim=3)
        return y, (None if x2 is None else x2.view(bs, T, nkv, rep, hd).sum(dim=3))
    x = x.contiguous()
    y = torch.empty((bs, T, nkv, hd), dtype=x.dtype, device=x.device)
    y2 = None
    if x2 is not None:
        x2 = x2.contiguous()
        y2 = torch.empty_like(y)
    C.call("oq_group_sum", C.ptr(x), C.ptr(y), C.ptr(x2), C.ptr(y2), C.dt(x), bs * T * nkv, int(rep), hd, C.stream())
    return y, y2


class AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        y = torch.empty_like(a)
        C.call("oq_add", C.ptr(a), C.ptr(b), C.ptr(y), C.dt(a), a.numel(), C.stream())
        return y

    @staticmethod
    def backward(ctx, gy):
        return gy, gy


class ScaleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, s):
        a = a.contiguous()
        y = torch.empty_like(a)
        C.call("oq_scale", C.ptr(a), float(s), C.ptr(y), C.dt(a), a.numel(), C.stream())
        ctx.s = float(s)
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        gx = torch.empty_like(gy)
        C.call("oq_scale", C.ptr(gy), ctx.s, C.ptr(gx), C.dt(gy), gy.numel(), C.stream())
        return gx, None


class MSELossFn(torch.autograd.Function):
    """loss = mse(t1, out) (+ mse(t2, out)) as one fused kernel that also writes d loss / d out
    (quantize/omniquant.py:220-222).  Returns a 0-dim f32 tensor that stays on the device."""

    @staticmethod
    def forward(ctx, out, t1, t2):
        wide = wide_of(out) if out.dtype == torch.bfloat16 else None     # (the block output's un-rounded side channel)
        out, t1 = out.contiguous(), t1.contiguous()
        t2 = t2.contiguous() if t2 is not None else None
        loss = torch.empty((1 + 1024,), dtype=torch.float32, device=out.device)       # [0] result, [1:] kernel scratch
        g = torch.empty_like(out)
        src = wide.contiguous() if wide is not None else out
        C.call("oq_mse_fwd_bwd", C.ptr(src), C.dt(src), C.ptr(t1), C.ptr(t2), C.dt(out), out.numel(), 1.0, C.fptr(loss), C.ptr(g),
               C.stream())
        ctx.save_for_backward(g)
        return loss[0]

    @staticmethod
    def backward(ctx, gl):
        (g,) = ctx.saved_tensors
        # d loss is 1.0 in the calibration loop; a different upstream factor is applied with the scale kernel
        return ScaleByTensor.apply_raw(g, gl), None, None


class ScaleByTensor:
    @staticmethod
    def apply_raw(g, gl):
        # gl is a 0-dim tensor; avoid a host sync: multiply on device (plumbing op, 1 launch)
        return g * gl.to(g.dtype)


class LetVectorsFn(torch.autograd.Function):
    """All [hidden]-sized LET algebra of a block in one launch (forward) + one launch (backward):
    norm weight/bias re-parameterisation and the bias side of smooth_ln_fcs / smooth_fc_fc / smooth_q_k
    (models/transformation.py:24-69).  Inputs are float32 vectors of length hidden; biases may be None."""

    @staticmethod
    def forward(ctx, s1, h1, s2, h2, s3, h3, t, ws_q, ws_k, ws_v, ws_o, ln1_w, ln1_b, ln2_w, ln2_b, bq0, bk0, bv0, bo0):
        n = s1.numel()
        ins = [x.detach().contiguous() if x is not None else None
               for x in (s1, h1, s2, h2, s3, h3, t, ln1_w, ln1_b, ln2_w, ln2_b, ws_q, ws_k, ws_v, ws_o, bq0, bk0, bv0, bo0)]
        for x in ins:
            # the kernel reads n elements of every vector: a shorter one (GQA k/v projections with LET, which the
            # reference rejects with a broadcast error, models/transformation.py:63-69) must not get that far
            if x is not None and x.numel() != n:
                raise NotImplementedError(f"LET vector of {x.numel()} elements in a block of hidden size {n}: LET needs "
                                          "equal q/k/v output widths (no grouped-query attention)")
        outs = [torch.empty(n, dtype=torch.float32, device=s1.device) for _ in range(4)]
        b3 = torch.empty(3 * n, dtype=torch.float32, device=s1.device)     # b_q | b_k | b_v back to back: one bias vector
        outs += [b3[:n], b3[n:2 * n], b3[2 * n:]]                           # for the stacked q/k/v GEMM (stacked_vectors)
        outs.append(torch.empty(n, dtype=torch.float32, device=s1.device))
        C.call("oq_let_vectors_fwd", n, *[C.fptr(x) for x in ins], *[C.fptr(o) for o in outs], C.stream())
        ctx.save_for_backward(*[x for x in ins if x is not None])
        ctx.present = [x is not None for x in ins]
        ctx.route = [p if (p is not None and getattr(p, "_oq_grad_sink", None) is not None and _gradient_routing_on())
                     else None for p in (s1, h1, s2, h2, s3, h3, t)]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        saved = list(ctx.saved_tensors)
        ins = [saved.pop(0) if pres else None for pres in ctx.present]
        n = ins[0].numel()
        dev = ins[0].device
        g = [go.contiguous() if go is not None else torch.zeros(n, dtype=torch.float32, device=dev) for go in gouts]
        res = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(11)]
        C.call("oq_let_vectors_bwd", n, *[C.fptr(x) for x in ins], *[C.fptr(x) for x in g], *[C.fptr(x) for x in res],
               C.stream())
        pg = list(res[:7])
        for i, par in enumerate(ctx.route):
            if par is not None:
                par._oq_collector.add(par, pg[i])      # summed into the arena by GradCollector.flush()
                pg[i] = None
        return tuple(pg) + tuple(res[7:]) + (None,) * 8


def _ragged_lengths(fn, lengths, bs, device, past=0):
    """Validate per-sequence lengths (kvcache.PackedKVCache(ragged=True).lengths): an int32 [bs] tensor on `device`, which
    excludes a non-zero `past`.  Host checks of dtype, shape and device only: the values are never read."""
    if not torch.is_tensor(lengths) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (bs,):
        what = f"{tuple(lengths.shape)} {lengths.dtype}" if torch.is_tensor(lengths) else type(lengths).__name__
        raise C.OQError(f"{fn}: lengths must be an int32 [{bs}] tensor, got {what}")
    if lengths.device != device:
        raise C.OQError(f"{fn}: lengths on {lengths.device}, the cache on {device}")
    if past:
        raise C.OQError(f"{fn}: lengths (one past per sequence) excludes past = {past}")
    return lengths.contiguous()


PAGE_SIZES = (16, 32, 64, 128)


def _page_pool(fn, page_table, lengths, past, mask, bs, nkv, pools):
    """Validate paged storage (kvcache.PagedKVCache): `pools` = ((tensor, last dim, dtype), ...) are page pools
    [num_pages, nkv, PS, last dim] with PS in PAGE_SIZES, page_table an int32 [bs, max_pages] tensor on their device; paged
    storage is ragged, so it needs lengths and takes neither a past nor a mask.  Host checks of shape, dtype and device only:
    the values are never read.  Returns (contiguous table, max_pages, num_pages, PS)."""
    if lengths is None:
        raise C.OQError(f"{fn}: page_table needs lengths (paged storage is ragged: an int32 [{bs}] device tensor)")
    if past:
        raise C.OQError(f"{fn}: page_table excludes past = {past} (each sequence's past is lengths[b])")
    if mask is not None:
        raise C.OQError(f"{fn}: page_table excludes a mask (row t of sequence b attends rows <= lengths[b] + t)")
    first = pools[0][0]
    if first is None or not torch.is_tensor(first) or first.dim() != 4:
        raise C.OQError(f"{fn}: page_table needs the page pools [num_pages, {nkv}, PS, ...] as the cache buffers")
    num_pages, ps = first.shape[0], first.shape[2]
    if ps not in PAGE_SIZES:
        raise C.OQError(f"{fn}: pool {tuple(first.shape)} has a page size of {ps} rows (one of {PAGE_SIZES})")
    for t, tail, dtype in pools:
        if not torch.is_tensor(t) or tuple(t.shape) != (num_pages, nkv, ps, tail) or t.dtype != dtype or num_pages <= 0 \
                or t.device != first.device:
            what = f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
            raise C.OQError(f"{fn}: pool {what} (expected [num_pages > 0, {nkv}, {ps}, {tail}] {dtype} on {first.device})")
    if not torch.is_tensor(page_table) or page_table.dtype != torch.int32 or page_table.dim() != 2 or page_table.shape[0] != bs \
            or page_table.shape[1] <= 0:
        what = f"{tuple(page_table.shape)} {page_table.dtype}" if torch.is_tensor(page_table) else type(page_table).__name__
        raise C.OQError(f"{fn}: page_table must be an int32 [{bs}, max_pages] tensor, got {what}")
    if page_table.device != first.device:
        raise C.OQError(f"{fn}: page_table on {page_table.device}, the pool on {first.device}")
    return page_table.contiguous(), page_table.shape[1], num_pages, ps


def _kv_append_args(fn, k, v, k_cache, v_cache, cache_dtype, past, q, cos, sin, positions, lengths=None):
    """What kv_append and kv_append_quant validate alike: the caches (None: no cache) against k, the row range (lengths: the
    kernel guards it), q, the cos / sin tables and the positions.  Returns (cap, nh, P, pos_bstride, contiguous positions)."""
    bs, Tq, nkv, hd = k.shape
    cap = 0
    if k_cache is not None:
        if v_cache is None or k_cache.dim() != 4 or tuple(k_cache.shape) != tuple(v_cache.shape) or \
                (k_cache.shape[0], k_cache.shape[1], k_cache.shape[3]) != (bs, nkv, hd) or k_cache.dtype != cache_dtype \
                or v_cache.dtype != cache_dtype:
            raise C.OQError(f"{fn}: cache {tuple(k_cache.shape)} {k_cache.dtype} does not fit k {tuple(k.shape)} {k.dtype}")
        cap = k_cache.shape[2]
        if lengths is None and (past < 0 or past + Tq > cap):
            raise C.OQError(f"{fn}: rows [{past}, {past + Tq}) beyond the capacity {cap}")
    nh = 0
    if q is not None:
        nh = q.shape[2]
        if q.dim() != 4 or tuple(q.shape[:2]) != (bs, Tq) or q.shape[3] != hd or q.dtype != k.dtype:
            raise C.OQError(f"{fn}: q {tuple(q.shape)} does not fit k {tuple(k.shape)}")
    P, pbs = 0, 0
    if cos is not None:
        if cos.dim() != 2 or cos.shape[1] != hd or tuple(sin.shape) != tuple(cos.shape):
            raise C.OQError(f"{fn}: cos / sin tables {tuple(cos.shape)} for head_dim {hd}")
        P = cos.shape[0]
        if positions is not None:
            if positions.dim() != 2 or positions.shape[1] != Tq or positions.shape[0] not in (1, bs) or positions.dtype != torch.int64:
                raise C.OQError(f"{fn}: positions {tuple(positions.shape)} {positions.dtype} (int64 [1 | {bs}, {Tq}])")
            positions = positions.contiguous()
            pbs = Tq if positions.shape[0] == bs and bs > 1 else 0
    return cap, nh, P, pbs, positions


def kv_append(k, v, k_cache, v_cache, past, q=None, q_out=None, k_out=None, cos=None, sin=None, positions=None, lengths=None,
              page_table=None):
    """Append one step's k / v [bs, Tq, nkv, hd] to rows [past, past + Tq) of the [bs, nkv, cap, hd] caches in ONE launch
    (csrc/oq_decode.hip), rotating q (into q_out) and k with the cos / sin tables [P, hd] (rows = positions 0..P-1) gathered at
    `positions` (int64 [1 | bs, Tq]; None = past + t).  cos None: no rotation (OPT).  k_out: optional [bs, Tq, nkv, hd] copy
    of the rotated k (the prefill's attention reads it).
    lengths (ragged batches; past must be 0): int32 [bs] on the cache's device, one past per sequence, read by the kernel
    only (oq_kv_append_ragged): sequence b's row t goes to cache row lengths[b] + t and, with positions None, rotates at that
    position.  A row outside [0, cap) is not stored to the cache (the kernel guards what the host cannot see).
    page_table (paged storage; needs lengths): int32 [bs, max_pages] on the device, and k_cache / v_cache are then the page
    pools [num_pages, nkv, PS, hd] (oq_kv_append_paged): logical row lengths[b] + t lives in page page_table[b, row // PS].  A
    row outside [0, max_pages * PS), or whose table entry is outside [0, num_pages), is not stored."""
    bs, Tq, nkv, hd = k.shape
    pages = None
    if page_table is not None:
        pages = _page_pool("kv_append", page_table, lengths, past, None, bs, nkv, ((k_cache, hd, k.dtype), (v_cache, hd, k.dtype)))
    if lengths is not None:
        lengths = _ragged_lengths("kv_append", lengths, bs, k_cache.device, past)
    if tuple(v.shape) != tuple(k.shape) or v.dtype != k.dtype:
        raise C.OQError(f"kv_append: k {tuple(k.shape)} / v {tuple(v.shape)} differ")
    cap, nh, P, pbs, positions = _kv_append_args("kv_append", k, v, None if pages else k_cache, None if pages else v_cache, k.dtype,
                                                 past, q, cos, sin, positions, lengths)
    if q is not None:
        q = q.contiguous()
        q_out = q if q_out is None else q_out
    k, v = k.contiguous(), v.contiguous()
    ragged = lengths is not None
    if pages:
        C.call("oq_kv_append_paged", C.ptr(q), C.ptr(k), C.ptr(v), C.ptr(q_out), C.ptr(k_out), C.ptr(k_cache), C.ptr(v_cache), C.dt(k),
               bs, Tq, nh, nkv, hd, C.ptr(pages[0]), *pages[1:], C.ptr(lengths), C.fptr(cos), C.fptr(sin), P, C.ptr(positions), pbs,
               C.stream())
        return q_out
    C.call("oq_kv_append_ragged" if ragged else "oq_kv_append", C.ptr(q), C.ptr(k), C.ptr(v), C.ptr(q_out), C.ptr(k_out),
           C.ptr(k_cache), C.ptr(v_cache), C.dt(k), bs, Tq, nh, nkv, hd, cap, C.ptr(lengths) if ragged else int(past), C.fptr(cos),
           C.fptr(sin), P, C.ptr(positions), pbs, C.stream())
    return q_out


def _kv_quant_outs(fn, q, k, v, out_dtype, q_out, k_out, v_out):
    """What the quantising appends validate alike: the destinations of the fake-quant values.  Returns contiguous (q, k, v)."""
    for t in (k_out, v_out):
        if t is not None and (tuple(t.shape) != tuple(k.shape) or t.dtype != out_dtype or not t.is_contiguous()):
            raise C.OQError(f"{fn}: k_out / v_out must be contiguous tensors of k's shape in the output dtype")
    if q is not None:
        if q_out is None or tuple(q_out.shape) != tuple(q.shape) or q_out.dtype != out_dtype:
            raise C.OQError(f"{fn}: q_out must be a tensor of q's shape in the output dtype")
        q = q.contiguous()
    return q, k.contiguous(), v.contiguous()


def _code_bits(k_codes, hd):
    """The width of a code cache's codes from its buffers: rows of hd bytes are 8-bit codes, everything else counts as 4-bit
    (rows of hd // 2 bytes; _code_buffers / _page_pool then check the shape for the width)."""
    return 8 if torch.is_tensor(k_codes) and k_codes.dim() == 4 and k_codes.shape[3] == hd else 4


def _code_buffers(fn, k_codes, v_codes, k_meta, v_meta, bs, nkv, hd, bits=4):
    """Validate the four buffers of a code cache of `bits` (kvcache.PackedKVCache(code_bits=4 | 8)): code rows of hd // 2 resp.
    hd bytes; returns the capacity."""
    if hd not in (64, 128):
        raise C.OQError(f"{fn}: head_dim {hd} (a code cache covers 64 and 128)")
    row = hd if bits == 8 else hd // 2
    if k_codes.dim() != 4 or (k_codes.shape[0], k_codes.shape[1], k_codes.shape[3]) != (bs, nkv, row):
        raise C.OQError(f"{fn}: codes {tuple(k_codes.shape)} (expected [{bs}, {nkv}, cap, {row}])")
    cap = k_codes.shape[2]
    for t, tail, dtype in ((k_codes, row, torch.uint8), (v_codes, row, torch.uint8), (k_meta, 2, torch.float32),
                           (v_meta, 2, torch.float32)):
        if tuple(t.shape) != (bs, nkv, cap, tail) or t.dtype != dtype:
            raise C.OQError(f"{fn}: code-cache buffer {tuple(t.shape)} {t.dtype} (expected {(bs, nkv, cap, tail)} {dtype})")
    return cap


def kv_append_codes(k, v, out_dtype, k_codes, v_codes, k_meta, v_meta, past=0, q=None, q_out=None, k_out=None, v_out=None,
                    cos=None, sin=None, positions=None, lengths=None, page_table=None):
    """kv_append_quant on the 4-bit grid with a code cache as the destination (csrc/oq_decode.hip, oq_kv_append_quant_codes):
    rows [past, past + Tq) of k_codes / v_codes (uint8 [bs, nkv, cap, hd // 2]) receive the quantiser's codes and k_meta /
    v_meta (float32 [bs, nkv, cap, 2]) its (scale, zero-point); (code - zp) * scale is, bit for bit, what kv_append_quant
    writes to a float32 cache.  q_out / k_out / v_out receive the fake-quant values in out_dtype as they do there.
    lengths: as in kv_append (oq_kv_append_quant_codes_ragged).  page_table: as in kv_append, the four buffers being page pools
    [num_pages, nkv, PS, hd // 2 | 2] (oq_kv_append_quant_codes_paged).
    Code rows of hd bytes (k_codes [..., hd]: the 8-bit code cache of the weight-only blocks) select oq_kv_append_codes8 and
    its _ragged / _paged forms: k and v alone are quantised, on the 255-level grid whose row range contains zero (an all-zero
    row: codes 0, meta (0, 0), exact zeros); q_out receives the rotated q's values as kv_append gives them, and k_out / v_out
    the dequantised values (code - zp) * scale rounded once to out_dtype."""
    bs, Tq, nkv, hd = k.shape
    bits = _code_bits(k_codes, hd)
    row = hd if bits == 8 else hd // 2
    names = ("oq_kv_append_codes8_paged", "oq_kv_append_codes8_ragged", "oq_kv_append_codes8") if bits == 8 else \
        ("oq_kv_append_quant_codes_paged", "oq_kv_append_quant_codes_ragged", "oq_kv_append_quant_codes")
    width = () if bits == 8 else (4,)           # the 4-bit entry points take nbits
    pages = None
    if page_table is not None:
        pages = _page_pool("kv_append_codes", page_table, lengths, past, None, bs, nkv,
                           ((k_codes, row, torch.uint8), (v_codes, row, torch.uint8), (k_meta, 2, torch.float32),
                            (v_meta, 2, torch.float32)))
        if hd not in (64, 128):
            raise C.OQError(f"kv_append_codes: head_dim {hd} (a code cache covers 64 and 128)")
    if lengths is not None:
        lengths = _ragged_lengths("kv_append_codes", lengths, bs, k_codes.device, past)
    if tuple(v.shape) != tuple(k.shape) or v.dtype != k.dtype or k.dtype not in (torch.float32, out_dtype):
        raise C.OQError(f"kv_append_codes: k {tuple(k.shape)} {k.dtype} / v {tuple(v.shape)} {v.dtype} (float32 or {out_dtype})")
    _, nh, P, pbs, positions = _kv_append_args("kv_append_codes", k, v, None, None, out_dtype, past, q, cos, sin, positions)
    cap = 0 if pages else _code_buffers("kv_append_codes", k_codes, v_codes, k_meta, v_meta, bs, nkv, hd, bits)
    ragged = lengths is not None
    if not ragged and (past < 0 or past + Tq > cap):
        raise C.OQError(f"kv_append_codes: rows [{past}, {past + Tq}) beyond the capacity {cap}")
    if (k_out is None) != (v_out is None):
        raise C.OQError("kv_append_codes: k_out and v_out go together")
    q, k, v = _kv_quant_outs("kv_append_codes", q, k, v, out_dtype, q_out, k_out, v_out)
    if pages:
        C.call(names[0], C.ptr(q), C.ptr(k), C.ptr(v), C.dt(k), C.ptr(q_out), C.ptr(k_out), C.ptr(v_out),
               C.ptr(k_codes), C.ptr(v_codes), C.fptr(k_meta), C.fptr(v_meta), C._DT[out_dtype], bs, Tq, nh, nkv, hd, C.ptr(pages[0]),
               *pages[1:], C.ptr(lengths), C.fptr(cos), C.fptr(sin), P, C.ptr(positions), pbs, *width, C.stream())
        return q_out
    C.call(names[1] if ragged else names[2], C.ptr(q), C.ptr(k), C.ptr(v), C.dt(k),
           C.ptr(q_out), C.ptr(k_out), C.ptr(v_out), C.ptr(k_codes), C.ptr(v_codes), C.fptr(k_meta), C.fptr(v_meta), C._DT[out_dtype],
           bs, Tq, nh, nkv, hd, cap, C.ptr(lengths) if ragged else int(past), C.fptr(cos), C.fptr(sin), P, C.ptr(positions), pbs, *width,
           C.stream())
    return q_out


def kv_append_quant(k, v, nbits, out_dtype, k_cache=None, v_cache=None, past=0, q=None, q_out=None, k_out=None, v_out=None,
                    cos=None, sin=None, positions=None, lengths=None, page_table=None):
    """kv_append for the W4A4 packed blocks (csrc/oq_decode.hip, oq_kv_append_quant): q / k / v [bs, Tq, heads, hd] in float32
    or out_dtype are rotated (q, k; cos None: no rotation) exactly as kv_append rotates them, from fp32, then quantised per
    (token, head) over hd on the nbits asymmetric grid; the fake-quant values go, in out_dtype, to q_out, to cache rows
    [past, past + Tq) and to k_out / v_out.  The caches may be None (the no-cache forward: k_out and v_out then).
    lengths: as in kv_append (oq_kv_append_quant_ragged; it needs the caches).  page_table: as in kv_append, k_cache / v_cache
    being the page pools in out_dtype (oq_kv_append_quant_paged)."""
    bs, Tq, nkv, hd = k.shape
    pages = None
    if page_table is not None:
        pages = _page_pool("kv_append_quant", page_table, lengths, past, None, bs, nkv,
                           ((k_cache, hd, out_dtype), (v_cache, hd, out_dtype)))
    if lengths is not None:
        if k_cache is None:
            raise C.OQError("kv_append_quant: lengths without a cache")
        lengths = _ragged_lengths("kv_append_quant", lengths, bs, k_cache.device, past)
    if tuple(v.shape) != tuple(k.shape) or v.dtype != k.dtype or k.dtype not in (torch.float32, out_dtype):
        raise C.OQError(f"kv_append_quant: k {tuple(k.shape)} {k.dtype} / v {tuple(v.shape)} {v.dtype} (float32 or {out_dtype})")
    cap, nh, P, pbs, positions = _kv_append_args("kv_append_quant", k, v, None if pages else k_cache, None if pages else v_cache,
                                                 out_dtype, past, q, cos, sin, positions, lengths)
    q, k, v = _kv_quant_outs("kv_append_quant", q, k, v, out_dtype, q_out, k_out, v_out)
    if pages:
        C.call("oq_kv_append_quant_paged", C.ptr(q), C.ptr(k), C.ptr(v), C.dt(k), C.ptr(q_out), C.ptr(k_out), C.ptr(v_out),
               C.ptr(k_cache), C.ptr(v_cache), C._DT[out_dtype], bs, Tq, nh, nkv, hd, C.ptr(pages[0]), *pages[1:], C.ptr(lengths),
               C.fptr(cos), C.fptr(sin), P, C.ptr(positions), pbs, int(nbits), C.stream())
        return q_out
    ragged = lengths is not None
    C.call("oq_kv_append_quant_ragged" if ragged else "oq_kv_append_quant", C.ptr(q), C.ptr(k), C.ptr(v), C.dt(k), C.ptr(q_out),
           C.ptr(k_out), C.ptr(v_out), C.ptr(k_cache), C.ptr(v_cache), C._DT[out_dtype], bs, Tq, nh, nkv, hd, cap,
           C.ptr(lengths) if ragged else int(past), C.fptr(cos), C.fptr(sin), P, C.ptr(positions), pbs, int(nbits), C.stream())
    return q_out


def act_codes(x2, nbits, out=None):
    """Per-token asymmetric quantiser (quantize/quantizer.py:84-147) of the rows of x2 [rows, cols] (float32 / bfloat16) ->
    IntCodes (csrc/oq_packed_a4.hip, oq_quant_codes: the arithmetic of every quantiser kernel).  out: optional destination of
    the fake-quant values (float32 / bfloat16 [rows, cols])."""
    if x2.dim() != 2 or x2.dtype not in (torch.float32, torch.bfloat16):
        raise C.OQError(f"act_codes: rows of float32 / bfloat16 expected, got {tuple(x2.shape)} {x2.dtype}")
    rows, cols = x2.shape
    x2 = x2.contiguous()
    codes = torch.empty((rows, cols), dtype=torch.int8, device=x2.device)
    vec = torch.empty((3, rows), dtype=torch.float32, device=x2.device)
    if rows:
        C.call("oq_quant_codes", C.ptr(x2), C.dt(x2), rows, cols, int(nbits), C.ptr(out), C.dt(out) if out is not None else 0,
               C.fptr(vec[0]), C.fptr(vec[1]), C.ptr(codes), C.fptr(vec[2]), C.stream())
    return IntCodes(codes, vec[0], vec[1], vec[2], int(nbits))


def _ragged_decode_args(fn, lengths, bs, device, mask, Tq, L, cap):
    """The lengths of a ragged decode attention, validated (they replace the mask: each query row sees its own past), and the
    bound L the launches are planned with."""
    if mask is not None:
        raise C.OQError(f"{fn}: lengths excludes a mask (row t of sequence b attends rows <= lengths[b] + t)")
    if not Tq <= int(L) <= cap:
        raise C.OQError(f"{fn}: the bound L = {L} of lengths + Tq must lie in [Tq = {Tq}, capacity = {cap}]")
    return _ragged_lengths(fn, lengths, bs, device)


def _decode_mask(fn, mask, bs, Tq, L):
    """The additive mask of a decode attention as (tensor kept alive, pointer, dtype, batch stride, row stride)."""
    if mask is None:
        return None, None, 0, 0, 0
    if mask.dim() != 4 or mask.shape[1] != 1 or tuple(mask.shape[2:]) != (Tq, L) or mask.shape[0] not in (1, bs):
        raise C.OQError(f"{fn}: mask {tuple(mask.shape)} (expected [{bs} | 1, 1, {Tq}, {L}])")
    if mask.stride(3) != 1:
        mask = mask.contiguous()
    return (mask, C.ptr(mask[:1, :1, :1, :1]), C.dt(mask), mask.stride(0) if mask.shape[0] == bs and bs > 1 else 0,
            mask.stride(2) if Tq > 1 else 0)


def decode_attention_codes(q, cache, L, scale, mask=None, out=None, workspace=None, lengths=None, page_table=None):
    """decode_attention over a 4-bit code cache (csrc/oq_decode.hip, oq_attn_decode_codes): `cache` is a PackedKVCache with
    code_bits 4 or the (k_codes, v_codes, k_meta, v_meta) buffers; K and V are dequantised in registers as (code - zp) * scale.
    Same scores, softmax, mask handling, split plan and reproducibility as decode_attention; q and o in the compute dtype.
    lengths: as in decode_attention (oq_attn_decode_codes_ragged).  page_table: as in decode_attention, `cache` being a
    PagedKVCache's four page pools or the cache itself (oq_attn_decode_codes_paged).
    An 8-bit code cache (code_bits 8, or buffers whose code rows have hd bytes) runs oq_attn_decode_codes8 and its _ragged /
    _paged forms: the same loops and sums on byte codes."""
    bs, Tq, nh, hd = q.shape
    bufs = cache if isinstance(cache, (tuple, list)) else (cache.k_codes, cache.v_codes, cache.k_meta, cache.v_meta)
    bits = _code_bits(bufs[0], hd) if isinstance(cache, (tuple, list)) else cache.code_bits
    row, sfx = (hd, "codes8") if bits == 8 else (hd // 2, "codes")
    pages = None
    if page_table is not None:
        if len(bufs) != 4 or not torch.is_tensor(bufs[0]) or bufs[0].dim() != 4:
            raise C.OQError("decode_attention_codes: page_table needs the (k_codes, v_codes, k_meta, v_meta) page pools")
        if hd not in (64, 128):
            raise C.OQError(f"decode_attention_codes: head_dim {hd} (a code cache covers 64 and 128)")
        nkv = bufs[0].shape[1]
        pages = _page_pool("decode_attention_codes", page_table, lengths, 0, mask, bs, nkv,
                           ((bufs[0], row, torch.uint8), (bufs[1], row, torch.uint8), (bufs[2], 2, torch.float32),
                            (bufs[3], 2, torch.float32)))
        cap = pages[1] * pages[3]
    else:
        if len(bufs) != 4 or bufs[0].dim() != 4 or bufs[0].shape[0] != bs:
            raise C.OQError(f"decode_attention_codes: (k_codes, v_codes, k_meta, v_meta) for a batch of {bs} expected")
        nkv = bufs[0].shape[1]
        cap = _code_buffers("decode_attention_codes", *bufs, bs, nkv, hd, bits)
    if lengths is not None:
        lengths = _ragged_decode_args("decode_attention_codes", lengths, bs, bufs[0].device, mask, Tq, L, cap)
    if q.dtype not in (torch.float32, torch.bfloat16):
        raise C.OQError(f"decode_attention_codes: q {q.dtype} (float32 or bfloat16)")
    q = q.contiguous()
    mask, mptr, mdt, mbs, mld = _decode_mask("decode_attention_codes", mask, bs, Tq, L)
    ws_n = C.size_call("oq_attn_decode_workspace", bs, nh, nkv, Tq, int(L), hd)
    if workspace is None or workspace.numel() * workspace.element_size() < ws_n:
        workspace = torch.empty(max(ws_n, 16), dtype=torch.uint8, device=q.device)
    o = torch.empty_like(q) if out is None else out
    if pages:
        C.call(f"oq_attn_decode_{sfx}_paged", C.ptr(q), C.ptr(bufs[0]), C.ptr(bufs[1]), C.fptr(bufs[2]), C.fptr(bufs[3]), C.ptr(o),
               C.dt(q), bs, Tq, nh, nkv, hd, C.ptr(pages[0]), *pages[1:], C.ptr(lengths), int(L), float(scale), C.ptr(workspace),
               workspace.numel() * workspace.element_size(), C.stream())
        return o
    if lengths is not None:
        C.call(f"oq_attn_decode_{sfx}_ragged", C.ptr(q), C.ptr(bufs[0]), C.ptr(bufs[1]), C.fptr(bufs[2]), C.fptr(bufs[3]), C.ptr(o),
               C.dt(q), bs, Tq, nh, nkv, hd, cap, C.ptr(lengths), int(L), float(scale), C.ptr(workspace),
               workspace.numel() * workspace.element_size(), C.stream())
        return o
    C.call(f"oq_attn_decode_{sfx}", C.ptr(q), C.ptr(bufs[0]), C.ptr(bufs[1]), C.fptr(bufs[2]), C.fptr(bufs[3]), C.ptr(o), C.dt(q),
           bs, Tq, nh, nkv, hd, cap, int(L), float(scale), mptr, mdt, mbs, mld, C.ptr(workspace),
           workspace.numel() * workspace.element_size(), C.stream())
    return o


def decode_attention(q, k_cache, v_cache, L, scale, mask=None, out=None, workspace=None, lengths=None, page_table=None):
    """o [bs, Tq, nh, hd] = softmax(max(scale * q k^T + mask, -FLT_MAX)) v over the first L rows of the [bs, nkv, cap, hd]
    caches (csrc/oq_decode.hip: split-L streaming, fp32 online softmax, one rounding).  mask: None or additive [bs | 1, 1, Tq, L]
    in float32 / float16 / bfloat16, read in place on the device (any batch / row stride; a batch of 1 is broadcast).
    lengths (ragged batches; mask must be None): int32 [bs] on the caches' device = the rows of each sequence BEFORE this step's
    append, read by the kernel only (oq_attn_decode_ragged).  L is then an upper bound of lengths[b] + Tq over the batch, L <= cap
    (launches and workspace depend on it, never on the values); query row t of sequence b attends rows j <= lengths[b] + t.
    page_table (paged storage; needs lengths, no mask): int32 [bs, max_pages] on the device, and k_cache / v_cache are then the
    page pools [num_pages, nkv, PS, hd] (oq_attn_decode_paged); L <= max_pages * PS.  A row whose table entry is outside
    [0, num_pages) is invisible.  On the same rows, lengths and L the output is the contiguous ragged call's bit for bit."""
    bs, Tq, nh, hd = q.shape
    pages = None
    if page_table is not None:
        if not torch.is_tensor(k_cache) or k_cache.dim() != 4:
            raise C.OQError("decode_attention: page_table needs the page pools [num_pages, nkv, PS, hd] as k_cache / v_cache")
        nkv = k_cache.shape[1]
        pages = _page_pool("decode_attention", page_table, lengths, 0, mask, bs, nkv, ((k_cache, hd, q.dtype), (v_cache, hd, q.dtype)))
        cap = pages[1] * pages[3]
    else:
        if k_cache.dim() != 4 or tuple(k_cache.shape) != tuple(v_cache.shape) or k_cache.shape[0] != bs or k_cache.shape[3] != hd \
                or k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
            raise C.OQError(f"decode_attention: caches {tuple(k_cache.shape)} {k_cache.dtype} do not fit q {tuple(q.shape)} {q.dtype}")
        nkv, cap = k_cache.shape[1], k_cache.shape[2]
    if lengths is not None:
        lengths = _ragged_decode_args("decode_attention", lengths, bs, k_cache.device, mask, Tq, L, cap)
    q = q.contiguous()
    mask, mptr, mdt, mbs, mld = _decode_mask("decode_attention", mask, bs, Tq, L)
    ws_n = C.size_call("oq_attn_decode_workspace", bs, nh, nkv, Tq, int(L), hd)
    if workspace is None or workspace.numel() * workspace.element_size() < ws_n:
        workspace = torch.empty(max(ws_n, 16), dtype=torch.uint8, device=q.device)
    o = torch.empty_like(q) if out is None else out
    if pages:
        C.call("oq_attn_decode_paged", C.ptr(q), C.ptr(k_cache), C.ptr(v_cache), C.ptr(o), C.dt(q), bs, Tq, nh, nkv, hd,
               C.ptr(pages[0]), *pages[1:], C.ptr(lengths), int(L), float(scale), C.ptr(workspace),
               workspace.numel() * workspace.element_size(), C.stream())
        return o
    if lengths is not None:
        C.call("oq_attn_decode_ragged", C.ptr(q), C.ptr(k_cache), C.ptr(v_cache), C.ptr(o), C.dt(q), bs, Tq, nh, nkv, hd, cap,
               C.ptr(lengths), int(L), float(scale), C.ptr(workspace), workspace.numel() * workspace.element_size(), C.stream())
        return o
    C.call("oq_attn_decode", C.ptr(q), C.ptr(k_cache), C.ptr(v_cache), C.ptr(o), C.dt(q), bs, Tq, nh, nkv, hd, cap, int(L),
           float(scale), mptr, mdt, mbs, mld, C.ptr(workspace), workspace.numel() * workspace.element_size(), C.stream())
    return o


def extend_attention_supported(dtype, Tq, hd):
    """Whether extend_attention / extend_attention_codes cover a step (oq_attn_extend_supported): bfloat16, head_dim 64 or 128."""
    return dtype in C._DT and bool(C.size_call("oq_attn_extend_supported", C._DT[dtype], int(Tq), int(hd)))


def _extend_args(fn, q, lengths, bs, device, Tq, L, cap, nh, nkv, out, workspace):
    """What the two chunked-prefill attentions validate alike once the cache buffers are checked; returns (contiguous q, lengths,
    o, workspace, its size in bytes)."""
    if lengths is None:
        raise C.OQError(f"{fn}: lengths is required (an int32 [{bs}] device tensor: the rows of each sequence before this step)")
    lengths = _ragged_decode_args(fn, lengths, bs, device, None, Tq, L, cap)
    if not extend_attention_supported(q.dtype, Tq, q.shape[3]):
        raise C.OQError(f"{fn}: q {q.dtype} with head_dim {q.shape[3]} (bfloat16 with head_dim 64 or 128; decode_attention "
                        "serves the rest)")
    ws_n = C.size_call("oq_attn_extend_workspace", bs, nh, nkv, Tq, int(L), q.shape[3])
    if workspace is None or workspace.numel() * workspace.element_size() < ws_n:
        workspace = torch.empty(max(ws_n, 16), dtype=torch.uint8, device=q.device)
    q = q.contiguous()
    o = torch.empty_like(q) if out is None else out
    return q, lengths, o, workspace, workspace.numel() * workspace.element_size()


def extend_attention(q, k_cache, v_cache, L, scale, lengths, page_table=None, out=None, workspace=None):
    """Chunked-prefill attention: decode_attention's ragged form for steps of MANY query rows over a cache that has a past
    (csrc/oq_extend.hip: bf16 MFMA, 64-row K/V tiles through LDS shared by a GQA group's query heads, fp32 online softmax).
    q [bs, Tq, nh, hd] bfloat16, hd 64 or 128; caches [bs, nkv, cap, hd] bfloat16; lengths (required) int32 [bs] on the device,
    the rows of each sequence BEFORE this step's append; L an upper bound of lengths[b] + Tq, L <= cap.  Query row t of
    sequence b attends rows j <= lengths[b] + t; rows at or beyond lengths[b] + Tq are never read.  There is no mask.
    page_table: as in decode_attention (oq_attn_extend_paged), bit-identical to the slab call on the same rows."""
    bs, Tq, nh, hd = q.shape
    pages = None
    if page_table is not None:
        if not torch.is_tensor(k_cache) or k_cache.dim() != 4:
            raise C.OQError("extend_attention: page_table needs the page pools [num_pages, nkv, PS, hd] as k_cache / v_cache")
        nkv = k_cache.shape[1]
        pages = _page_pool("extend_attention", page_table, lengths, 0, None, bs, nkv, ((k_cache, hd, q.dtype), (v_cache, hd, q.dtype)))
        cap = pages[1] * pages[3]
    else:
        if k_cache.dim() != 4 or tuple(k_cache.shape) != tuple(v_cache.shape) or k_cache.shape[0] != bs or k_cache.shape[3] != hd \
                or k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
            raise C.OQError(f"extend_attention: caches {tuple(k_cache.shape)} {k_cache.dtype} do not fit q {tuple(q.shape)} {q.dtype}")
        nkv, cap = k_cache.shape[1], k_cache.shape[2]
    q, lengths, o, workspace, ws_n = _extend_args("extend_attention", q, lengths, bs, k_cache.device, Tq, L, cap, nh, nkv, out, workspace)
    if pages:
        C.call("oq_attn_extend_paged", C.ptr(q), C.ptr(k_cache), C.ptr(v_cache), C.ptr(o), C.dt(q), bs, Tq, nh, nkv, hd,
               C.ptr(pages[0]), *pages[1:], C.ptr(lengths), int(L), float(scale), C.ptr(workspace), ws_n, C.stream())
        return o
    C.call("oq_attn_extend", C.ptr(q), C.ptr(k_cache), C.ptr(v_cache), C.ptr(o), C.dt(q), bs, Tq, nh, nkv, hd, cap, C.ptr(lengths),
           int(L), float(scale), C.ptr(workspace), ws_n, C.stream())
    return o


def extend_attention_codes(q, cache, L, scale, lengths, page_table=None, out=None, workspace=None):
    """extend_attention over a 4-bit code cache (oq_attn_extend_codes): `cache` is a cache with code_bits 4 or its (k_codes,
    v_codes, k_meta, v_meta) buffers.  A row enters the MFMA as code - zero_point; its scale multiplies the score (K) and the
    probability (V) once per row, as in decode_attention_codes.  page_table: the buffers are page pools
    (oq_attn_extend_codes_paged).  An 8-bit code cache (code_bits 8, or code rows of hd bytes) runs oq_attn_extend_codes8 /
    _paged: its zero-points lie in [0, 255], so code - zero_point stays exact in bfloat16."""
    bs, Tq, nh, hd = q.shape
    bufs = cache if isinstance(cache, (tuple, list)) else (cache.k_codes, cache.v_codes, cache.k_meta, cache.v_meta)
    bits = _code_bits(bufs[0], hd) if isinstance(cache, (tuple, list)) else cache.code_bits
    row, sfx = (hd, "codes8") if bits == 8 else (hd // 2, "codes")
    if len(bufs) != 4 or not torch.is_tensor(bufs[0]) or bufs[0].dim() != 4:
        raise C.OQError("extend_attention_codes: (k_codes, v_codes, k_meta, v_meta) buffers or page pools expected")
    nkv = bufs[0].shape[1]
    pages = None
    if page_table is not None:
        if hd not in (64, 128):
            raise C.OQError(f"extend_attention_codes: head_dim {hd} (a code cache covers 64 and 128)")
        pages = _page_pool("extend_attention_codes", page_table, lengths, 0, None, bs, nkv,
                           ((bufs[0], row, torch.uint8), (bufs[1], row, torch.uint8), (bufs[2], 2, torch.float32),
                            (bufs[3], 2, torch.float32)))
        cap = pages[1] * pages[3]
    else:
        if bufs[0].shape[0] != bs:
            raise C.OQError(f"extend_attention_codes: (k_codes, v_codes, k_meta, v_meta) for a batch of {bs} expected")
        cap = _code_buffers("extend_attention_codes", *bufs, bs, nkv, hd, bits)
    q, lengths, o, workspace, ws_n = _extend_args("extend_attention_codes", q, lengths, bs, bufs[0].device, Tq, L, cap, nh, nkv, out,
                                                  workspace)
    if pages:
        C.call(f"oq_attn_extend_{sfx}_paged", C.ptr(q), C.ptr(bufs[0]), C.ptr(bufs[1]), C.fptr(bufs[2]), C.fptr(bufs[3]), C.ptr(o),
               C.dt(q), bs, Tq, nh, nkv, hd, C.ptr(pages[0]), *pages[1:], C.ptr(lengths), int(L), float(scale), C.ptr(workspace),
               ws_n, C.stream())
        return o
    C.call(f"oq_attn_extend_{sfx}", C.ptr(q), C.ptr(bufs[0]), C.ptr(bufs[1]), C.fptr(bufs[2]), C.fptr(bufs[3]), C.ptr(o), C.dt(q),
           bs, Tq, nh, nkv, hd, cap, C.ptr(lengths), int(L), float(scale), C.ptr(workspace), ws_n, C.stream())
    return o


def tree_attention(q, cache, L, scale, lengths, tree, page_table=None, out=None, workspace=None):
    """Attention of a speculative TREE step (oq_attn_tree, the TREE form of csrc/oq_extend.hip): the Tq <= 64 rows of q
    [bs, Tq, nh, hd] (bfloat16, hd 64 or 128) are the nodes of `tree` (a kvcache.TokenTree, one tree for the batch or one per
    sequence; or its int32 [1 | bs, Tq, 2] `anc` tensor on the device), whose k / v rows the step has appended at rows
    lengths[b] + t.  Node t attends the committed past (rows < lengths[b]) plus itself and its ancestors, nothing else.
    `cache`: a ragged bfloat16 cache of any kind (PackedKVCache(ragged=True), PagedKVCache, a pool's layer view; float rows, 4-
    or 8-bit codes) or its buffers, (k, v) or (k_codes, v_codes, k_meta, v_meta); page_table: the buffers are page pools (taken
    from a paged cache object by itself).  lengths, L, out and workspace are extend_attention's, as are the split plan and the
    rows never read; with a chain as the tree the output is extend_attention's bit for bit.  Tree steps always run this kernel,
    also below block_common.EXTEND_MIN_TQ."""
    fn = "tree_attention"
    if not torch.is_tensor(q) or q.dim() != 4:
        raise C.OQError(f"{fn}: q must be a [bs, Tq, nh, hd] tensor")
    if not q.is_cuda:
        raise C.OQError(f"{fn}: q on {q.device}: the tree attention needs GPU tensors; there is no CPU fallback")
    bs, Tq, nh, hd = q.shape
    if isinstance(cache, (tuple, list)):
        bufs = tuple(cache)
    else:
        bufs = (cache.k, cache.v) if cache.code_bits is None else (cache.k_codes, cache.v_codes, cache.k_meta, cache.v_meta)
        if page_table is None and getattr(cache, "paged", False):
            page_table = cache.page_table
    if len(bufs) not in (2, 4) or not all(torch.is_tensor(t) and t.dim() == 4 for t in bufs):
        raise C.OQError(f"{fn}: a cache, its (k, v) buffers or its (k_codes, v_codes, k_meta, v_meta) buffers expected")
    if Tq > 64:
        raise C.OQError(f"{fn}: Tq {Tq} (a token tree has at most 64 nodes)")
    nkv = bufs[0].shape[1]
    if len(bufs) == 4:
        bits = _code_bits(bufs[0], hd)
        row = hd if bits == 8 else hd // 2
        kinds = ((bufs[0], row, torch.uint8), (bufs[1], row, torch.uint8), (bufs[2], 2, torch.float32), (bufs[3], 2, torch.float32))
    else:
        bits = 0
        kinds = ((bufs[0], hd, q.dtype), (bufs[1], hd, q.dtype))
    pages = None
    if page_table is not None:
        if hd not in (64, 128):
            raise C.OQError(f"{fn}: head_dim {hd} (64 or 128)")
        pages = _page_pool(fn, page_table, lengths, 0, None, bs, nkv, kinds)
        cap = pages[1] * pages[3]
    elif bits:
        if bufs[0].shape[0] != bs:
            raise C.OQError(f"{fn}: (k_codes, v_codes, k_meta, v_meta) for a batch of {bs} expected")
        cap = _code_buffers(fn, *bufs, bs, nkv, hd, bits)
    else:
        k_cache, v_cache = bufs
        if tuple(k_cache.shape) != tuple(v_cache.shape) or k_cache.shape[0] != bs or k_cache.shape[3] != hd \
                or k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
            raise C.OQError(f"{fn}: caches {tuple(k_cache.shape)} {k_cache.dtype} do not fit q {tuple(q.shape)} {q.dtype}")
        cap = k_cache.shape[2]
    from .kvcache import TokenTree
    if not torch.is_tensor(tree) and not isinstance(tree, TokenTree):
        raise C.OQError(f"{fn}: tree must be a kvcache.TokenTree or its int32 [1 | {bs}, {Tq}, 2] anc tensor, got {type(tree).__name__}")
    anc = tree if torch.is_tensor(tree) else tree.to(q.device).anc
    if anc.dtype != torch.int32 or anc.dim() != 3 or anc.shape[0] not in (1, bs) or tuple(anc.shape[1:]) != (Tq, 2):
        raise C.OQError(f"{fn}: the tree's ancestor sets {tuple(anc.shape)} {anc.dtype} (int32 [1 | {bs}, {Tq}, 2]: a tree of the "
                        "step's Tq nodes)")
    if anc.device != q.device:
        raise C.OQError(f"{fn}: the tree's ancestor sets on {anc.device}, q on {q.device}")
    anc = anc.contiguous()
    q, lengths, o, workspace, ws_n = _extend_args(fn, q, lengths, bs, bufs[0].device, Tq, L, cap, nh, nkv, out, workspace)
    meta = (C.fptr(bufs[2]), C.fptr(bufs[3])) if bits else (None, None)
    table = (C.ptr(pages[0]), *pages[1:]) if pages else (None, 0, 0, 0)
    C.call("oq_attn_tree", C.ptr(q), C.ptr(bufs[0]), C.ptr(bufs[1]), *meta, C.ptr(o), C.dt(q), bits, bs, Tq, nh, nkv, hd, cap, *table,
           C.ptr(lengths), int(L), C.ptr(anc), anc.shape[0], float(scale), C.ptr(workspace), ws_n, C.stream())
    return o


def kv_tree_commit(buffer, lengths, accept, page_table=None):
    """Make the accepted root path of a verified token tree a sequence's next rows (oq_kv_tree_commit, csrc/oq_kvpool.hip): in
    ONE launch over all layers, row lengths[b] + accept[b, i] of `buffer` moves to row lengths[b] + i, for i = 0, 1, ... while
    accept[b, i] is a valid entry (i <= accept[b, i] < Tq, strictly above the previous one; the first other value, the -1
    padding for one, ends sequence b's moves).  buffer: one buffer kind of a ragged cache, any dtype, contiguous:
    [bs, nkv, cap, x] or, for all layers at once, [layers, bs, nkv, cap, x]; with page_table (int32 [bs, max_pages]) the page
    pools [num_pages, nkv, PS, x] or [layers, num_pages, nkv, PS, x].  lengths int32 [bs] and accept int32 [bs, Tq] live on the
    buffer's device and are never read by the host.  Rows outside the capacity and pages the table does not hold are skipped.
    Only rows at or beyond lengths[b] are written.  Returns buffer."""
    fn = "kv_tree_commit"
    if not torch.is_tensor(buffer) or buffer.dim() not in (4, 5):
        what = f"{tuple(buffer.shape)}" if torch.is_tensor(buffer) else type(buffer).__name__
        raise C.OQError(f"{fn}: buffer must be a [(layers,) bs | num_pages, nkv, cap | PS, x] tensor, got {what}")
    if not buffer.is_cuda:
        raise C.OQError(f"{fn}: buffer on {buffer.device}: the commit needs GPU tensors; there is no CPU fallback")
    if not buffer.is_contiguous():
        raise C.OQError(f"{fn}: buffer {tuple(buffer.shape)} with strides {buffer.stride()} is not contiguous")
    layers = buffer.shape[0] if buffer.dim() == 5 else 1
    lead, nkv, rows, x = buffer.shape[-4:]
    row_bytes = x * buffer.element_size()
    if not torch.is_tensor(accept) or accept.dtype != torch.int32 or accept.dim() != 2 or not 1 <= accept.shape[1] <= 64:
        what = f"{tuple(accept.shape)} {accept.dtype}" if torch.is_tensor(accept) else type(accept).__name__
        raise C.OQError(f"{fn}: accept must be an int32 [bs, Tq <= 64] tensor, got {what}")
    bs, Tq = accept.shape
    if accept.device != buffer.device:
        raise C.OQError(f"{fn}: accept on {accept.device}, the buffer on {buffer.device}")
    lengths = _ragged_lengths(fn, lengths, bs, buffer.device)
    if page_table is not None:
        if rows not in PAGE_SIZES:
            raise C.OQError(f"{fn}: pool {tuple(buffer.shape)} has a page size of {rows} rows (one of {PAGE_SIZES})")
        if not torch.is_tensor(page_table) or page_table.dtype != torch.int32 or page_table.dim() != 2 or page_table.shape[0] != bs \
                or page_table.shape[1] <= 0 or page_table.device != buffer.device:
            what = f"{tuple(page_table.shape)} {page_table.dtype} on {page_table.device}" if torch.is_tensor(page_table) \
                else type(page_table).__name__
            raise C.OQError(f"{fn}: page_table must be an int32 [{bs}, max_pages] tensor on {buffer.device}, got {what}")
        page_table = page_table.contiguous()
        table = (C.ptr(page_table), page_table.shape[1], lead, rows)
        cap = 0
    else:
        if lead != bs:
            raise C.OQError(f"{fn}: buffer {tuple(buffer.shape)} for a batch of {bs} (accept {tuple(accept.shape)})")
        table, cap = (None, 0, 0, 0), rows
    C.call("oq_kv_tree_commit", C.ptr(buffer), row_bytes, layers, lead * nkv * rows * row_bytes, bs, nkv, cap, *table, C.ptr(lengths),
           C.ptr(accept.contiguous()), Tq, C.stream())
    return buffer


def _head_rows(fn, name, t, H=None):
    """A [rows, H] operand of the LM-head kernels: (tensor that holds it, rows, H, leading dimension).  A 2-D view whose rows are
    contiguous and a multiple of 8 elements apart is taken as it is (its padding is never read); anything else is copied."""
    if not torch.is_tensor(t) or t.dim() < 1:
        raise C.OQError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise C.OQError(f"{fn}: {name} on {t.device}: the LM-head kernels need GPU tensors; there is no CPU fallback")
    if t.dtype not in (torch.bfloat16, torch.float16):
        raise C.OQError(f"{fn}: {name} is {t.dtype} (bfloat16 or float16, the same for h and the head)")
    if H is not None and t.shape[-1] != H:
        raise C.OQError(f"{fn}: {name} {tuple(t.shape)} does not fit a hidden size of {H}")
    H = t.shape[-1]
    if H % 64 != 0 or not 64 <= H <= 16384:
        raise C.OQError(f"{fn}: hidden size {H} (a multiple of 64 from 64 to 16384)")
    if not (t.dim() == 2 and t.stride(1) == 1 and (t.shape[0] == 1 or (t.stride(0) >= H and t.stride(0) % 8 == 0))):
        t = t.reshape(-1, H).contiguous()
    rows = t.shape[0]
    if rows < 1:
        raise C.OQError(f"{fn}: {name} {tuple(t.shape)} has no rows")
    if t.data_ptr() % 16 != 0:
        t = t.clone(memory_format=torch.contiguous_format)
    return t, rows, H, (t.stride(0) if rows > 1 else H)


def _head_workspace(M, V, workspace, device):
    ws_n = C.size_call("oq_lm_head_workspace", M, V)
    if workspace is not None and (not torch.is_tensor(workspace) or workspace.device != device or not workspace.is_contiguous()):
        raise C.OQError(f"lm head: workspace must be a contiguous tensor on {device}")
    if workspace is None or workspace.numel() * workspace.element_size() < ws_n or workspace.data_ptr() % 8 != 0:
        workspace = torch.empty(max(ws_n, 16), dtype=torch.uint8, device=device)
    return workspace, workspace.numel() * workspace.element_size()


def lm_head_workspace(M, V):
    """Bytes of workspace lm_head_argmax / tree_verify_greedy use for M rows over a vocabulary of V (oq_lm_head_workspace)."""
    return C.size_call("oq_lm_head_workspace", int(M), int(V))


def lm_head_argmax(h, weight, out=None, logits=None, workspace=None):
    """Greedy token of every row without storing logits (oq_lm_head_argmax, csrc/oq_lmhead.hip): h [..., H] hidden rows after the
    final norm, weight [V, H] the head as nn.Linear.weight, both bfloat16 or both float16.  Returns (idx int32, val float32)
    shaped like h without its last dimension: idx = the lowest index of the row's largest logit h @ weight.T (fp32
    accumulation on the MFMA), val = that logit.  out: an (idx, val) pair to write into; logits: a float32 [..., V] tensor that
    also receives every logit; workspace: a device byte buffer of lm_head_workspace(M, V) bytes to reuse (one is allocated if it
    is missing or too small).  2-D views with padded rows (stride a multiple of 8 elements) are read in place."""
    fn = "lm_head_argmax"
    lead = tuple(h.shape[:-1]) if torch.is_tensor(h) else ()
    h2, M, H, ld_h = _head_rows(fn, "h", h)
    w2, V, _, ld_w = _head_rows(fn, "weight", weight, H)
    if weight.dim() != 2:
        raise C.OQError(f"{fn}: weight must be [V, H], got {tuple(weight.shape)}")
    if w2.dtype != h2.dtype or w2.device != h2.device:
        raise C.OQError(f"{fn}: h is {h2.dtype} on {h2.device}, weight {w2.dtype} on {w2.device}")
    if out is None:
        idx = torch.empty(lead, dtype=torch.int32, device=h2.device)
        val = torch.empty(lead, dtype=torch.float32, device=h2.device)
    else:
        idx, val = out
        for t, dt, name in ((idx, torch.int32, "idx"), (val, torch.float32, "val")):
            if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != lead or t.device != h2.device or not t.is_contiguous():
                raise C.OQError(f"{fn}: out {name} must be a contiguous {dt} {lead} tensor on {h2.device}")
    if logits is not None and (not torch.is_tensor(logits) or logits.dtype != torch.float32 or tuple(logits.shape) != lead + (V,)
                               or logits.device != h2.device or not logits.is_contiguous()):
        raise C.OQError(f"{fn}: logits must be a contiguous float32 {lead + (V,)} tensor on {h2.device}")
    workspace, ws_n = _head_workspace(M, V, workspace, h2.device)
    C.call("oq_lm_head_argmax", h2.data_ptr(), w2.data_ptr(), C.dt(h2), M, V, H, ld_h, ld_w, C.ptr(idx), C.fptr(val), C.fptr(logits),
           C.ptr(workspace), ws_n, C.stream())
    return idx, val


def tree_verify_greedy(h, weight, tree, draft, expect=None, workspace=None):
    """Greedy verification of a speculative tree step in two launches (oq_tree_verify_greedy, csrc/oq_lmhead.hip), nothing read
    by the host.  h [bs, Tq, H]: the tree step's output rows after the final norm (row t = node t); weight [V, H] the head; both
    bfloat16 or both float16.  tree: the step's kvcache.TokenTree (or its int32 [1 | bs, Tq, 2] anc tensor on the device); draft
    int32 [bs, Tq] on the device, the drafted token of every node, -1 for padding nodes (a sequence whose drafts are all -1 is
    inactive); expect int32 [bs] on the device, the token the model chose after the committed past (the previous step's
    next_token), or None to admit every root.  The rule is TokenTree.greedy_accept's.  Returns (accept int32 [bs, Tq] for
    commit_tree, counts int32 [bs], next_token int32 [bs], target int32 [bs, Tq], target_val float32 [bs, Tq])."""
    fn = "tree_verify_greedy"
    if not torch.is_tensor(h) or h.dim() != 3:
        raise C.OQError(f"{fn}: h must be a [bs, Tq, H] tensor")
    if not h.is_cuda:
        raise C.OQError(f"{fn}: h on {h.device}: the verification needs GPU tensors; there is no CPU fallback")
    bs, Tq, _ = h.shape
    if not 1 <= Tq <= 64:
        raise C.OQError(f"{fn}: Tq {Tq} (a token tree has 1 to 64 nodes)")
    h2, M, H, ld_h = _head_rows(fn, "h", h)
    w2, V, _, ld_w = _head_rows(fn, "weight", weight, H)
    if weight.dim() != 2:
        raise C.OQError(f"{fn}: weight must be [V, H], got {tuple(weight.shape)}")
    if w2.dtype != h2.dtype or w2.device != h2.device:
        raise C.OQError(f"{fn}: h is {h2.dtype} on {h2.device}, weight {w2.dtype} on {w2.device}")
    from .kvcache import TokenTree
    if isinstance(tree, TokenTree):
        if tree.bs not in (None, bs):
            raise C.OQError(f"{fn}: {tree!r} for a batch of {bs}")
        anc = tree.to(h.device).anc
    elif torch.is_tensor(tree):
        anc = tree
    else:
        raise C.OQError(f"{fn}: tree must be a kvcache.TokenTree or its int32 [1 | {bs}, {Tq}, 2] anc tensor, got {type(tree).__name__}")
    if anc.dtype != torch.int32 or anc.dim() != 3 or anc.shape[0] not in (1, bs) or tuple(anc.shape[1:]) != (Tq, 2):
        raise C.OQError(f"{fn}: the tree's ancestor sets {tuple(anc.shape)} {anc.dtype} (int32 [1 | {bs}, {Tq}, 2]: a tree of the "
                        "step's Tq nodes)")
    if anc.device != h.device:
        raise C.OQError(f"{fn}: the tree's ancestor sets on {anc.device}, h on {h.device}")
    if not torch.is_tensor(draft) or draft.dtype != torch.int32 or tuple(draft.shape) != (bs, Tq) or draft.device != h.device:
        what = f"{tuple(draft.shape)} {draft.dtype} on {draft.device}" if torch.is_tensor(draft) else type(draft).__name__
        raise C.OQError(f"{fn}: draft must be an int32 [{bs}, {Tq}] tensor on {h.device}, got {what}")
    if expect is not None and (not torch.is_tensor(expect) or expect.dtype != torch.int32 or tuple(expect.shape) != (bs,)
                               or expect.device != h.device):
        what = f"{tuple(expect.shape)} {expect.dtype} on {expect.device}" if torch.is_tensor(expect) else type(expect).__name__
        raise C.OQError(f"{fn}: expect must be None or an int32 [{bs}] tensor on {h.device}, got {what}")
    workspace, ws_n = _head_workspace(M, V, workspace, h.device)
    i32 = dict(dtype=torch.int32, device=h.device)
    accept, counts, next_token = torch.empty(bs, Tq, **i32), torch.empty(bs, **i32), torch.empty(bs, **i32)
    target, target_val = torch.empty(bs, Tq, **i32), torch.empty(bs, Tq, dtype=torch.float32, device=h.device)
    C.call("oq_tree_verify_greedy", h2.data_ptr(), w2.data_ptr(), C.dt(h2), bs, Tq, V, H, ld_h, ld_w, C.ptr(anc.contiguous()),
           anc.shape[0], C.ptr(draft.contiguous()), None if expect is None else C.ptr(expect.contiguous()), C.ptr(accept),
           C.ptr(counts), C.ptr(next_token), C.ptr(target), C.fptr(target_val), C.ptr(workspace), ws_n, C.stream())
    return accept, counts, next_token, target, target_val


def _kv_pages_args(fn, pool, ids, flat=None, flat_name=None):
    """Validate a page move of a model-wide pool (kvcache.PagedKVPool), on the host and before any device call: `ids` =
    ((name, tensor), ...) are int32 1-D tensors of one length on the pool's device, `pool` a contiguous [layers, num_pages, ...]
    tensor whose pages (everything behind the first two dimensions) are a multiple of 16 bytes, `flat` (gather's dst, scatter's
    src; None: no such buffer) a contiguous tensor of layers * n * page_bytes bytes on that device.  The values are never read.
    Returns (contiguous ids, layers, num_pages, page_bytes, n)."""
    if not torch.is_tensor(pool) or pool.dim() < 3:
        what = f"{tuple(pool.shape)} {pool.dtype}" if torch.is_tensor(pool) else type(pool).__name__
        raise C.OQError(f"{fn}: pool must be a [layers, num_pages, ...] tensor, got {what}")
    out = []
    for name, t in ids:
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1:
            what = f"{tuple(t.shape)} {t.dtype}" if torch.is_tensor(t) else type(t).__name__
            raise C.OQError(f"{fn}: {name} must be an int32 1-D device tensor, got {what}")
        if t.device != pool.device:
            raise C.OQError(f"{fn}: {name} on {t.device}, the pool on {pool.device}")
        if t.shape[0] != ids[0][1].shape[0]:
            raise C.OQError(f"{fn}: {name} names {t.shape[0]} pages, {ids[0][0]} {ids[0][1].shape[0]}")
        out.append(t.contiguous())
    n = out[0].shape[0]
    layers, num_pages = pool.shape[0], pool.shape[1]
    page_bytes = pool[0, 0].numel() * pool.element_size() if layers and num_pages else 0
    if page_bytes <= 0 or page_bytes % 16:
        raise C.OQError(f"{fn}: pool {tuple(pool.shape)} {pool.dtype} has pages of {page_bytes} bytes (page_bytes must be a "
                        "positive multiple of 16)")
    if not pool.is_contiguous():
        raise C.OQError(f"{fn}: pool {tuple(pool.shape)} with strides {pool.stride()} is not contiguous")
    if flat_name is not None:
        want = layers * n * page_bytes
        if not torch.is_tensor(flat) or not flat.is_contiguous() or flat.numel() * flat.element_size() != want:
            what = f"{tuple(flat.shape)} {flat.dtype}" + ("" if flat.is_contiguous() else " (not contiguous)") \
                if torch.is_tensor(flat) else type(flat).__name__
            raise C.OQError(f"{fn}: {flat_name} {what} (expected {want} contiguous bytes: [{layers}, {n}, {page_bytes}])")
        if flat.device != pool.device:
            raise C.OQError(f"{fn}: {flat_name} on {flat.device}, the pool on {pool.device}")
    return out, layers, num_pages, page_bytes, n


def kv_pages_gather(pool, page_ids, dst=None):
    """dst [layers, n, page_bytes] <- pages page_ids of every layer of pool [layers, num_pages, ...] in ONE launch
    (oq_kv_pages_gather, csrc/oq_kvpool.hip).  pool: contiguous (a slice pool[l0:l1] of layers is), any dtype; a page is
    everything behind its first two dimensions, page_bytes a multiple of 16.  page_ids: int32 [n] on the pool's device, never
    read by the host; an id outside [0, num_pages) is skipped and dst keeps its bytes there; ids may repeat.  dst: a contiguous
    tensor of layers * n * page_bytes bytes on that device (None: a fresh uint8 [layers, n, page_bytes]).  Returns dst."""
    (ids,), layers, num_pages, pb, n = _kv_pages_args("kv_pages_gather", pool, (("page_ids", page_ids),), dst,
                                                      None if dst is None else "dst")
    if dst is None:
        dst = torch.empty((layers, n, pb), dtype=torch.uint8, device=pool.device)
    C.call("oq_kv_pages_gather", C.ptr(pool), num_pages, pb, num_pages * pb, layers, C.ptr(ids), n, C.ptr(dst), C.stream())
    return dst


def kv_pages_scatter(src, pool, page_ids):
    """Pages page_ids of every layer of pool <- src [layers, n, page_bytes]: the reverse of kv_pages_gather in one launch
    (oq_kv_pages_scatter).  An id outside [0, num_pages) is skipped and the pool untouched; the valid ids must be distinct."""
    (ids,), layers, num_pages, pb, n = _kv_pages_args("kv_pages_scatter", pool, (("page_ids", page_ids),), src, "src")
    C.call("oq_kv_pages_scatter", C.ptr(src), C.ptr(pool), num_pages, pb, num_pages * pb, layers, C.ptr(ids), n, C.stream())
    return pool


def kv_pages_copy(pool, src_ids, dst_ids):
    """pool[:, dst_ids[i]] <- pool[:, src_ids[i]] for every layer in one launch (oq_kv_pages_copy).  A pair with src == dst, or
    with either id outside [0, num_pages), is skipped.  The valid dst ids must be distinct and none of them another pair's src."""
    (s, d), layers, num_pages, pb, n = _kv_pages_args("kv_pages_copy", pool, (("src_ids", src_ids), ("dst_ids", dst_ids)))
    C.call("oq_kv_pages_copy", C.ptr(pool), num_pages, pb, num_pages * pb, layers, C.ptr(s), C.ptr(d), n, C.stream())
    return pool


def mask_is_causal(attention_mask):
    """True iff the additive attention mask ([T,T] or [bs,1,T,T]) is exactly the causal one: 0 on/below the diagonal
    and <= -3e4 above it -- finfo(float32).min, or finfo(float16).min = -65504 as transformers builds it for the fp16
    model the reference hands to its Catcher (quantize/omniquant.py:89-113); either way exp(masked - row max) is exactly
    0 in float32, so masked probabilities are exactly 0 on both paths.  The check costs one host sync, so its
    result is cached ON the tensor object (or on the base tensor of an expand()/index view) together with the
    tensor's version counter; the causal fast path then skips the masked half of every attention GEMM and of the
    softmax."""
    if attention_mask is None or attention_mask.dim() not in (2, 4) or attention_mask.shape[-1] != attention_mask.shape[-2]:
        return False
    if os.environ.get("OQ_NO_CAUSAL_FASTPATH"):      # A/B switch: always take the dense masked path
        return False
    Tm = attention_mask.shape[-1]
    if Tm >= 256 and Tm % 256 != 0:                  # the causal GEMM modes contract in 256-blocks: dense path instead
        return False
    root = attention_mask._base if attention_mask._base is not None else attention_mask
    # (a view is identified by its window into the base tensor: two slices of one batched mask must not share a verdict)
    tag = (root._version, tuple(attention_mask.shape), tuple(attention_mask.stride()), attention_mask.storage_offset())
    cached = getattr(root, "_oq_causal", None)
    if cached is not None and cached[0] == tag:
        return cached[1]
    T = attention_mask.shape[-1]
    m = attention_mask.reshape(-1, T, T).float()
    lower = torch.tril(torch.ones(T, T, dtype=torch.bool, device=m.device))
    hit = bool(T > 1 and ((m == 0) == lower).all().item() and (m[:, ~lower] <= -3e4).all().item())
    try:
        root._oq_causal = (tag, hit)
    except Exception:
        pass
    return hit


def cast(x, dtype):
    """dtype conversion on the HIP path (RNE)."""
    if x.dtype == dtype:
        return x
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    n = x.numel()
    if n % 8 != 0:
        return x.to(dtype)
    C.call("oq_cast", C.ptr(x), C.dt(x), C.ptr(y), C._DT[dtype], n, C.stream())
    return y


def attention_scale(hd):
    return 1.0 / math.sqrt(hd)
