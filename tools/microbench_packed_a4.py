"""Microbenchmark of the W4A4 real-quant kernels (csrc/oq_packed_a4.hip) on the LLaMA-7B and LLaMA-2-13B projection shapes,
against the W4A16 kernels on the same packed words (4-bit per-channel):
  decode  (M 1 / 4 / 16)      oq_packed_gemv_a4 (int8 codes + per-row vectors in)  vs  oq_packed_gemv (bf16 x in)
  prefill (M 64 / 512 / 2048) oq_packed_codes + oq_gemm_i8                        vs  oq_packed_dequant (bf16) + oq_gemm
and one LLaMA-7B-shape block at bs 1: the decode-step device time (L 2048, from a captured graph) and the T = 2048 prefill
time (no cache), W4A4 against a W4A16 per-channel pack of the same block, in the same process.

Cache state as tools/microbench_packed.py: decode rows rotate through enough distinct weight sets that one round reads more
than the 256 MiB Infinity Cache (every launch streams its weight from HBM); prefill rows rotate through 2 sets.  Every
number is the mean per launch of one captured graph of `reps` rounds, replayed once warm and once under hipEvents.

`--step-only --kv-codes`: instead of N eager steps, the W4A4 block's decode step (bs 1, L 2048) on the bf16 cache and on a
4-bit code cache (PackedKVCache(code_bits=4)), one captured graph each, replayed alternately `--rounds` times: median,
minimum and maximum device time per step of both, and the ratio of the medians.

usage: python tools/microbench_packed_a4.py [--out FILE] [--reps 3] [--quick] [--step-only --steps N [--kv-codes --rounds 7]]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omniquant_amd import _capi as C  # noqa: E402
from omniquant_amd import ops  # noqa: E402

SHAPES = [("7b qkv/o", 4096, 4096), ("7b gate/up", 4096, 11008), ("7b down", 11008, 4096),
          ("13b qkv/o", 5120, 5120), ("13b gate/up", 5120, 13824), ("13b down", 13824, 5120)]
DECODE_MS, PREFILL_MS = [1, 4, 16], [64, 512, 2048]
COLD_BYTES = 320 << 20           # > 256 MiB Infinity Cache
HBM_BPS = 6.3e12


def packed_set(K, N, dev):
    return dict(qw=torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 8, N), dtype=torch.int32, device=dev),
                qz=torch.randint(-2 ** 31, 2 ** 31 - 1, (1, N // 8), dtype=torch.int32, device=dev),
                sc=((torch.rand(1, N, device=dev) + 0.5) * (0.5 / 16)).half())


def act_codes(M, K, dev):
    return ops.IntCodes(torch.randint(0, 16, (M, K), dtype=torch.int8, device=dev), torch.rand(M, device=dev) * 0.1,
                        torch.randint(0, 16, (M,), device=dev).float(), torch.full((M,), 7.5 * K, device=dev), 4)


def timed(fns, reps):
    for f in fns:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            for f in fns:
                f()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / (reps * len(fns))


def kernel_rows(reps, quick, dev):
    rows = []
    for label, K, N in (SHAPES[:1] if quick else SHAPES):
        wbytes = K * N // 2 + N * 3
        nsets = max(2, -(-COLD_BYTES // wbytes))
        sets = [packed_set(K, N, dev) for _ in range(nsets)]
        for M in DECODE_MS:
            xi = act_codes(M, K, dev)
            xb = (torch.randn(M, K, device=dev) * 0.5).bfloat16()
            y32 = torch.empty(M, N, device=dev)
            yb = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            ws_a = torch.empty(max(16, C.size_call("oq_packed_gemv_a4_workspace", M, K, N)), dtype=torch.uint8, device=dev)
            ws_b = torch.empty(max(16, C.size_call("oq_packed_gemv_workspace", M, K, N, 4)), dtype=torch.uint8, device=dev)

            def a4(s):
                return lambda: C.call("oq_packed_gemv_a4", C.ptr(xi.codes), C.fptr(xi.scale), C.fptr(xi.zp), C.fptr(xi.csum), M, K, N,
                                      C.ptr(s["qw"]), C.ptr(s["qz"]), C.ptr(s["sc"]), None, None, 0, C.ptr(y32), C.dt(y32),
                                      C.ptr(ws_a), ws_a.numel(), C.stream())

            def a16(s):
                return lambda: C.call("oq_packed_gemv", C.ptr(xb), C.dt(xb), M, K, N, K, 4, C.ptr(s["qw"]), C.ptr(s["qz"]),
                                      C.ptr(s["sc"]), None, None, C.ptr(yb), C.ptr(ws_b), ws_b.numel(), C.stream())
            for name, mk in (("gemv_a4", a4), ("gemv_w4a16", a16)):
                us = timed([mk(s) for s in sets], reps)
                r = dict(shape=label, K=K, N=N, M=M, kernel=name, us=round(us, 2), weight_GBps=round(wbytes / us / 1e3, 1),
                         frac_hbm=round(wbytes / (us * 1e-6) / HBM_BPS, 3), cache="cold")
                print(json.dumps(r), flush=True)
                rows.append(r)
        two = sets[:2]
        del sets
        for M in PREFILL_MS:
            xi = act_codes(M, K, dev)
            xb = (torch.randn(M, K, device=dev) * 0.5).bfloat16()
            y32 = torch.empty(M, N, device=dev)
            yb = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            wc = torch.empty(N, K, dtype=torch.int8, device=dev)
            vec = torch.empty(3, N, device=dev)
            wd = torch.empty(N, K, dtype=torch.bfloat16, device=dev)

            def a4p(s):
                def f():
                    C.call("oq_packed_codes", C.ptr(s["qw"]), C.ptr(s["qz"]), C.ptr(s["sc"]), K, N, C.ptr(wc), C.fptr(vec[0]),
                           C.fptr(vec[1]), C.fptr(vec[2]), C.stream())
                    ops.gemm_i8(xi, ops.IntCodes(wc, vec[0], vec[1], vec[2], 4), yb)
                return f

            def a16p(s):
                def f():
                    C.call("oq_packed_dequant", C.ptr(s["qw"]), C.ptr(s["qz"]), C.ptr(s["sc"]), K, N, K, 4, C.ptr(wd), C.dt(wd),
                           C.stream())
                    ops.gemm(xb, wd, yb, M, N, K, K, K, N, True, True)
                return f

            def codes_only(s):
                return lambda: C.call("oq_packed_codes", C.ptr(s["qw"]), C.ptr(s["qz"]), C.ptr(s["sc"]), K, N, C.ptr(wc),
                                      C.fptr(vec[0]), C.fptr(vec[1]), C.fptr(vec[2]), C.stream())
            for name, mk in (("a4_codes+gemm_i8", a4p), ("w4a16_dequant+gemm", a16p), ("a4_codes_only", codes_only)):
                us = timed([mk(s) for s in two], reps)
                r = dict(shape=label, K=K, N=N, M=M, kernel=name, us=round(us, 2), TOPs=round(2.0 * M * N * K / us / 1e6, 1),
                         cache="warm")
                print(json.dumps(r), flush=True)
                rows.append(r)
    return rows


def packed_7b_block(dev, act_quant):
    """A LLaMA-7B block with random 4-bit per-channel AutoGPTQ buffers (the costs do not depend on their values); act_quant:
    the W4A4 integer path (4-bit activation quantisers, act_bits 4 linears), else the W4A16 weight-only path."""
    from omniquant_amd.calibrate import decoder_layer_class, default_args
    from omniquant_amd.linear import QuantLinear
    from omniquant_amd.realquant import PackedLinear, _mark_packed
    from omniquant_amd.synthetic import make_config, make_layer
    cfg = make_config("llama-7b")
    args = default_args(wbits=4, abits=4 if act_quant else 16, group_size=None, lwc=True, let=False, epochs=0, nsamples=1,
                        net="llama-7b")
    blk = decoder_layer_class("llama")(cfg, make_layer(cfg, device=dev, outliers=False), args).to(dev)
    for name, m in list(blk.named_modules()):
        if isinstance(m, QuantLinear):
            inn, out = m.in_features, m.out_features
            s = packed_set(inn, out, dev)
            p = dict(qweight=s["qw"], qzeros=s["qz"], scales=s["sc"], g_idx=torch.zeros(inn, dtype=torch.int32, device=dev), bias=None)
            parent = blk
            parts = name.split(".")
            for p_ in parts[:-1]:
                parent = getattr(parent, p_)
            setattr(parent, parts[-1], PackedLinear(4, inn, inn, out, p, act_bits=4 if act_quant else 16))
    _mark_packed(blk, 4 if act_quant else 16, act_quant)
    blk.compute_dtype = torch.bfloat16
    return blk, cfg


def block_rows(dev, reps, steps_only=0):
    from omniquant_amd.kvcache import PackedKVCache
    from omniquant_amd.synthetic import causal_mask
    L = 2048
    rows = []
    for act_quant in ((True,) if steps_only else (True, False)):
        blk, cfg = packed_7b_block(dev, act_quant)
        H, nh = cfg.hidden_size, cfg.num_attention_heads
        cache = PackedKVCache(1, nh, H // nh, torch.bfloat16, dev, capacity=L + 64)
        cache.k.normal_()
        cache.v.normal_()
        x = (torch.randn(1, 1, H, device=dev) * 0.5).bfloat16()
        pos = torch.tensor([[L - 1]], device=dev)

        def step():
            cache.length = L - 1
            with torch.no_grad():
                return blk(x, attention_mask=None, position_ids=pos, past_key_value=cache, use_cache=True)[0]
        step()
        torch.cuda.synchronize()
        if steps_only:
            for _ in range(steps_only):
                step()
            torch.cuda.synchronize()
            return rows
        calls = []
        orig = C.call
        C.call = lambda name, *a: calls.append(name) or orig(name, *a)
        try:
            step()
        finally:
            C.call = orig
        step_us = timed([step], reps * 10)
        xp = (torch.randn(1, L, H, device=dev) * 0.5).bfloat16()
        mask = causal_mask(L).to(dev)
        posp = torch.arange(L, device=dev)[None]

        def prefill():
            with torch.no_grad():
                return blk(xp, attention_mask=mask, position_ids=posp)[0]
        prefill()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            prefill()
        b.record()
        torch.cuda.synchronize()
        r = dict(what=f"packed llama-7b {'W4A4' if act_quant else 'W4A16'} per-channel block", bs=1, L=L, dtype="bfloat16",
                 decode_graph_device_us_per_step=round(step_us, 2), capi_calls_per_step=len(calls),
                 prefill_T2048_eager_us=round(a.elapsed_time(b) * 1000.0 / reps, 1))
        print(json.dumps(r), flush=True)
        rows.append(r)
        del blk, cache
        torch.cuda.empty_cache()
    return rows


def step_kv_codes(dev, reps, rounds):
    """The W4A4 7B block's decode step on the bf16 cache and on the code cache, interleaved."""
    from omniquant_amd.kvcache import PackedKVCache
    L = 2048
    blk, cfg = packed_7b_block(dev, True)
    H, nh = cfg.hidden_size, cfg.num_attention_heads
    x = (torch.randn(1, 1, H, device=dev) * 0.5).bfloat16()
    pos = torch.tensor([[L - 1]], device=dev)
    caches = [PackedKVCache(1, nh, H // nh, torch.bfloat16, dev, capacity=L + 64),
              PackedKVCache(1, nh, H // nh, torch.bfloat16, dev, capacity=L + 64, code_bits=4)]
    caches[0].k.normal_()
    caches[0].v.normal_()
    for codes, meta in ((caches[1].k_codes, caches[1].k_meta), (caches[1].v_codes, caches[1].v_meta)):
        codes.copy_(torch.randint(0, 256, codes.shape, dtype=torch.uint8, device=dev))
        meta[..., 0] = 0.35
        meta[..., 1] = 8.0
    graphs, calls = [], []
    for cache in caches:
        def step(cache=cache):
            cache.length = L - 1
            with torch.no_grad():
                return blk(x, attention_mask=None, position_ids=pos, past_key_value=cache, use_cache=True)[0]
        names = []
        orig = C.call
        C.call = lambda name, *a: names.append(name) or orig(name, *a)
        try:
            step()
        finally:
            C.call = orig
        calls.append(sorted(set(names)))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps * 10):
                step()
        g.replay()
        torch.cuda.synchronize()
        graphs.append(g)
    us = ([], [])
    for _ in range(rounds):
        for i, g in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            us[i].append(a.elapsed_time(b) * 1000.0 / (reps * 10))
    med = [sorted(u)[len(u) // 2] for u in us]
    r = dict(what="packed llama-7b W4A4 per-channel block decode step, bf16 cache vs 4-bit code cache", bs=1, L=L,
             dtype="bfloat16", rounds=rounds, bf16_cache_us=round(med[0], 2), bf16_cache_us_min=round(min(us[0]), 2),
             bf16_cache_us_max=round(max(us[0]), 2), code_cache_us=round(med[1], 2), code_cache_us_min=round(min(us[1]), 2),
             code_cache_us_max=round(max(us[1]), 2), code_over_bf16=round(med[1] / med[0], 4),
             cache_bytes=[c.nbytes() for c in caches], code_cache_capi_calls=calls[1])
    print(json.dumps(r), flush=True)
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--step-only", action="store_true", help="only N eager W4A4 decode steps of the 7B block (for rocprofv3)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--kv-codes", action="store_true", help="with --step-only: the step on the bf16 cache vs the 4-bit code cache")
    ap.add_argument("--rounds", type=int, default=7, help="--kv-codes: alternating replays of the two graphs")
    a = ap.parse_args()
    dev = "cuda:0"
    if not torch.cuda.is_available():
        raise SystemExit("microbench_packed_a4 needs a GPU")
    C.load()
    if a.kv_codes and not a.step_only:
        ap.error("--kv-codes goes with --step-only")
    if a.step_only and a.kv_codes:
        rows = step_kv_codes(dev, a.reps, a.rounds)
    elif a.step_only:
        block_rows(dev, a.reps, steps_only=a.steps)
        return
    else:
        rows = kernel_rows(a.reps, a.quick, dev) + block_rows(dev, a.reps)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
