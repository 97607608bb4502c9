"""Microbenchmark of the incremental-decoding kernels (csrc/oq_decode.hip) and of one packed LLaMA-7B decode step.

1. oq_attn_decode (bf16, Tq = 1) at the LLaMA-7B shape (32 / 32 heads of 128) and the LLaMA-2-70B GQA shape (64 / 8), bs 1
   and 8, L = 512 ... 32768.  Cold caches: each shape rotates through enough distinct K/V caches that one round reads more
   than the 256 MiB Infinity Cache.  Time per launch from one captured graph of `reps` rounds, replayed under hipEvents.
   GB/s counts the algorithmic bytes (2 * bs * nkv * L * hd * 2 of K and V; no mask), "frac" is that over the 6.3 TB/s
   achievable HBM rate (MI355X_MICROARCH.md).  Baseline: what the block would otherwise need -- a [bs, L, nkv, hd] copy of
   the cache, then AttnScoresFn -> SoftmaxFn -> AttnPVFn (oq_gemm + oq_softmax_fwd; the softmax kernel covers L <= 4096).
2. One packed LLaMA-7B W4A16g128 block decode step (bs 1, L 2048, bf16): device time per step from a captured graph, the
   eager host time per forward call, and the HIP launches of the step (C-ABI calls counted on the host).
   `--step-only --steps N` runs N eager steps and nothing else (for a `rocprofv3 --kernel-trace --stats` run of its own).

3. `--codes`: instead of 1 and 2, oq_attn_decode_codes on a 4-bit code cache (72 bytes per head row of 128) against
   oq_attn_decode on the bf16 cache, same shape table, same process, both on cold cache sets (the code cache rotates through
   more sets: each is smaller).  The two graphs are replayed alternately `--rounds` times; a row reports the median, minimum
   and maximum of each kernel, the bf16 kernel's own run-to-run spread (max - min over its median) and the ratio of the
   medians.

   `--codes8`: the `--codes` run with oq_attn_decode_codes8 on an 8-bit code cache (136 bytes per head row of 128) as a third
   interleaved contestant, at the 7B shape, bs 8, L 8192 and 32768.  A row adds the 8-bit kernel's median / min / max, its
   ratio to the bf16 kernel of the same run and `codes8_faster_beyond_spread`: whether its median beats the bf16 kernel's by
   more than the bf16 kernel's own run-to-run spread.

4. `--ragged`: instead of 1 and 2, a batch of 8 sequences of lengths 128 ... 8192 (geometric) at the 7B shape, Tq = 1, on a
   bf16 cache and on a 4-bit code cache: oq_attn_decode_ragged / oq_attn_decode_codes_ragged (per-sequence lengths on the
   device, bound 8192, no mask) against oq_attn_decode / oq_attn_decode_codes on the same batch left-padded to 8192 with a
   transformers-style fp16 mask.  Same buffers, same process, cold cache sets (one round over the sets reads more than the
   Infinity Cache even for the ragged kernel, which reads the fewest bytes); the four graphs are replayed alternately
   `--rounds` times.  A row reports median / min / max per kernel, the bytes each must read, the run-to-run spread (max -
   min over the median) of both bf16 kernels and the ratios of the medians.

5. `--paged`: instead of 1 and 2, paged against ragged contiguous storage at the same lengths: a batch of 8 sequences of
   mixed lengths (geometric, L / 64 ... L) at the 7B shape, Tq = 1, bounds L = 8192 and 32768, on a bf16 cache and on a 4-bit
   code cache.  oq_attn_decode_paged / oq_attn_decode_codes_paged with page sizes 16 and 128, on pools that hold exactly the
   pages the lengths need, in a random page order, against oq_attn_decode_ragged / oq_attn_decode_codes_ragged on
   [bs, nkv, L, hd] slabs.  Cold cache sets, the three graphs of a row replayed alternately `--rounds` times; a row reports
   median / min / max per kernel, the contiguous kernel's run-to-run spread (max - min over its median) and the ratios of
   the medians.  Then the three appends' paged forms next to their ragged forms at Tq = 1 (bound 8192).

6. `--extend`: instead of 1 and 2, the MFMA chunked-prefill kernel (csrc/oq_extend.hip, oq_attn_extend*) against the ragged
   decode kernel on the same inputs: one sequence with a past of 2048 and of 8192 rows, Tq = 16, 64, 256 and 1024 query
   rows, at the 7B (32 / 32) and the 70B GQA (64 / 8) shape, on a bf16 slab, on bf16 pools of 16-row pages in a random page
   order and on a 4-bit code slab.  The six graphs of a row (decode and extend per storage, the same cold cache sets for
   both) are replayed alternately `--rounds` times; a row reports median / min / max per kernel, each decode kernel's
   run-to-run spread (max - min over its median) and extend over decode.  `slower_beyond_spread` names the storage kinds
   where the new kernel's median exceeds the decode kernel's by more than that spread: block_common.EXTEND_MIN_TQ must lie
   above every Tq that has one.  FLOPs are not reported here: a share of the MFMA peak wants a counter run of its own.

usage: python tools/microbench_decode.py [--out FILE] [--reps 3] [--quick] [--step-only --steps N]
                                         [--codes | --codes8 | --ragged | --paged | --extend [--rounds 7]]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omniquant_amd import _capi as C  # noqa: E402
from omniquant_amd import ops  # noqa: E402

SHAPES = [("7b", 32, 32, 128), ("70b gqa", 64, 8, 128)]
BS = [1, 8]
LS = [512, 2048, 8192, 32768]
COLD_BYTES = 320 << 20           # > 256 MiB Infinity Cache
HBM_BPS = 6.3e12


def timed(fns, reps):
    """Mean time per launch of `reps` rounds over fns, replayed from one captured graph."""
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


def interleaved(launch_lists, reps, rounds):
    """Time several kernels against each other in one process: each list of launches (one per cold cache set) is warmed up and
    captured as one graph of `reps` rounds, then the graphs are replayed alternately `rounds` times under hipEvents.  Returns
    (per-launch microseconds of every replay, per list; their medians)."""
    graphs = []
    for fns in launch_lists:
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
        graphs.append((g, reps * len(fns)))
    us = [[] for _ in graphs]
    for _ in range(rounds):
        for i, (g, n) in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            us[i].append(a.elapsed_time(b) * 1000.0 / n)
    return us, [sorted(u)[len(u) // 2] for u in us]


def kernel_rows(reps, quick, dev):
    rows = []
    for name, nh, nkv, hd in SHAPES:
        for bs in BS:
            for L in LS:
                if quick and (bs != 1 or L not in (2048, 8192)):
                    continue
                kv_bytes = 2 * bs * nkv * L * hd * 2
                nsets = max(2, -(-COLD_BYTES // kv_bytes))
                sets = [(torch.randn(bs, nkv, L, hd, device=dev).bfloat16(), torch.randn(bs, nkv, L, hd, device=dev).bfloat16())
                        for _ in range(nsets)]
                q = torch.randn(bs, 1, nh, hd, device=dev).bfloat16()
                o = torch.empty_like(q)
                ws_n = C.size_call("oq_attn_decode_workspace", bs, nh, nkv, 1, L, hd)
                ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
                scale = hd ** -0.5
                r = dict(shape=name, nh=nh, nkv=nkv, hd=hd, bs=bs, L=L, Tq=1, dtype="bfloat16", cache="cold", sets=nsets)

                def dec(s):
                    return lambda: ops.decode_attention(q, s[0], s[1], L, scale, out=o, workspace=ws)

                r["decode_us"] = timed([dec(s) for s in sets], reps)
                r["decode_GBps"] = kv_bytes / r["decode_us"] / 1e3
                r["decode_frac_hbm"] = r["decode_GBps"] * 1e9 / HBM_BPS
                if L <= 4096:
                    def base(s):
                        def f():
                            k = s[0].transpose(1, 2).contiguous()          # [bs, L, nkv, hd]: the layout the GEMMs read
                            v = s[1].transpose(1, 2).contiguous()
                            p = ops.SoftmaxFn.apply(ops.AttnScoresFn.apply(q, k, False), None, scale, False)
                            ops.AttnPVFn.apply(p, v, False)
                        return f

                    with torch.no_grad():
                        r["baseline_us"] = timed([base(s) for s in sets], reps)
                    r["speedup"] = r["baseline_us"] / r["decode_us"]
                rows.append(r)
                print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
                del sets
                torch.cuda.empty_cache()
    return rows


def codes_rows(reps, rounds, quick, dev, codes8=False):
    rows = []
    for name, nh, nkv, hd in SHAPES:
        for bs in BS:
            for L in LS:
                if quick and (bs != 1 or L not in (2048, 8192)):
                    continue
                if codes8 and (name != "7b" or bs != 8 or L not in (8192, 32768)):
                    continue
                kv_bytes = 2 * bs * nkv * L * hd * 2
                code_bytes = 2 * bs * nkv * L * (hd // 2 + 8)
                q = torch.randn(bs, 1, nh, hd, device=dev).bfloat16()
                o = torch.empty_like(q)
                ws = torch.empty(C.size_call("oq_attn_decode_workspace", bs, nh, nkv, 1, L, hd), dtype=torch.uint8, device=dev)
                scale = hd ** -0.5
                fsets = [(torch.randn(bs, nkv, L, hd, device=dev).bfloat16(), torch.randn(bs, nkv, L, hd, device=dev).bfloat16())
                         for _ in range(max(2, -(-COLD_BYTES // kv_bytes)))]

                def meta():      # scales and integer zero-points of the size a 4-bit grid over N(0, 1) rows has
                    m = torch.empty(bs, nkv, L, 2, device=dev)
                    m[..., 0] = torch.rand(bs, nkv, L, device=dev) * 0.1 + 0.3
                    m[..., 1] = torch.randint(5, 11, (bs, nkv, L), device=dev).float()
                    return m

                csets = [(torch.randint(0, 256, (bs, nkv, L, hd // 2), dtype=torch.uint8, device=dev),
                          torch.randint(0, 256, (bs, nkv, L, hd // 2), dtype=torch.uint8, device=dev), meta(), meta())
                         for _ in range(max(2, -(-COLD_BYTES // code_bytes)))]
                lists = [[(lambda s=s: ops.decode_attention(q, s[0], s[1], L, scale, out=o, workspace=ws)) for s in fsets],
                         [(lambda s=s: ops.decode_attention_codes(q, s, L, scale, out=o, workspace=ws)) for s in csets]]
                if codes8:
                    code8_bytes = 2 * bs * nkv * L * (hd + 8)

                    def meta8():     # scales and zero-points of a 255-level grid whose range contains zero
                        m = torch.empty(bs, nkv, L, 2, device=dev)
                        m[..., 0] = torch.rand(bs, nkv, L, device=dev) * 0.01 + 0.02
                        m[..., 1] = torch.randint(96, 160, (bs, nkv, L), device=dev).float()
                        return m

                    c8sets = [(torch.randint(0, 256, (bs, nkv, L, hd), dtype=torch.uint8, device=dev),
                               torch.randint(0, 256, (bs, nkv, L, hd), dtype=torch.uint8, device=dev), meta8(), meta8())
                              for _ in range(max(2, -(-COLD_BYTES // code8_bytes)))]
                    lists.append([(lambda s=s: ops.decode_attention_codes(q, s, L, scale, out=o, workspace=ws)) for s in c8sets])
                us, med = interleaved(lists, reps, rounds)
                r = dict(shape=name, nh=nh, nkv=nkv, hd=hd, bs=bs, L=L, Tq=1, dtype="bfloat16", cache="cold", rounds=rounds,
                         bf16_sets=len(fsets), code_sets=len(csets),
                         bf16_us=med[0], bf16_us_min=min(us[0]), bf16_us_max=max(us[0]),
                         bf16_spread=(max(us[0]) - min(us[0])) / med[0],
                         codes_us=med[1], codes_us_min=min(us[1]), codes_us_max=max(us[1]),
                         codes_spread=(max(us[1]) - min(us[1])) / med[1],
                         codes_over_bf16=med[1] / med[0], bf16_GBps=kv_bytes / med[0] / 1e3, codes_GBps=code_bytes / med[1] / 1e3,
                         codes_frac_hbm=code_bytes / med[1] * 1e6 / HBM_BPS)
                if codes8:
                    r.update(code8_sets=len(c8sets), codes8_us=med[2], codes8_us_min=min(us[2]), codes8_us_max=max(us[2]),
                             codes8_spread=(max(us[2]) - min(us[2])) / med[2], codes8_over_bf16=med[2] / med[0],
                             codes8_GBps=code8_bytes / med[2] / 1e3, codes8_frac_hbm=code8_bytes / med[2] * 1e6 / HBM_BPS,
                             codes8_faster_beyond_spread=bool(med[0] - med[2] > max(us[0]) - min(us[0])))
                    del c8sets
                rows.append(r)
                print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
                del fsets, csets
                torch.cuda.empty_cache()
    return rows


RAGGED_LENGTHS = [128, 232, 420, 760, 1378, 2496, 4522, 8192]      # a batch of 8, geometric from 128 to 8192


def ragged_bytes(lengths, nkv, hd):
    """Bytes of K and V each kernel must read for one step of the batch: (bf16 ragged, bf16 padded, codes ragged, codes
    padded).  The padded kernels stream every sequence at the longest length, and their fp16 mask on top."""
    bs, Lmax, rows = len(lengths), max(lengths), sum(lengths)
    mask = bs * Lmax * 2
    return (2 * nkv * rows * hd * 2, 2 * nkv * bs * Lmax * hd * 2 + mask,
            2 * nkv * rows * (hd // 2 + 8), 2 * nkv * bs * Lmax * (hd // 2 + 8) + mask)


def ragged_rows(reps, rounds, dev):
    name, nh, nkv, hd = SHAPES[0]
    lengths = RAGGED_LENGTHS
    bs, L = len(lengths), max(lengths)
    need = ragged_bytes(lengths, nkv, hd)
    scale = hd ** -0.5
    q = torch.randn(bs, 1, nh, hd, device=dev).bfloat16()
    o = torch.empty_like(q)
    ws = torch.empty(C.size_call("oq_attn_decode_workspace", bs, nh, nkv, 1, L, hd), dtype=torch.uint8, device=dev)
    lens = torch.tensor([n - 1 for n in lengths], dtype=torch.int32, device=dev)      # the rows before this step's append
    # the padded form of the batch: sequence b occupies the LAST lengths[b] rows, the mask hides the pad rows in front
    mask = torch.zeros(bs, 1, 1, L, dtype=torch.float16, device=dev)
    for b, n in enumerate(lengths):
        mask[b, 0, 0, :L - n] = torch.finfo(torch.float16).min
    fsets = [(torch.randn(bs, nkv, L, hd, device=dev).bfloat16(), torch.randn(bs, nkv, L, hd, device=dev).bfloat16())
             for _ in range(max(2, -(-COLD_BYTES // need[0])))]

    def meta():
        m = torch.empty(bs, nkv, L, 2, device=dev)
        m[..., 0] = torch.rand(bs, nkv, L, device=dev) * 0.1 + 0.3
        m[..., 1] = torch.randint(5, 11, (bs, nkv, L), device=dev).float()
        return m

    csets = [(torch.randint(0, 256, (bs, nkv, L, hd // 2), dtype=torch.uint8, device=dev),
              torch.randint(0, 256, (bs, nkv, L, hd // 2), dtype=torch.uint8, device=dev), meta(), meta())
             for _ in range(max(2, -(-COLD_BYTES // need[2])))]
    kinds = ("bf16_ragged", "bf16_padded", "codes_ragged", "codes_padded")
    launches = ([(lambda s=s: ops.decode_attention(q, s[0], s[1], L, scale, out=o, workspace=ws, lengths=lens)) for s in fsets],
                [(lambda s=s: ops.decode_attention(q, s[0], s[1], L, scale, mask, out=o, workspace=ws)) for s in fsets],
                [(lambda s=s: ops.decode_attention_codes(q, s, L, scale, out=o, workspace=ws, lengths=lens)) for s in csets],
                [(lambda s=s: ops.decode_attention_codes(q, s, L, scale, mask, out=o, workspace=ws)) for s in csets])
    us, med = interleaved(launches, reps, rounds)
    r = dict(shape=name, nh=nh, nkv=nkv, hd=hd, bs=bs, lengths=lengths, L_bound=L, Tq=1, dtype="bfloat16", cache="cold",
             rounds=rounds, bf16_sets=len(fsets), code_sets=len(csets))
    for i, k in enumerate(kinds):
        r.update({k + "_us": med[i], k + "_us_min": min(us[i]), k + "_us_max": max(us[i]), k + "_bytes": need[i],
                  k + "_GBps": need[i] / med[i] / 1e3})
    r.update(bf16_ragged_spread=(max(us[0]) - min(us[0])) / med[0], bf16_padded_spread=(max(us[1]) - min(us[1])) / med[1],
             bf16_ragged_over_padded=med[0] / med[1],
             codes_ragged_over_padded=med[2] / med[3], bf16_bytes_ragged_over_padded=need[0] / need[1],
             codes_bytes_ragged_over_padded=need[2] / need[3])
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return [r]


def paged_rows(reps, rounds, quick, dev):
    name, nh, nkv, hd = SHAPES[0]
    bs, scale = 8, hd ** -0.5
    rows = []
    q = torch.randn(bs, 1, nh, hd, device=dev).bfloat16()
    o = torch.empty_like(q)

    def tensors(kind, lead):
        """K and V of a cache kind with leading dims `lead` + (rows,): (k, v) bf16, or (k_codes, v_codes, k_meta, v_meta)."""
        if kind == "bf16":
            return tuple(torch.randn(*lead, hd, device=dev).bfloat16() for _ in range(2))
        out = [torch.randint(0, 256, (*lead, hd // 2), dtype=torch.uint8, device=dev) for _ in range(2)]
        for _ in range(2):
            m = torch.empty(*lead, 2, device=dev)
            m[..., 0] = torch.rand(*lead, device=dev) * 0.1 + 0.3
            m[..., 1] = torch.randint(5, 11, tuple(lead), device=dev).float()
            out.append(m)
        return tuple(out)

    def attend(kind, s, L, lens, table=None):
        if kind == "bf16":
            return lambda: ops.decode_attention(q, s[0], s[1], L, scale, out=o, workspace=ws, lengths=lens, page_table=table)
        return lambda: ops.decode_attention_codes(q, s, L, scale, out=o, workspace=ws, lengths=lens, page_table=table)

    def table_of(lengths, ps, L, seed):
        """A pool of exactly the pages the lengths need, handed out in a random order; unused entries -1."""
        need = [-(-n // ps) for n in lengths]
        perm = torch.randperm(sum(need), generator=torch.Generator().manual_seed(seed)).tolist()
        t = torch.full((bs, L // ps), -1, dtype=torch.int32)
        at = 0
        for b, n in enumerate(need):
            t[b, :n] = torch.tensor(perm[at:at + n], dtype=torch.int32)
            at += n
        return t.to(dev), sum(need)

    for L in ((8192,) if quick else (8192, 32768)):
        lengths = [n * (L // 8192) for n in RAGGED_LENGTHS]
        lens = torch.tensor([n - 1 for n in lengths], dtype=torch.int32, device=dev)
        ws = torch.empty(C.size_call("oq_attn_decode_workspace", bs, nh, nkv, 1, L, hd), dtype=torch.uint8, device=dev)
        for kind, row_bytes in (("bf16", 2 * hd), ("codes", hd // 2 + 8)):
            need = 2 * nkv * sum(lengths) * row_bytes
            nsets = max(2, -(-COLD_BYTES // need))
            launches = [[attend(kind, tensors(kind, (bs, nkv, L)), L, lens) for _ in range(nsets)]]
            pools = {}
            for ps in (16, 128):
                fns = []
                for i in range(nsets):
                    table, num_pages = table_of(lengths, ps, L, 100 * ps + i)
                    fns.append(attend(kind, tensors(kind, (num_pages, nkv, ps)), L, lens, table))
                pools[ps] = num_pages
                launches.append(fns)
            us, med = interleaved(launches, reps, rounds)
            r = dict(what="attention", shape=name, nh=nh, nkv=nkv, hd=hd, bs=bs, lengths=lengths, L_bound=L, Tq=1, cache=kind,
                     sets=nsets, rounds=rounds, bytes=need, slab_rows=bs * L, pool_rows_ps16=pools[16] * 16,
                     pool_rows_ps128=pools[128] * 128)
            for i, k in enumerate(("contiguous", "paged16", "paged128")):
                r.update({k + "_us": med[i], k + "_us_min": min(us[i]), k + "_us_max": max(us[i]), k + "_GBps": need / med[i] / 1e3})
            r.update(contiguous_spread=(max(us[0]) - min(us[0])) / med[0], paged16_over_contiguous=med[1] / med[0],
                     paged128_over_contiguous=med[2] / med[0])
            rows.append(r)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
            del launches, fns
            torch.cuda.empty_cache()
    # the appends at Tq = 1 (bound 8192): one row per sequence and kv head, the launch dominates
    L = 8192
    lengths = RAGGED_LENGTHS
    lens = torch.tensor([n - 1 for n in lengths], dtype=torch.int32, device=dev)
    cos, sin = torch.randn(L, hd, device=dev), torch.randn(L, hd, device=dev)
    k32, v32 = (torch.randn(bs, 1, nkv, hd, device=dev) for _ in range(2))
    q32 = torch.randn(bs, 1, nh, hd, device=dev)
    qo = torch.empty_like(q)
    ko, vo = (torch.empty(bs, 1, nkv, hd, dtype=torch.bfloat16, device=dev) for _ in range(2))
    kb, vb = k32.bfloat16(), v32.bfloat16()
    for kind in ("plain", "quant", "codes"):
        def append(bufs, table=None, kind=kind):
            kw = dict(q_out=qo, cos=cos, sin=sin, lengths=lens, page_table=table)
            if kind == "plain":
                return lambda: ops.kv_append(kb, vb, bufs[0], bufs[1], 0, q=q, **kw)
            if kind == "quant":
                return lambda: ops.kv_append_quant(k32, v32, 4, torch.bfloat16, k_cache=bufs[0], v_cache=bufs[1], q=q32, k_out=ko,
                                                   v_out=vo, **kw)
            return lambda: ops.kv_append_codes(k32, v32, torch.bfloat16, *bufs, q=q32, k_out=ko, v_out=vo, **kw)

        store = "codes" if kind == "codes" else "bf16"
        launches = [[append(tensors(store, (bs, nkv, L)))]]
        for ps in (16, 128):
            table, num_pages = table_of(lengths, ps, L, ps)
            launches.append([append(tensors(store, (num_pages, nkv, ps)), table)])
        us, med = interleaved(launches, reps * 10, rounds)
        r = dict(what="append " + kind, shape=name, nh=nh, nkv=nkv, hd=hd, bs=bs, Tq=1, L_bound=L, rounds=rounds)
        for i, k in enumerate(("contiguous", "paged16", "paged128")):
            r.update({k + "_us": med[i], k + "_us_min": min(us[i]), k + "_us_max": max(us[i])})
        r.update(contiguous_spread=(max(us[0]) - min(us[0])) / med[0], paged16_over_contiguous=med[1] / med[0],
                 paged128_over_contiguous=med[2] / med[0])
        rows.append(r)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return rows


EXTEND_TQ = [16, 64, 256, 1024]
EXTEND_PAST = [2048, 8192]


def extend_rows(reps, rounds, quick, dev):
    rows = []
    bs, ps = 1, 16
    for name, nh, nkv, hd in SHAPES:
        scale = hd ** -0.5
        for past in EXTEND_PAST:
            for Tq in EXTEND_TQ:
                if quick and (past != 2048 or Tq not in (16, 256)):
                    continue
                L = past + Tq
                lens = torch.tensor([past], dtype=torch.int32, device=dev)
                q = torch.randn(bs, Tq, nh, hd, device=dev).bfloat16()
                o = torch.empty_like(q)
                ws = torch.empty(max(C.size_call("oq_attn_decode_workspace", bs, nh, nkv, Tq, L, hd),
                                     C.size_call("oq_attn_extend_workspace", bs, nh, nkv, Tq, L, hd), 16), dtype=torch.uint8, device=dev)
                kv_bytes, code_bytes = 2 * nkv * L * hd * 2, 2 * nkv * L * (hd // 2 + 8)
                nsets = max(2, -(-COLD_BYTES // kv_bytes))
                mp = -(-L // ps)

                def meta(lead):
                    m = torch.empty(*lead, 2, device=dev)
                    m[..., 0] = torch.rand(*lead, device=dev) * 0.1 + 0.3
                    m[..., 1] = torch.randint(5, 11, tuple(lead), device=dev).float()
                    return m

                slabs = [tuple(torch.randn(bs, nkv, L, hd, device=dev).bfloat16() for _ in range(2)) for _ in range(nsets)]
                pools = [tuple(torch.randn(mp, nkv, ps, hd, device=dev).bfloat16() for _ in range(2)) for _ in range(nsets)]
                tables = [torch.randperm(mp, generator=torch.Generator().manual_seed(i)).to(torch.int32)[None].to(dev)
                          for i in range(nsets)]
                codes = [tuple(torch.randint(0, 256, (bs, nkv, L, hd // 2), dtype=torch.uint8, device=dev) for _ in range(2))
                         + (meta((bs, nkv, L)), meta((bs, nkv, L))) for _ in range(max(2, -(-COLD_BYTES // code_bytes)))]
                kw = dict(out=o, workspace=ws)
                launches = (
                    [(lambda s=s: ops.decode_attention(q, s[0], s[1], L, scale, lengths=lens, **kw)) for s in slabs],
                    [(lambda s=s: ops.extend_attention(q, s[0], s[1], L, scale, lens, **kw)) for s in slabs],
                    [(lambda s=s, t=t: ops.decode_attention(q, s[0], s[1], L, scale, lengths=lens, page_table=t, **kw))
                     for s, t in zip(pools, tables)],
                    [(lambda s=s, t=t: ops.extend_attention(q, s[0], s[1], L, scale, lens, page_table=t, **kw))
                     for s, t in zip(pools, tables)],
                    [(lambda s=s: ops.decode_attention_codes(q, s, L, scale, lengths=lens, **kw)) for s in codes],
                    [(lambda s=s: ops.extend_attention_codes(q, s, L, scale, lens, **kw)) for s in codes])
                us, med = interleaved(launches, reps, rounds)
                r = dict(shape=name, nh=nh, nkv=nkv, hd=hd, bs=bs, past=past, Tq=Tq, L_bound=L, dtype="bfloat16", cache="cold",
                         rounds=rounds, sets=nsets, code_sets=len(codes), kv_bytes=kv_bytes, code_bytes=code_bytes)
                slower = []
                for i, k in enumerate(("slab", "paged16", "codes")):
                    d, e = 2 * i, 2 * i + 1
                    spread = (max(us[d]) - min(us[d])) / med[d]
                    r.update({k + "_decode_us": med[d], k + "_decode_us_min": min(us[d]), k + "_decode_us_max": max(us[d]),
                              k + "_decode_spread": spread, k + "_extend_us": med[e], k + "_extend_us_min": min(us[e]),
                              k + "_extend_us_max": max(us[e]), k + "_extend_over_decode": med[e] / med[d]})
                    if med[e] > med[d] * (1.0 + spread):
                        slower.append(k)
                r["slower_beyond_spread"] = slower
                rows.append(r)
                print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
                del launches, slabs, pools, codes
                torch.cuda.empty_cache()
    return rows


def packed_7b_block(dev, L_cap):
    """A LLaMA-7B block with random W4 g128 AutoGPTQ buffers (the decode step's cost does not depend on their values)."""
    from omniquant_amd.calibrate import decoder_layer_class, default_args
    from omniquant_amd.linear import QuantLinear
    from omniquant_amd.realquant import PackedLinear, _mark_packed
    from omniquant_amd.synthetic import make_config, make_layer
    cfg = make_config("llama-7b")
    args = default_args(wbits=4, abits=16, group_size=128, lwc=True, let=False, epochs=0, nsamples=1, net="llama-7b")
    blk = decoder_layer_class("llama")(cfg, make_layer(cfg, device=dev, outliers=False), args).to(dev)
    bits, group = 4, 128
    for name, m in list(blk.named_modules()):
        if isinstance(m, QuantLinear):
            inn, out = m.in_features, m.out_features
            ng = inn // group
            p = dict(qweight=torch.randint(-2 ** 31, 2 ** 31 - 1, (inn // 32 * bits, out), dtype=torch.int32, device=dev),
                     qzeros=torch.randint(-2 ** 31, 2 ** 31 - 1, (ng, out // 32 * bits), dtype=torch.int32, device=dev),
                     scales=((torch.rand(ng, out, device=dev) + 0.5) * (0.5 / (1 << bits))).half(),
                     g_idx=torch.arange(inn, dtype=torch.int32, device=dev) // group, bias=None)
            parent = blk
            parts = name.split(".")
            for p_ in parts[:-1]:
                parent = getattr(parent, p_)
            setattr(parent, parts[-1], PackedLinear(bits, group, inn, out, p))
    _mark_packed(blk, 16)
    blk.compute_dtype = torch.bfloat16
    return blk, cfg


def block_step(dev, reps, steps_only=0):
    from omniquant_amd.kvcache import PackedKVCache
    L = 2048
    blk, cfg = packed_7b_block(dev, L)
    H, nh = cfg.hidden_size, cfg.num_attention_heads
    hd = H // nh
    cache = PackedKVCache(1, nh, hd, torch.bfloat16, dev, capacity=L + max(steps_only, 64) + 8)
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
        return None
    # launches of one step: every C-ABI call is one or more kernel launches (oq_attn_decode: two)
    calls = []
    orig = C.call
    C.call = lambda name, *a: calls.append(name) or orig(name, *a)
    try:
        step()
    finally:
        C.call = orig
    torch.cuda.synchronize()
    # eager: host time per forward call (enqueue only), and wall time per call with the device drained at the end
    n = 200
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    # device time per step from a captured graph of `reps * 10` steps
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps * 10):
            step()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    r = dict(what="packed llama-7b W4A16g128 block decode step", bs=1, L=L, dtype="bfloat16",
             graph_device_us_per_step=a.elapsed_time(b) * 1000.0 / (reps * 10),
             eager_host_us_per_call=(t1 - t0) * 1e6 / n, eager_wall_us_per_call=(t2 - t0) * 1e6 / n,
             capi_calls_per_step=len(calls), capi_calls=sorted(set(calls)),
             hip_launches_per_step=len(calls) + calls.count("oq_attn_decode"))
    print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--step-only", action="store_true", help="only N eager decode steps of the 7B block (for rocprofv3)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--codes", action="store_true", help="the code-cache kernel interleaved with the bf16-cache kernel")
    ap.add_argument("--codes8", action="store_true", help="--codes with the 8-bit code-cache kernel as a third contestant (7B, bs 8)")
    ap.add_argument("--ragged", action="store_true", help="ragged-batch kernels interleaved with the padded, masked ones")
    ap.add_argument("--paged", action="store_true", help="paged kernels interleaved with the ragged contiguous ones")
    ap.add_argument("--extend", action="store_true", help="the MFMA chunked-prefill kernel interleaved with the ragged decode kernel")
    ap.add_argument("--rounds", type=int, default=7, help="--codes / --ragged / --paged / --extend: alternating replays of the graphs")
    a = ap.parse_args()
    dev = "cuda:0"
    if not torch.cuda.is_available():
        raise SystemExit("microbench_decode needs a GPU")
    C.load()
    if a.step_only:
        block_step(dev, a.reps, steps_only=a.steps)
        return
    if a.extend:
        rows = extend_rows(a.reps, a.rounds, a.quick, dev)
    elif a.paged:
        rows = paged_rows(a.reps, a.rounds, a.quick, dev)
    elif a.ragged:
        rows = ragged_rows(a.reps, a.rounds, dev)
    elif a.codes or a.codes8:
        rows = codes_rows(a.reps, a.rounds, a.quick, dev, codes8=a.codes8)
    else:
        rows = kernel_rows(a.reps, a.quick, dev)
        rows.append(block_step(dev, a.reps))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
