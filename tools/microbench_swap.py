"""Microbenchmark of the model-wide paged KV pool (kvcache.PagedKVPool, csrc/oq_kvpool.hip) at a 7B-shaped pool: 32 layers,
32 kv heads of 128, bfloat16, 16-row pages (a page of one layer and one of k / v is 128 KiB), sequences of 512, 4096 and
16384 rows (32, 256 and 1024 pages).

1. `--part moves`: ops.kv_pages_gather and ops.kv_pages_scatter of one sequence's pages of the k buffer, all layers in one
   launch, pages in a random order of a pool twice the sequence's size.  Next to them, in the same process and alternating
   `--rounds` times: a contiguous `copy_` of the same bytes (the ceiling: what a device-to-device copy reaches) and the
   per-page way the per-layer caches move pages, one `t[l][dst].copy_(t[l][src])` per page and layer (PagedKVCache._copy_page;
   the baseline).  GB/s counts the payload once; a copy reads and writes it, so the memory traffic is twice that.  Times are
   device events around `reps` back-to-back repetitions, median / min / max over the rounds.
2. `--part swap`: PagedKVPool.swap_out / swap_in of one sequence (k and v, all layers, default 64 MiB staging buffer): wall time
   from the call to the completion of its last copy, the first call (which allocates the pinned host tensors) apart from the
   later ones (which find them in the pinned-memory cache).  Next to it the PCIe leg alone: one non-blocking copy of the same
   bytes between a contiguous device tensor and a pinned host tensor, each way.
3. `--part host`: host milliseconds of cache bookkeeping per decode step (reserve + book_step, none of the block's kernels) at
   bs 64, 32 per-layer PagedKVCaches against the 32 views of one pool: 32 steps from 100 rows a sequence, so that step 13
   crosses a page boundary in every sequence.  book_step launches `lengths.add_` -- once per layer on the per-layer caches,
   once on the pool -- and the figure includes the host cost of those launches and of the table uploads.  Reports the median
   of the steps inside held pages, the crossing step, and the table uploads of each.

Host memory: the 16384-row rows of part 2 pin about 8 GiB (the handle's k and v tensors); torch keeps freed pinned blocks in
its cache, which `torch.cuda.empty_cache()` does not release, so the part can hold up to about 16 GiB pinned.

Without --part the three parts run as child processes, each under its own time limit, and the rows go to --out (default
profiles/kv_swap_microbench.txt); a part that fails or runs out of time ends the run.

usage: python tools/microbench_swap.py [--out FILE] [--rounds 5] [--quick] [--part moves|swap|host]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from omniquant_amd import _capi as C  # noqa: E402
from omniquant_amd import ops  # noqa: E402
from omniquant_amd.kvcache import PagedKVCache, PagedKVPool  # noqa: E402

LAYERS, NKV, HD, PS = 32, 32, 128, 16
ROWS = [512, 4096, 16384]
LIMITS = {"moves": 300, "swap": 300, "host": 120}          # seconds per part


def emit(r):
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)


def stats(name, ms, payload=None):
    med = sorted(ms)[len(ms) // 2]
    r = {name + "_ms": med, name + "_ms_min": min(ms), name + "_ms_max": max(ms)}
    if payload is not None:
        r[name + "_GBps"] = payload / med / 1e6
    return r


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def moves_rows(rounds, quick, dev):
    rows = []
    for n_rows in (ROWS[:2] if quick else ROWS):
        n = n_rows // PS
        num_pages = 2 * n
        pool = torch.empty(LAYERS, num_pages, NKV, PS, HD, dtype=torch.bfloat16, device=dev).normal_()
        pb = pool[0, 0].numel() * 2
        payload = LAYERS * n * pb
        perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(n)).tolist()
        src_l, dst_l = perm[:n], perm[n:]
        ids = torch.tensor(src_l, dtype=torch.int32, device=dev)
        flat = torch.empty((LAYERS, n, pb), dtype=torch.uint8, device=dev)
        flat2 = torch.empty_like(flat)
        reps = max(2, min(100, (16 << 30) // payload))

        def per_page():
            for l in range(LAYERS):
                t = pool[l]
                for s, d in zip(src_l, dst_l):
                    t[d].copy_(t[s])

        fns = {"gather": (lambda: ops.kv_pages_gather(pool, ids, flat), reps),
               "scatter": (lambda: ops.kv_pages_scatter(flat, pool, ids), reps),
               "contiguous_copy": (lambda: flat2.copy_(flat), reps),
               "per_page_copies": (per_page, 1)}
        for fn, _ in fns.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(rounds):
            for k, (fn, rp) in fns.items():
                ms[k].append(device_ms(fn, rp))
        r = dict(part="moves", rows=n_rows, pages=n, layers=LAYERS, page_bytes=pb, payload_bytes=payload, reps=reps, rounds=rounds,
                 per_page_launches=LAYERS * n)
        for k in fns:
            r.update(stats(k, ms[k], payload))
        med = {k: r[k + "_ms"] for k in fns}
        r.update(gather_over_contiguous=med["gather"] / med["contiguous_copy"],
                 scatter_over_contiguous=med["scatter"] / med["contiguous_copy"],
                 per_page_over_gather=med["per_page_copies"] / med["gather"],
                 contiguous_spread=(max(ms["contiguous_copy"]) - min(ms["contiguous_copy"])) / med["contiguous_copy"])
        rows.append(r)
        emit(r)
        del pool, flat, flat2
        torch.cuda.empty_cache()
    return rows


def wall_ms(fn, done):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    done(out)
    return (time.perf_counter() - t0) * 1e3, out


def swap_rows(rounds, quick, dev):
    rows = []
    for n_rows in (ROWS[:2] if quick else ROWS):
        n = n_rows // PS
        pool = PagedKVPool(LAYERS, 2, NKV, HD, torch.bfloat16, dev, num_pages=n + 8, page_size=PS, max_pages=n)
        pool.k.normal_()
        pool.v.normal_()
        pool.set_lengths([n_rows, 0])
        out_ms, in_ms = [], []
        for i in range(rounds + 1):
            ms, h = wall_ms(lambda: pool.swap_out(0), lambda h: h.event.synchronize())
            out_ms.append(ms)
            ms, _ = wall_ms(lambda: pool.swap_in(0, h), lambda _: torch.cuda.synchronize())
            in_ms.append(ms)
            payload = h.nbytes
            h = None                        # (its pinned tensors return to the pinned-memory cache before the next swap_out)
        r = dict(part="swap", rows=n_rows, pages=n, layers=LAYERS, payload_bytes=payload, staging_bytes=pool.swap_staging_bytes,
                 rounds=rounds, swap_out_first_ms=out_ms[0], swap_in_first_ms=in_ms[0])
        r.update(stats("swap_out", out_ms[1:], payload))
        r.update(stats("swap_in", in_ms[1:], payload))
        del pool
        torch.cuda.empty_cache()
        # the PCIe leg alone: the same bytes in the handle's two pieces (k and v), contiguous on both sides
        devt = [torch.empty(payload // 2, dtype=torch.uint8, device=dev) for _ in range(2)]
        host = [torch.empty(payload // 2, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        d2h, h2d = [], []
        for i in range(rounds + 1):
            d2h.append(wall_ms(lambda: [h_.copy_(d_, non_blocking=True) for h_, d_ in zip(host, devt)],
                               lambda _: torch.cuda.synchronize())[0])
            h2d.append(wall_ms(lambda: [d_.copy_(h_, non_blocking=True) for h_, d_ in zip(host, devt)],
                               lambda _: torch.cuda.synchronize())[0])
        r.update(stats("pcie_d2h", d2h[1:], payload))
        r.update(stats("pcie_h2d", h2d[1:], payload))
        r.update(swap_out_over_pcie=r["swap_out_ms"] / r["pcie_d2h_ms"], swap_in_over_pcie=r["swap_in_ms"] / r["pcie_h2d_ms"])
        rows.append(r)
        emit(r)
        del devt, host
        torch.cuda.empty_cache()
    return rows


def host_rows(dev):
    bs, start, steps = 64, 100, 32
    num_pages = bs * (-(-(start + steps) // PS) + 1)
    tokens = (None, 1, None)
    rows = []
    for kind in ("per_layer", "pool"):
        if kind == "pool":
            pool = PagedKVPool(LAYERS, bs, NKV, HD, torch.bfloat16, dev, num_pages, page_size=PS)
            caches, owners = [pool.layer(l) for l in range(LAYERS)], [pool]
        else:
            caches = [PagedKVCache(bs, NKV, HD, torch.bfloat16, dev, num_pages, page_size=PS) for _ in range(LAYERS)]
            owners = caches
        for o in owners:
            o.set_lengths([start] * bs)
        uploads = []
        for o in owners:
            def counted(inner=o._upload):
                uploads.append(1)
                inner()
            o._upload = counted
        torch.cuda.synchronize()
        ms, ups = [], []
        for s in range(steps):
            before = len(uploads)
            t0 = time.perf_counter()
            for c in caches:
                c.reserve(1)
                c.book_step(1, tokens)
            ms.append((time.perf_counter() - t0) * 1e3)
            ups.append(len(uploads) - before)
        torch.cuda.synchronize()
        cross = [i for i, u in enumerate(ups) if u]
        inside = sorted(m for i, m in enumerate(ms) if not ups[i] and i > 0)
        r = dict(part="host", kind=kind, bs=bs, layers=LAYERS, steps=steps, crossing_steps=cross,
                 inside_pages_ms=inside[len(inside) // 2], inside_pages_ms_min=inside[0], inside_pages_ms_max=inside[-1],
                 crossing_ms=max(ms[i] for i in cross), uploads_on_crossing=max(ups), uploads_inside_pages=min(ups))
        rows.append(r)
        emit(r)
        del caches, owners
        torch.cuda.empty_cache()
    rows.append(dict(part="host", per_layer_over_pool_inside_pages=rows[0]["inside_pages_ms"] / rows[1]["inside_pages_ms"],
                     per_layer_over_pool_crossing=rows[0]["crossing_ms"] / rows[1]["crossing_ms"]))
    emit(rows[-1])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_swap_microbench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="sequences of 512 and 4096 rows only")
    ap.add_argument("--part", choices=sorted(LIMITS), default=None)
    a = ap.parse_args()
    if a.part is None:
        # each part in a process of its own, under its own time limit; the first one that fails ends the run
        lines = []
        for part in ("moves", "swap", "host"):
            cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--rounds", str(a.rounds)] + (["--quick"] if a.quick else [])
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMITS[part])
            except subprocess.TimeoutExpired as e:
                got = e.stdout or ""
                lines += [ln for ln in (got if isinstance(got, str) else got.decode()).splitlines() if ln.startswith("{")]
                lines.append(json.dumps(dict(part=part, error=f"ended at its time limit of {LIMITS[part]} s")))
                break
            lines += [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0:
                lines.append(json.dumps(dict(part=part, error=f"exit status {p.returncode}")))
                break
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        raise SystemExit(1 if any('"error"' in ln for ln in lines) else 0)
    if not torch.cuda.is_available():
        raise SystemExit("microbench_swap needs a GPU")
    C.load()
    dev = "cuda:0"
    if a.part == "moves":
        moves_rows(a.rounds, a.quick, dev)
    elif a.part == "swap":
        swap_rows(a.rounds, a.quick, dev)
    else:
        host_rows(dev)


if __name__ == "__main__":
    main()
