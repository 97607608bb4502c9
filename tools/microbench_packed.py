"""Microbenchmark of the real-quant inference kernels (csrc/oq_packed.hip) on the LLaMA-7B projection shapes and one
LLaMA-2-70B GQA k/v shape, against two baselines (bf16 activations only):
  deq+gemm   oq_packed_dequant -> bf16 weight, then oq_gemm   (what an unfused dequantise-then-matmul costs)
  resident   oq_gemm on a bf16 weight that is already resident (the unquantised model)

Cache state: decode rows (M <= 16) rotate through enough distinct weight sets (packed AND bf16) that one round reads more than
the 256 MiB Infinity Cache, so every launch streams its weight from HBM ("cold").  M = 64 / 2048 reuse each weight tile many
times and are compute-bound; they rotate through 2 sets ("warm": the weight may be cache-resident).  Every shape is warmed up
once before it is timed; all numbers come from one process, each from one captured graph of `reps` rounds over the sets,
replayed once warm and once under hipEvents (divided by the launch count).

usage: python tools/microbench_packed.py [--out FILE] [--reps 3] [--quick]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omniquant_amd import _capi as C  # noqa: E402
from omniquant_amd import ops  # noqa: E402

SHAPES = [("7b qkv/o", 4096, 4096), ("7b gate/up", 11008, 4096), ("7b down", 4096, 11008), ("70b k/v (GQA)", 1024, 8192)]
MS = [1, 4, 16, 64, 2048]
COLD_BYTES = 320 << 20           # > 256 MiB Infinity Cache


def packed_set(bits, group, K, N, dev):
    ng = K // group
    return dict(qw=torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 32 * bits, N), dtype=torch.int32, device=dev),
                qz=torch.randint(-2 ** 31, 2 ** 31 - 1, (ng, N // 32 * bits), dtype=torch.int32, device=dev),
                sc=((torch.rand(ng, N, device=dev) + 0.5) * (0.5 / (1 << bits))).half())


def packed_bytes(bits, group, K, N):
    return K * N * bits // 8 + (K // group) * N * (2 + bits / 8)


def timed(fns, reps):
    """Mean time per launch of `reps` rounds over fns, replayed from one captured graph (a decode launch takes a few us: the
    host-side cost of a ctypes call would otherwise be what is measured)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="4-bit g128 only")
    a = ap.parse_args()
    dev = "cuda:0"
    C.load()
    rows = []
    configs = [(4, 128)] if a.quick else [(4, 128), (4, None), (3, 128), (3, None), (2, 128), (2, None)]
    for name, N, K in SHAPES:
        for bits, g in configs:
            group = g or K
            for M in MS:
                cold = M <= 16
                nsets = max(2, -(-COLD_BYTES // int(packed_bytes(bits, group, K, N)))) if cold else 2
                sets = [packed_set(bits, group, K, N, dev) for _ in range(nsets)]
                for dtype in (torch.bfloat16, torch.float16):
                    x = torch.randn(M, K, device=dev).to(dtype)
                    y = torch.empty(M, N, device=dev, dtype=dtype)
                    dt = C.dt(x)
                    ws_n = C.size_call("oq_packed_gemv_workspace", M, K, N, bits) if M <= 16 else 0
                    ws = torch.empty(max(ws_n, 1), dtype=torch.uint8, device=dev)
                    r = dict(shape=name, N=N, K=K, bits=bits, group=g or "channel", M=M, dtype=str(dtype).split(".")[-1],
                             cache="cold" if cold else "warm")

                    def gemv(s):
                        return lambda: C.call("oq_packed_gemv", x.data_ptr(), dt, M, K, N, group, bits, s["qw"].data_ptr(),
                                              s["qz"].data_ptr(), s["sc"].data_ptr(), None, None, y.data_ptr(), ws.data_ptr(),
                                              ws_n, C.stream())

                    def gemm(s):
                        return lambda: C.call("oq_packed_gemm", x.data_ptr(), dt, M, K, N, group, bits, s["qw"].data_ptr(),
                                              s["qz"].data_ptr(), s["sc"].data_ptr(), None, None, y.data_ptr(), C.stream())

                    if M <= 16:
                        r["gemv_us"] = timed([gemv(s) for s in sets], a.reps)
                        r["gemv_GBps"] = packed_bytes(bits, group, K, N) / r["gemv_us"] / 1e3
                    r["gemm_us"] = timed([gemm(s) for s in sets], a.reps)
                    if dtype == torch.bfloat16:
                        wtmp = torch.empty(N, K, device=dev, dtype=torch.bfloat16)

                        def deq_gemm(s):
                            def f():
                                C.call("oq_packed_dequant", s["qw"].data_ptr(), s["qz"].data_ptr(), s["sc"].data_ptr(), K, N, group,
                                       bits, wtmp.data_ptr(), C.OQ_BF16, C.stream())
                                ops.gemm(x, wtmp, y, M, N, K, K, K, N, True, True)
                            return f

                        r["deq_gemm_us"] = timed([deq_gemm(s) for s in sets], a.reps)
                        nres = max(2, -(-COLD_BYTES // (N * K * 2))) if cold else 2
                        if g == 128 and bits == 4:          # the resident bf16 weight does not depend on the packing
                            dense = [torch.randn(N, K, device=dev).to(torch.bfloat16) for _ in range(nres)]
                            r["resident_us"] = timed([(lambda w: (lambda: ops.gemm(x, w, y, M, N, K, K, K, N, True, True)))(w)
                                                      for w in dense], a.reps)
                            r["resident_GBps"] = N * K * 2 / r["resident_us"] / 1e3
                            del dense
                        del wtmp
                    if M == 2048:
                        fl = 2.0 * M * N * K
                        for k in ("gemm_us", "deq_gemm_us", "resident_us"):
                            if k in r:
                                r[k.replace("_us", "_TFLOPs")] = fl / r[k] / 1e6
                    rows.append(r)
                    print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
                del sets
                torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
