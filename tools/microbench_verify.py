"""Microbenchmark of greedy verification on one GPU (H 4096, bfloat16, cold operands):

* ops.lm_head_argmax against `(h @ w.T).argmax(-1)` (torch's GEMM writing fp32-accumulated bf16 logits, then its argmax) on the
  same tensors, V in {32000, 128256}, M in {1, 8, 64, 512}, in ONE process, the graphs replayed alternately
  (microbench_decode.interleaved) over head copies that together exceed the Infinity Cache.  Reported per case: the medians, the
  baseline's run-to-run spread, the ratio, and the share of the HBM rate (microbench_decode.HBM_BPS) the fused call reaches on
  the head's bytes alone.
* ops.tree_verify_greedy at bs 8 x Tq 64 (M = 512) next to ops.lm_head_argmax at M = 512: the difference of the two is the
  acceptance kernel in the place of the combine kernel; the same call at H = 64, where the strip kernel reads 1/64 of the head, is
  an upper bound of the acceptance kernel alone.

One JSON line per case; --out also writes them to a file.

    python tools/microbench_verify.py --out profiles/lm_head_microbench.txt
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from microbench_decode import COLD_BYTES, HBM_BPS, interleaved  # noqa: E402
from omniquant_amd import ops  # noqa: E402
from omniquant_amd.kvcache import TokenTree  # noqa: E402

H, VS, MS, BS, TQ = 4096, (32000, 128256), (1, 8, 64, 512), 8, 64


def _line(r, lines):
    lines.append(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}))
    print(lines[-1], flush=True)


def _stats(name, us, med, i, r):
    r.update({name + "_us": med[i], name + "_us_min": min(us[i]), name + "_us_max": max(us[i])})


def head_rows(V, reps, rounds, dev, lines):
    head_bytes = V * H * 2
    nsets = max(2, -(-COLD_BYTES // head_bytes))
    heads = [(torch.randn(V, H, device=dev) * 0.02).bfloat16() for _ in range(nsets)]
    for M in MS:
        h = torch.randn(M, H, device=dev).bfloat16()
        out = (torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.float32, device=dev))
        ws = torch.empty(max(ops.lm_head_workspace(M, V), 16), dtype=torch.uint8, device=dev)
        logits = torch.empty(M, V, dtype=torch.bfloat16, device=dev)
        pick = torch.empty(M, dtype=torch.int64, device=dev)

        def eager(w):
            torch.matmul(h, w.T, out=logits)
            torch.argmax(logits, dim=-1, out=pick)
        launches = ([(lambda w=w: ops.lm_head_argmax(h, w, out=out, workspace=ws)) for w in heads],
                    [(lambda w=w: eager(w)) for w in heads])
        us, med = interleaved(launches, reps, rounds)
        agree = float((out[0].long() == pick).float().mean())            # (bf16-rounded logits tie where fp32 ones do not)
        r = dict(what="lm_head_argmax", V=V, H=H, M=M, dtype="bfloat16", cache="cold", sets=nsets, rounds=rounds, head_bytes=head_bytes)
        _stats("fused", us, med, 0, r)
        _stats("matmul_argmax", us, med, 1, r)
        r.update(matmul_argmax_spread=(max(us[1]) - min(us[1])) / med[1], fused_over_matmul_argmax=med[0] / med[1],
                 fused_hbm_share=head_bytes / (med[0] * 1e-6) / HBM_BPS, picks_agree=agree)
        _line(r, lines)
    del heads
    torch.cuda.empty_cache()


def verify_rows(V, reps, rounds, dev, lines):
    head_bytes = V * H * 2
    nsets = max(2, -(-COLD_BYTES // head_bytes))
    heads = [(torch.randn(V, H, device=dev) * 0.02).bfloat16() for _ in range(nsets)]
    tree = TokenTree([-1] + [(t - 1) // 3 for t in range(1, TQ)])
    h = torch.randn(BS, TQ, H, device=dev).bfloat16()
    draft = torch.randint(0, V, (BS, TQ), dtype=torch.int32, device=dev)
    expect = torch.randint(0, V, (BS,), dtype=torch.int32, device=dev)
    out = (torch.empty(BS, TQ, dtype=torch.int32, device=dev), torch.empty(BS, TQ, dtype=torch.float32, device=dev))
    ws = torch.empty(ops.lm_head_workspace(BS * TQ, V), dtype=torch.uint8, device=dev)
    h64, heads64 = h[:, :, :64].contiguous(), [w[:, :64].contiguous() for w in heads[:2]]
    launches = ([(lambda w=w: ops.tree_verify_greedy(h, w, tree, draft, expect, workspace=ws)) for w in heads],
                [(lambda w=w: ops.lm_head_argmax(h, w, out=out, workspace=ws)) for w in heads],
                [(lambda w=w: ops.tree_verify_greedy(h64, w, tree, draft, expect, workspace=ws)) for w in heads64])
    us, med = interleaved(launches, reps, rounds)
    r = dict(what="tree_verify_greedy", V=V, H=H, bs=BS, Tq=TQ, dtype="bfloat16", cache="cold", sets=nsets, rounds=rounds)
    _stats("verify", us, med, 0, r)
    _stats("lm_head_argmax", us, med, 1, r)
    _stats("verify_at_H64", us, med, 2, r)
    r.update(acceptance_minus_combine_us=med[0] - med[1])
    _line(r, lines)
    del heads
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []
    for V in VS:
        head_rows(V, a.reps, a.rounds, dev, lines)
        verify_rows(V, a.reps, a.rounds, dev, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
