"""Microbenchmark of the speculative tree step's two kernels on one GPU (7B geometry, bs 8, bfloat16 cache, cold K/V):

* ops.tree_attention against the causal ops.extend_attention of the same Tq, slab and paged (page size 16), in ONE process,
  the graphs replayed alternately (microbench_decode.interleaved); the causal kernel's run-to-run spread is printed next to
  the ratio, and a tree kernel slower than the causal one by more than that spread is named in "slower_beyond_spread".
* ops.kv_tree_commit of one accepted path over 32 layers (one launch per buffer, K and V) against a plain strided copy of
  `height` rows per buffer (torch's copy kernel), which moves the same bytes without the path lookup.

One JSON line per case; --out also writes them to a file.

    python tools/microbench_tree.py --out profiles/tree_attention_microbench.txt
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from microbench_decode import COLD_BYTES, interleaved  # noqa: E402
from omniquant_amd import _capi as C  # noqa: E402
from omniquant_amd import ops  # noqa: E402
from omniquant_amd.kvcache import TokenTree  # noqa: E402

NH, NKV, HD, BS, LAYERS, PS = 32, 32, 128, 8, 32, 16
PASTS = (2048, 8192)


def branching(Tq):
    return TokenTree([-1] + [(t - 1) // 3 for t in range(1, Tq)])


def attention_rows(Tq, reps, rounds, dev, lines):
    tree, scale = branching(Tq), HD ** -0.5
    for past in PASTS:
        L = past + Tq
        lens = torch.full((BS,), past, dtype=torch.int32, device=dev)
        q = torch.randn(BS, Tq, NH, HD, device=dev).bfloat16()
        o = torch.empty_like(q)
        ws = torch.empty(max(C.size_call("oq_attn_extend_workspace", BS, NH, NKV, Tq, L, HD), 16), dtype=torch.uint8, device=dev)
        kv_bytes = 2 * BS * NKV * L * HD * 2
        nsets = max(2, -(-COLD_BYTES // kv_bytes))
        mp = -(-L // PS)
        slabs = [tuple(torch.randn(BS, NKV, L, HD, device=dev).bfloat16() for _ in range(2)) for _ in range(nsets)]
        pools = [tuple(torch.randn(BS * mp, NKV, PS, HD, device=dev).bfloat16() for _ in range(2)) for _ in range(nsets)]
        tables = [torch.randperm(BS * mp, generator=torch.Generator().manual_seed(i)).to(torch.int32).view(BS, mp).to(dev)
                  for i in range(nsets)]
        kw = dict(out=o, workspace=ws)
        launches = (
            [(lambda s=s: ops.extend_attention(q, s[0], s[1], L, scale, lens, **kw)) for s in slabs],
            [(lambda s=s: ops.tree_attention(q, s, L, scale, lens, tree, **kw)) for s in slabs],
            [(lambda s=s, t=t: ops.extend_attention(q, s[0], s[1], L, scale, lens, page_table=t, **kw)) for s, t in zip(pools, tables)],
            [(lambda s=s, t=t: ops.tree_attention(q, s, L, scale, lens, tree, page_table=t, **kw)) for s, t in zip(pools, tables)])
        us, med = interleaved(launches, reps, rounds)
        r = dict(what="attention", nh=NH, nkv=NKV, hd=HD, bs=BS, past=past, Tq=Tq, height=tree.height, dtype="bfloat16", cache="cold",
                 rounds=rounds, sets=nsets, kv_bytes=kv_bytes)
        slower = []
        for i, k in enumerate(("slab", "paged16")):
            c, t = 2 * i, 2 * i + 1
            spread = (max(us[c]) - min(us[c])) / med[c]
            r.update({k + "_causal_us": med[c], k + "_causal_us_min": min(us[c]), k + "_causal_us_max": max(us[c]),
                      k + "_causal_spread": spread, k + "_tree_us": med[t], k + "_tree_us_min": min(us[t]),
                      k + "_tree_us_max": max(us[t]), k + "_tree_over_causal": med[t] / med[c]})
            if med[t] > med[c] * (1.0 + spread):
                slower.append(k)
        r["slower_beyond_spread"] = slower
        lines.append(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}))
        print(lines[-1], flush=True)
        del launches, slabs, pools
        torch.cuda.empty_cache()


def commit_rows(Tq, reps, rounds, dev, lines):
    tree = branching(Tq)
    path = tree.path(Tq - 1)
    h, cap, past = len(path), 256, 128
    lens = torch.full((BS,), past, dtype=torch.int32, device=dev)
    accept = torch.tensor([path + [-1] * (Tq - h)] * BS, dtype=torch.int32, device=dev)
    k, v = (torch.randn(LAYERS, BS, NKV, cap, HD, device=dev).bfloat16() for _ in range(2))
    launches = (
        [lambda: (ops.kv_tree_commit(k, lens, accept), ops.kv_tree_commit(v, lens, accept))],
        [lambda: (k[:, :, :, past:past + h].copy_(k[:, :, :, past + Tq - h:past + Tq]),
                  v[:, :, :, past:past + h].copy_(v[:, :, :, past + Tq - h:past + Tq]))])
    us, med = interleaved(launches, reps, rounds)
    moved = 2 * LAYERS * BS * NKV * sum(1 for i, a in enumerate(path) if a != i) * HD * 2
    r = dict(what="commit", layers=LAYERS, bs=BS, nkv=NKV, hd=HD, Tq=Tq, height=h, path=path, buffers="k, v (bfloat16 slabs)",
             bytes_moved=moved, rounds=rounds, commit_us=med[0], commit_us_min=min(us[0]), commit_us_max=max(us[0]),
             copy_us=med[1], copy_us_min=min(us[1]), copy_us_max=max(us[1]), commit_over_copy=med[0] / med[1])
    lines.append(json.dumps({k_: (round(v_, 4) if isinstance(v_, float) else v_) for k_, v_ in r.items()}))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--Tq", type=int, default=33)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []
    attention_rows(a.Tq, a.reps, a.rounds, dev, lines)
    commit_rows(a.Tq, a.reps, a.rounds, dev, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
