"""Greedy verification on the device (csrc/oq_lmhead.hip): the LM head reduced to (max, argmax) per row against a float64
matmul, the tie rule (lowest index: inside an MFMA tile, a strip and across strips), the rows and columns it must never touch,
the tree acceptance kernel against kvcache.TokenTree.greedy_accept, the packed blocks end to end (tree step, verify, commit,
next step) and the refusals of the ABI."""
import random

import pytest
import torch

import test_hip_kv_tree as TR
from omniquant_amd import OQError, ops
from omniquant_amd import _capi as C
from omniquant_amd.kvcache import TokenTree
from omniquant_amd.specdec import GreedyVerifier
from test_hip_kv_ragged import H as RG_H
from test_hip_kv_ragged import PROMPTS, RAGGED_BLOCKS, _i32, _same, _x

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, F16, F64, I32 = torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int32
STRIP = 64                         # vocabulary rows per workgroup of lm_head_strip_kernel (only the tie placements lean on it)
VS, MS = (1, 17, 1003, 4099), (1, 5, 16, 33, 130)
_PROBLEM = {}


def _problem(dtype, H):
    """Random h [130, H] and head [4099, H], their float64 product and sum_k |h w|, computed once and left alone; the smaller
    problems are their leading rows."""
    if (dtype, H) not in _PROBLEM:
        g = torch.Generator(device=DEV).manual_seed(H + (1 if dtype == BF16 else 2))
        h = torch.randn(max(MS), H, generator=g, device=DEV).to(dtype)
        w = torch.randn(max(VS), H, generator=g, device=DEV).to(dtype)
        _PROBLEM[(dtype, H)] = (h, w, h.double() @ w.double().T, h.double().abs() @ w.double().abs().T)
    return _PROBLEM[(dtype, H)]


def _bound(mag, H):
    """B[m] = H * 2^-23 * max_v sum_k |h[m,k] w[v,k]|: bf16 / fp16 products are exact in fp32, the rest is the fp32 accumulation
    of H terms, 2^-23 per term allowing for truncating accumulators."""
    return H * 2.0 ** -23 * mag.max(dim=-1).values


def _rows_i32(rows):
    return torch.tensor(rows, dtype=I32, device=DEV)


def _first_max(x):
    V = x.shape[-1]
    cols = torch.arange(V, device=x.device).expand_as(x)
    return torch.where(x == x.max(dim=-1, keepdim=True).values, cols, V).min(dim=-1).values


# ---------------------------------------------------------------------------------------------------------------------
# 1. float64 reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 192, 1024])
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_argmax_matches_float64(dtype, H):
    h_all, w_all, ref_all, mag_all = _problem(dtype, H)
    for V in VS:
        for M in MS:
            h, w, ref = h_all[:M], w_all[:V], ref_all[:M, :V]
            B = _bound(mag_all[:M, :V], H)
            idx, val = ops.lm_head_argmax(h, w)
            assert idx.dtype == I32 and val.dtype == F32 and idx.shape == val.shape == (M,)
            assert bool(((idx >= 0) & (idx < V)).all())
            picked = ref.gather(1, idx.long()[:, None])[:, 0]
            slack = (ref.max(dim=-1).values - picked) / B
            verr = (val.double() - picked).abs() / B
            logits = torch.full((M, V), float("nan"), dtype=F32, device=DEV)
            idx2, val2 = ops.lm_head_argmax(h, w, logits=logits)
            lerr = (logits.double() - ref).abs() / B[:, None]
            print(f"{dtype} H {H} V {V} M {M}: (max - ref[idx]) / B {float(slack.max()):.3f}, |val - ref[idx]| / B "
                  f"{float(verr.max()):.3f}, |logits - ref| / B {float(lerr.max()):.3f}")
            assert bool((slack <= 2).all()) and bool((verr <= 1).all()), (V, M)
            assert bool((lerr <= 1).all()), (V, M)                   # (NaN where a logit was not written fails this)
            assert torch.equal(idx2.long(), _first_max(logits)), (V, M)
            assert _same(val2, logits.max(dim=-1).values) and _same(idx, idx2) and _same(val, val2), (V, M)


def test_argmax_shapes_and_outputs():
    h_all, w_all, _, _ = _problem(BF16, 192)
    h = h_all[:12].reshape(3, 4, 192)
    idx, val = ops.lm_head_argmax(h, w_all[:1003])
    assert idx.shape == val.shape == (3, 4)
    flat = ops.lm_head_argmax(h_all[:12], w_all[:1003])
    assert _same(idx.flatten(), flat[0]) and _same(val.flatten(), flat[1])
    out = (torch.empty(3, 4, dtype=I32, device=DEV), torch.empty(3, 4, dtype=F32, device=DEV))
    ws = torch.full((ops.lm_head_workspace(12, 1003) + 64,), 0xFF, dtype=torch.uint8, device=DEV)      # a caller's, dirty
    got = ops.lm_head_argmax(h, w_all[:1003], out=out, workspace=ws)
    assert got[0] is out[0] and got[1] is out[1] and _same(out[0], idx) and _same(out[1], val)
    one = ops.lm_head_argmax(h_all[0], w_all[:1003])
    assert one[0].shape == () and int(one[0]) == int(flat[0][0])
    v = GreedyVerifier(w_all[:1003], norm=lambda x: x)
    assert _same(v.argmax(h)[0], idx) and v._workspace is not None
    ws_id = v._workspace.data_ptr()
    assert _same(v.argmax(h)[1], val) and v._workspace.data_ptr() == ws_id                               # reused
    with pytest.raises(OQError, match="float16"):
        ops.lm_head_argmax(h.float(), w_all[:1003].float())
    with pytest.raises(OQError, match="weight"):
        ops.lm_head_argmax(h, w_all[:1003].half())
    with pytest.raises(OQError, match="hidden size"):
        ops.lm_head_argmax(h[..., :96], w_all[:1003, :96])
    with pytest.raises(OQError, match="logits"):
        ops.lm_head_argmax(h, w_all[:1003], logits=torch.empty(3, 4, 1002, dtype=F32, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------
# 2. ties
# ---------------------------------------------------------------------------------------------------------------------
TIE_V = 1003                       # 15 whole strips and a last one of 43 columns
TIE_PAIRS = {
    "tile": [(3, 9), (64 + 33, 64 + 47), (960 + 5, 960 + 12), (1001, 1002), (0, 1)],
    "strip": [(5, 50), (64 + 1, 64 + 17), (128 + 15, 128 + 16), (960, 1002), (320 + 31, 320 + 32)],
    "strips": [(10, 700), (100, 1002), (0, 961), (63, 64), (959, 960)],
}


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("where", list(TIE_PAIRS))
def test_ties_go_to_the_lowest_index(where, dtype):
    """Rows in different row tiles each get two identical head rows j1 < j2 = 4 h[m] (exact in the dtype), whose logit
    4 |h[m]|^2 ~ 4 H dominates the random rows' ~ N(0, H): the answer is j1, with the bits of j2's logit."""
    H = 128
    for p in TIE_PAIRS[where]:
        assert (p[0] // 16 == p[1] // 16) == (where == "tile") and (p[0] // STRIP == p[1] // STRIP) == (where != "strips")
    for M, rows in ((130, (0, 15, 16, 77, 129)), (20, (0, 7, 15, 16, 19)), (5, (0, 1, 2, 3, 4))):
        g = torch.Generator(device=DEV).manual_seed(M)
        h = torch.randn(M, H, generator=g, device=DEV).to(dtype)
        w = torch.randn(TIE_V, H, generator=g, device=DEV).to(dtype)
        for m, (j1, j2) in zip(rows, TIE_PAIRS[where]):
            w[j1] = w[j2] = (4 * h[m].float()).to(dtype)
            assert torch.equal(w[j1].float(), 4 * h[m].float())
        logits = torch.empty(M, TIE_V, dtype=F32, device=DEV)
        idx, val = ops.lm_head_argmax(h, w, logits=logits)
        for m, (j1, j2) in zip(rows, TIE_PAIRS[where]):
            assert _same(logits[m, j1], logits[m, j2]), (where, M, m)                 # equal rows, bit-equal logits
            others = logits[m].clone()
            others[[j1, j2]] = -float("inf")
            assert float(logits[m, j1]) > float(others.max()) + 50, (where, M, m)     # the planted pair dominates
            assert int(idx[m]) == j1 and _same(val[m], logits[m, j1]), (where, M, m, int(idx[m]))
        again = ops.lm_head_argmax(h, w)
        assert _same(again[0], idx) and _same(again[1], val)
        assert torch.equal(idx.long(), _first_max(logits))


# ---------------------------------------------------------------------------------------------------------------------
# 3. nothing outside the problem is read or written
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", ["max", "nan"])
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_nothing_outside_the_problem_is_read_or_written(dtype, poison):
    H, PAD, R = 192, 64, 70
    bad = float("nan") if poison == "nan" else torch.finfo(dtype).max
    h_all, w_all, _, _ = _problem(dtype, H)
    for V, M in ((1003, 33), (17, 5), (4099, 130), (1, 20)):
        clean_logits = torch.empty(M, V, dtype=F32, device=DEV)
        clean = ops.lm_head_argmax(h_all[:M].clone(), w_all[:V].clone(), logits=clean_logits)
        for padded in (False, True):
            wb = torch.full((V + R, H + (PAD if padded else 0)), bad, dtype=dtype, device=DEV)
            hb = torch.full((M + R, H + (PAD if padded else 0)), bad, dtype=dtype, device=DEV)
            wb[:V, :H], hb[:M, :H] = w_all[:V], h_all[:M]
            h, w = hb[:M, :H], wb[:V, :H]
            assert w.stride(0) == H + (PAD if padded else 0)
            idx = torch.full((M + 3,), -7, dtype=I32, device=DEV)
            val = torch.full((M + 3,), -7.0, dtype=F32, device=DEV)
            logits = torch.full((M + 3, V), -7.0, dtype=F32, device=DEV)
            ops.lm_head_argmax(h, w, out=(idx[:M], val[:M]), logits=logits[:M])
            assert _same(idx[:M], clean[0]) and _same(val[:M], clean[1]) and _same(logits[:M], clean_logits), (V, M, padded)
            assert bool((idx[M:] == -7).all()) and bool((val[M:] == -7.0).all()) and bool((logits[M:] == -7.0).all())
            # the verification entry reads the same operands: bs * Tq = M rows
            if M in (33, 20):
                Tq = M // (3 if M == 33 else 4)
                bs = M // Tq
                tree = TokenTree([-1] + list(range(Tq - 1)))
                draft = torch.zeros(bs, Tq, dtype=I32, device=DEV)
                got = ops.tree_verify_greedy(h.reshape(bs, Tq, H), w, tree, draft)
                assert _same(got[3].flatten(), clean[0]) and _same(got[4].flatten(), clean[1]), (V, M, padded)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the acceptance kernel against TokenTree.greedy_accept
# ---------------------------------------------------------------------------------------------------------------------
VH, VV, VBS = 128, 1003, 3
_PLANTED = {}


def _planted(Tq):
    """h [3, Tq, 128] and a head whose row T[b][t] is 4 h[b, t], so that target[b, t] = T[b][t] (distinct ids) by a margin
    above 2 B, checked here once against float64.  Ids 1000, 1001 and 1002 are no node's target: `expect` and wrong drafts."""
    if Tq not in _PLANTED:
        g = torch.Generator(device=DEV).manual_seed(Tq)
        h = torch.randn(VBS, Tq, VH, generator=g, device=DEV).to(BF16)
        w = torch.randn(VV, VH, generator=g, device=DEV).to(BF16)
        ids = torch.randperm(1000, generator=torch.Generator().manual_seed(Tq))[:VBS * Tq].reshape(VBS, Tq)
        w[ids.flatten().to(DEV)] = (4 * h.float()).to(BF16).reshape(-1, VH)
        ref = h.double().reshape(-1, VH) @ w.double().T
        B = _bound(h.double().abs().reshape(-1, VH) @ w.double().abs().T, VH)
        top = torch.topk(ref, 2, dim=-1)
        assert torch.equal(top.indices[:, 0].cpu(), ids.flatten())
        assert bool((top.values[:, 0] - top.values[:, 1] > 2 * B).all())
        _PLANTED[Tq] = (h, w, ids.tolist())
    return _PLANTED[Tq]


def _trees(Tq):
    chain = [-1] + list(range(Tq - 1))
    shared = [TR._branching(Tq).parents, TR._forest(Tq).parents, chain]
    return [TokenTree(p) for p in shared] + [TokenTree(shared), TokenTree(shared[::-1])]


WRONG, EXPECT = 1001, [1000, 1002, 1000]


def _script(tree, b, T, goal, keep, expect, rest, twin=False):
    """Sequence b's drafts: the first `keep` nodes of the root path of `goal` match (a root drafts expect[b], any other node its
    parent's target); every other node drafts `rest` (WRONG or -1); twin: a sibling of the deepest matching node drafts the
    same token as that node."""
    par = tree.parents[b] if tree.bs is not None else tree.parents
    row = [rest] * tree.Tq
    path = tree.path(goal, b)[:keep]
    for t in path:
        row[t] = T[b][par[t]] if par[t] >= 0 else (EXPECT[b] if expect else 7)
    if twin and path:
        sib = [s for s in range(tree.Tq) if s != path[-1] and par[s] == par[path[-1]]]
        if sib:
            row[sib[0]] = row[path[-1]]
    return row


def _check_verify(h, w, tree, draft, expect, T):
    exp_dev = _i32(EXPECT) if expect else None
    accept, counts, nxt, target, tval = ops.tree_verify_greedy(h, w, tree, _rows_i32(draft), exp_dev)
    Tq = tree.Tq
    assert accept.shape == target.shape == tval.shape == (VBS, Tq) and counts.shape == nxt.shape == (VBS,)
    assert target.tolist() == T
    paths, nexts = tree.greedy_accept(draft, T, EXPECT if expect else None)
    assert accept.tolist() == [p + [-1] * (Tq - len(p)) for p in paths], (tree, draft, expect)
    assert counts.tolist() == [len(p) for p in paths] and nxt.tolist() == nexts, (tree, draft, expect)
    return paths, nexts


@pytest.mark.parametrize("Tq", [1, 5, 33, 64])
def test_verification_matches_the_host_rule(Tq):
    h, w, T = _planted(Tq)
    ref_idx, ref_val = ops.lm_head_argmax(h, w)
    rng = random.Random(Tq)
    seen_high = False
    for tree in _trees(Tq):
        depth = [tree.depth[b] if tree.bs is not None else tree.depth for b in range(VBS)]
        goal = Tq - 1
        for expect in (False, True):
            # the full path of the last node, everything else wrong: exactly that path
            draft = [_script(tree, b, T, goal, Tq, expect, WRONG) for b in range(VBS)]
            paths, nexts = _check_verify(h, w, tree, draft, expect, T)
            if expect:
                assert paths == [tree.path(goal, b) for b in range(VBS)] and nexts == [T[b][goal] for b in range(VBS)]
                seen_high |= any(n >= 32 for p in paths for n in p)
            # a break at every depth (keep = 0: no root accepted), three depths at a time
            for k0 in range(0, tree.height + 1, VBS):
                keeps = [min(k0 + b, depth[b][goal] + 1) for b in range(VBS)]
                draft = [_script(tree, b, T, goal, keeps[b], expect, WRONG if expect else -1) for b in range(VBS)]
                paths, nexts = _check_verify(h, w, tree, draft, expect, T)
                assert [len(p) for p in paths] == keeps
                assert nexts == [T[b][paths[b][-1]] if paths[b] else (EXPECT[b] if expect else -1) for b in range(VBS)]
            # two accepted paths of equal depth, padded leaves, an inactive sequence
            draft = [_script(tree, 0, T, goal, Tq, expect, WRONG, twin=True), _script(tree, 1, T, goal, Tq, expect, -1), [-1] * Tq]
            paths, nexts = _check_verify(h, w, tree, draft, expect, T)
            assert paths[2] == [] and nexts[2] == (EXPECT[2] if expect else -1) and len(paths[1]) == depth[1][goal] + 1
            # random drafts: each node matches with probability 0.8, else a wrong token or padding
            for _ in range(4):
                draft = []
                for b in range(VBS):
                    par = tree.parents[b] if tree.bs is not None else tree.parents
                    draft.append([(T[b][par[t]] if par[t] >= 0 else EXPECT[b]) if rng.random() < 0.8 else rng.choice((WRONG, -1))
                                  for t in range(Tq)])
                _check_verify(h, w, tree, draft, expect, T)
    assert seen_high == (Tq > 32)                                     # a node id >= 32 on an accepted path: the high anc word
    accept, counts, nxt, target, tval = ops.tree_verify_greedy(h, w, _trees(Tq)[0], _rows_i32(draft))
    assert _same(target, ref_idx) and _same(tval, ref_val)            # the fold of the two second-stage kernels agrees


def test_verify_refuses_loudly():
    h, w, T = _planted(5)
    tree = TokenTree([-1, 0, 0, 1, 1])
    draft = torch.zeros(VBS, 5, dtype=I32, device=DEV)
    ops.tree_verify_greedy(h, w, tree, draft)
    with pytest.raises(OQError, match="batch of 3"):
        ops.tree_verify_greedy(h, w, TokenTree([tree.parents] * 2), draft)
    with pytest.raises(OQError, match="ancestor sets"):
        ops.tree_verify_greedy(h, w, TokenTree([-1, 0, 0, 1]), draft)
    with pytest.raises(OQError, match="draft"):
        ops.tree_verify_greedy(h, w, tree, draft.long())
    with pytest.raises(OQError, match="draft"):
        ops.tree_verify_greedy(h, w, tree, draft.cpu())
    with pytest.raises(OQError, match="draft"):
        ops.tree_verify_greedy(h, w, tree, draft[:, :4])
    with pytest.raises(OQError, match="expect"):
        ops.tree_verify_greedy(h, w, tree, draft, expect=torch.zeros(VBS, dtype=torch.int64, device=DEV))
    with pytest.raises(OQError, match="float16"):
        ops.tree_verify_greedy(h.float(), w.float(), tree, draft)
    with pytest.raises(OQError, match="weight"):
        ops.tree_verify_greedy(h, w.half(), tree, draft)
    with pytest.raises(OQError, match="TokenTree"):
        ops.tree_verify_greedy(h, w, tree.parents, draft)


# ---------------------------------------------------------------------------------------------------------------------
# 5. blocks end to end
# ---------------------------------------------------------------------------------------------------------------------
E2E_V = 1003


def _final_norm(x):
    x = x.float()
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6)).to(BF16)


def _host_targets(h, head):
    """Greedy tokens of rows h by a float64 matmul, and the smallest top-2 gap of a row in units of its bound B."""
    h2 = _final_norm(h).reshape(-1, h.shape[-1])
    ref = h2.double() @ head.double().T
    B = _bound(h2.double().abs() @ head.double().abs().T, h2.shape[-1])
    top = torch.topk(ref, 2, dim=-1)
    return top.indices[:, 0].reshape(h.shape[:-1]).tolist(), float(((top.values[:, 0] - top.values[:, 1]) / B).min())


def _tree_step(blk, fam, caches, tree, head, seed):
    """A tree step over drafted rows whose float64 recomputation has a top-2 gap above 2 B at EVERY node, so that no rounding of
    the kernel can flip a pick.  A gap that small turns up in about one draw of 9 x 3 random rows in a hundred (2 B is ~ 1/200
    of a typical gap), so the rows are redrawn -- by the float64 reference alone, before the kernel under test runs -- until
    the precondition holds; a redrawn step overwrites the scratch rows of the pending one."""
    for s in range(seed, seed + 40, 5):
        nodes = _x(3, tree.Tq, s)
        out = TR._model(blk, fam, nodes, caches, chain=False, tree=tree)
        target, gap = _host_targets(out, head)
        if gap > 2:
            break
    assert gap > 2, gap
    return nodes, out, target


def _drafts_for(tree, paths, target, expect):
    """Drafts under which exactly `paths` are accepted: the nodes of a path match, every other node drafts a token that is
    neither its parent's target nor expect."""
    draft = []
    for b, path in enumerate(paths):
        row = []
        for t in range(tree.Tq):
            par = tree.parents[t]
            good = target[b][par] if par >= 0 else expect[b]
            row.append(good if t in path else (good + 1) % E2E_V)
        draft.append(row)
    return draft


@pytest.mark.parametrize("storage", ["slab", "paged", "pool"])
@pytest.mark.parametrize("case", list(TR.TREE_BLOCKS))
def test_blocks_verify_and_commit_end_to_end(case, storage):
    name, _ = TR.TREE_BLOCKS[case]
    build, fam, _, _, _, _ = RAGGED_BLOCKS[name]
    blk = build()
    layers = 2 if storage == "pool" else 1
    tree = TokenTree(TR.TREE9)
    head = (torch.randn(E2E_V, RG_H, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV) * 0.5).to(BF16)
    verifier = GreedyVerifier(head, norm=_final_norm)
    caches, pool = TR._new_cache(case, storage, layers)
    top = pool or caches[0]
    TR._prefill(blk, fam, caches)
    nodes, out, target = _tree_step(blk, fam, caches, tree, head, 55)
    assert top._tree_pending == 9
    expect = [11, 12, 13]
    draft = _drafts_for(tree, TR.ACCEPT9, target, expect)
    res = verifier.verify(out, tree, _rows_i32(draft), _i32(expect))
    paths, nexts = tree.greedy_accept(draft, target, expect)
    assert paths == TR.ACCEPT9 and nexts == [target[0][4], expect[1], target[2][7]]
    assert res.target.tolist() == target
    assert res.accept.tolist() == [p + [-1] * (9 - len(p)) for p in paths]
    assert res.counts.tolist() == [len(p) for p in paths] and res.next_token.tolist() == nexts
    top.commit_tree(tree, res.accept)
    assert top._tree_pending is None
    # the ordinary step over the accepted tokens on a second cache
    counts = [len(p) for p in paths]
    lin_caches, lin_pool = TR._new_cache(case, storage, layers)
    TR._prefill(blk, fam, lin_caches)
    X = _x(3, 9, 56)
    for i, path in enumerate(paths):
        X[i, :len(path)] = nodes[i, path]
    TR._model(blk, fam, X, lin_caches, chain=False, new_tokens=_i32(counts) if storage == "pool" else counts)
    after = [n + c for n, c in zip(PROMPTS, counts)]

    def same_rows(rows):
        for l, (c, lc) in enumerate(zip(caches, lin_caches)):
            for b in range(3):
                for got, ref in zip(c.sequence(b), lc.sequence(b)):
                    assert got.shape[1] == rows[b] and _same(got, ref), (case, storage, l, b)
    if storage != "pool":                                            # (the pool's lengths are read once, at the end)
        same_rows(after)
    # the second speculative step: expect is the first one's next_token, never read by the host in between
    _, out2, target2 = _tree_step(blk, fam, caches, tree, head, 58)
    paths2 = [[0, 2, 5], [6], [0]]
    draft2 = _drafts_for(tree, paths2, target2, nexts)
    res2 = verifier.verify(out2, tree, _rows_i32(draft2), res.next_token)
    got2 = tree.greedy_accept(draft2, target2, nexts)
    assert got2[0] == paths2
    assert res2.accept.tolist() == [p + [-1] * (9 - len(p)) for p in paths2] and res2.next_token.tolist() == got2[1]
    assert res2.target.tolist() == target2
    top.commit_tree(tree, res2.accept)
    assert top.lengths.tolist() == [n + len(p) for n, p in zip(after, paths2)]
    if storage == "pool":
        assert lin_pool.lengths.tolist() == after
        for l, (c, lc) in enumerate(zip(caches, lin_caches)):       # the first commit's rows lie below the second's
            for b in range(3):
                for got, ref in zip(c.sequence(b), lc.sequence(b)):
                    assert _same(got[:, :after[b]], ref), (case, storage, l, b)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_the_abi_refuses_by_return_code():
    lib = C.load()
    M, V, H, bs, Tq = 12, 100, 128, 3, 4
    g = torch.Generator(device=DEV).manual_seed(3)
    h = torch.randn(M, H, generator=g, device=DEV).to(BF16)
    w = torch.randn(V, H, generator=g, device=DEV).to(BF16)
    ws = torch.zeros(ops.lm_head_workspace(M, V), dtype=torch.uint8, device=DEV)
    assert ws.numel() == C.size_call("oq_lm_head_workspace", M, V) > 0 and C.size_call("oq_lm_head_workspace", 0, V) == 0
    idx = torch.full((M,), -7, dtype=I32, device=DEV)
    val = torch.full((M,), -7.0, dtype=F32, device=DEV)
    outs = [torch.full((bs, Tq), -7, dtype=I32, device=DEV), torch.full((bs,), -7, dtype=I32, device=DEV),
            torch.full((bs,), -7, dtype=I32, device=DEV), torch.full((bs, Tq), -7, dtype=I32, device=DEV),
            torch.full((bs, Tq), -7.0, dtype=F32, device=DEV)]
    anc = TokenTree([-1, 0, 1, 2]).to(DEV).anc
    draft = torch.zeros(bs, Tq, dtype=I32, device=DEV)

    def head(dtype=C.OQ_BF16, H=H, ld_h=H, ld_w=H, idx=idx, wsp=ws, ws_n=ws.numel(), M=M, V=V):
        return lib.oq_lm_head_argmax(C.ptr(h), C.ptr(w), dtype, M, V, H, ld_h, ld_w, C.ptr(idx), C.ptr(val), None, C.ptr(wsp), ws_n,
                                     C.stream())

    def verify(dtype=C.OQ_BF16, H=H, Tq=Tq, anc=anc, anc_bs=1, ws_n=ws.numel(), draft=draft):
        return lib.oq_tree_verify_greedy(C.ptr(h), C.ptr(w), dtype, bs, Tq, V, H, H, H, C.ptr(anc), anc_bs, C.ptr(draft), None,
                                         *[C.ptr(t) for t in outs], C.ptr(ws), ws_n, C.stream())
    assert head(H=96) == C_UNSUPPORTED and "64" in lib.oq_last_error().decode()
    assert head(H=0) == C_UNSUPPORTED and head(H=16384 + 64) == C_UNSUPPORTED
    assert head(dtype=C.OQ_F32) == C_UNSUPPORTED and "bf16" in lib.oq_last_error().decode()
    assert head(idx=None) == C_ARG and head(wsp=None) == C_ARG
    assert head(ws_n=ws.numel() - 1) == C_ARG and "workspace" in lib.oq_last_error().decode()
    assert head(ld_h=H - 8) == C_ARG and head(ld_w=H + 4) == C_ARG and head(M=0) == C_ARG and head(V=0) == C_ARG
    assert verify(H=96) == C_UNSUPPORTED and verify(dtype=C.OQ_F32) == C_UNSUPPORTED
    assert verify(Tq=65) == C_UNSUPPORTED and "64" in lib.oq_last_error().decode()
    assert verify(Tq=0) == C_ARG
    assert verify(anc_bs=2) == C_ARG and "anc_bs" in lib.oq_last_error().decode()
    assert verify(anc_bs=0) == C_ARG and verify(anc=None) == C_ARG and verify(draft=None) == C_ARG
    assert verify(ws_n=ws.numel() - 1) == C_ARG
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((val == -7.0).all()) and bool((ws == 0).all())        # nothing was launched
    assert all(bool((t == -7).all()) for t in outs)
    assert head() == 0 and verify() == 0
    ref = ops.lm_head_argmax(h, w)
    assert _same(idx, ref[0]) and _same(val, ref[1]) and _same(outs[3].flatten(), ref[0]) and _same(outs[4].flatten(), ref[1])


C_ARG, C_UNSUPPORTED = -1, -3
