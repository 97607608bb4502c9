// Greedy verification on the device: the LM head reduced to one (max, argmax) pair per row without storing logits, and the
// greedy acceptance of a speculative step's token tree (the reference's evaluation / generation path runs lm_head and an
// argmax over a stored [rows, vocab] logits tensor; the token tree is kvcache.TokenTree's).
//
//   lm_head_strip_kernel   one workgroup (4 waves) owns a strip of LH_SN = 64 vocabulary rows of the head over ALL of H and
//                          walks the row tiles of h itself, so a strip is fetched by one workgroup only.  Per row tile (16 * MT
//                          rows, MT in {1, 2, 4} chosen from M) it runs K in steps of 128: the h tile and the strip's tile go
//                          global -> registers -> LDS (16-B chunks, XOR-swizzled rows; the loads of the next TWO steps are in
//                          flight under the MFMAs), each wave multiplies its 16 vocabulary rows against every row of the tile with
//                          v_mfma_f32_16x16x32_bf16 / _f16 (fp32 accumulators), and the [rows, 64] logits are reduced in
//                          registers (4 columns per lane), across the 4 lane groups of a wave (two shuffles) and across the 4
//                          waves (LDS) to ONE (max, index) pair per row, written to workspace[row][strip].  Logits reach memory
//                          only when the caller passes a logits buffer.
//   lm_head_combine_kernel one wave per row folds the strip partials into idx / val.
//   tree_verify_kernel     one workgroup per sequence: its 16 waves share the same fold for the Tq nodes, then ONE wave, lane t =
//                          node t, decides the accepted root path from the ancestor words kvcache.TokenTree.to(device) uploads.
// Ties: every comparison is "greater, or equal with the lower index", so the lowest index wins in a lane, in a wave, in a strip
// and across strips.  Every output element accumulates the same MFMA sequence over k, so equal head rows give bit-equal
// logits.  No atomics, no arrival order: results are bit-identical run to run.  Rows >= M are loaded as row M - 1 and never
// stored; columns >= V are loaded as row V - 1 of the head and excluded from every comparison.
#include "oq_common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

constexpr int LH_SN = 64;        // vocabulary rows of a strip: V = 32000 -> 500 workgroups, two per CU of 256
constexpr int LH_BK = 128;       // K step: one LDS row is 256 bytes = 16 chunks of 16 bytes
constexpr int LH_ROWB = LH_BK * 2;

struct LmP {
    const void* h;
    const void* w;
    int64_t M, V, H, ld_h, ld_w, ns;
    float* logits;
    int2* part;                  // [M][ns] (max as float bits, index)
};

__device__ __forceinline__ int lh_off(int row, int chunk) { return row * LH_ROWB + ((chunk ^ (row & 15)) << 4); }

// (v, i) <- the better of (v, i) and (ov, oi): greater value, or the lower index among equals; a NaN never replaces anything
__device__ __forceinline__ void lh_take(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

__device__ __forceinline__ void lh_wave_best(float& v, int& i, int from = 1) {
#pragma unroll
    for (int s = from; s < 64; s <<= 1) {
        const float ov = __shfl_xor(v, s, 64);
        const int oi = __shfl_xor(i, s, 64);
        lh_take(v, i, ov, oi);
    }
}

// the fold of one row's strip partials by one wave: every lane ends with the row's (max, lowest argmax); four loads in flight
__device__ __forceinline__ void lh_fold_row(const int2* part, int64_t ns, int lane, float& v, int& i) {
    v = -INFINITY;
    i = 0x7fffffff;
    for (int64_t s0 = lane; s0 < ns; s0 += 256) {
        int2 pr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            pr[j] = s0 + 64 * j < ns ? part[s0 + 64 * j] : make_int2(__builtin_bit_cast(int, -INFINITY), 0x7fffffff);
#pragma unroll
        for (int j = 0; j < 4; ++j) lh_take(v, i, __builtin_bit_cast(float, pr[j].x), pr[j].y);
    }
    lh_wave_best(v, i);
}

template <typename TX, int MT>
__global__ void __launch_bounds__(256) lm_head_strip_kernel(LmP p) {
    constexpr int ROWS = MT * 16;
    __shared__ __attribute__((aligned(16))) char smem[(LH_SN + ROWS) * LH_ROWB];     // the strip's tile, then the h tile
    __shared__ float red_v[4][ROWS];
    __shared__ int red_i[4][ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * LH_SN;
    const TX* W = reinterpret_cast<const TX*>(p.w);
    const TX* Hp = reinterpret_cast<const TX*>(p.h);
    char* sw = smem;
    char* sh = smem + LH_SN * LH_ROWB;
    // staging: chunk c = tid + 256 * i -> row c >> 4, 16-byte chunk c & 15 of the K step (the same for every i)
    const int kc = tid & 15, r0 = tid >> 4;
    const TX* wsrc[4];
    int woff[4], hoff[MT];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = r0 + 16 * i;
        const int64_t n = n0 + row < p.V ? n0 + row : p.V - 1;
        wsrc[i] = W + n * p.ld_w + kc * 8;
        woff[i] = lh_off(row, kc);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) hoff[i] = lh_off(r0 + 16 * i, kc);
    const int64_t nt = (p.H + LH_BK - 1) / LH_BK;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    for (int64_t m0 = 0; m0 < p.M; m0 += ROWS) {
        const TX* hsrc[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int64_t m = m0 + r0 + 16 * i < p.M ? m0 + r0 + 16 * i : p.M - 1;
            hsrc[i] = Hp + m * p.ld_h + kc * 8;
        }
        f32x4 acc[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        // two register stages: K step t + 2 is requested before step t is multiplied, so two steps of the strip are in flight
        auto load = [&](u32x4(&rw)[4], u32x4(&rh)[MT], int64_t t) {
            const int64_t k = t * LH_BK;
            const bool in = t < nt && k + kc * 8 < p.H;   // H is a multiple of 64: chunks 8..15 of a last, half K step are zeros
#pragma unroll
            for (int i = 0; i < 4; ++i) rw[i] = in ? *reinterpret_cast<const u32x4*>(wsrc[i] + k) : zero4;
#pragma unroll
            for (int i = 0; i < MT; ++i) rh[i] = in ? *reinterpret_cast<const u32x4*>(hsrc[i] + k) : zero4;
        };
        auto step = [&](u32x4(&rw)[4], u32x4(&rh)[MT], int64_t t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(sw + woff[i]) = rw[i];
#pragma unroll
            for (int i = 0; i < MT; ++i) *reinterpret_cast<u32x4*>(sh + hoff[i]) = rh[i];
            __syncthreads();
            load(rw, rh, t + 2);
            const int steps = p.H - t * LH_BK >= LH_BK ? 4 : 2;
            for (int ks = 0; ks < steps; ++ks) {
                const int ch = ks * 4 + (lane >> 4);
                const s16x8 fb = *reinterpret_cast<const s16x8*>(sw + lh_off(wid * 16 + (lane & 15), ch));
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const s16x8 fa = *reinterpret_cast<const s16x8*>(sh + lh_off(i * 16 + (lane & 15), ch));
                    // head rows as the first operand: lane ends with C[m = lane & 15][n = 4 * (lane >> 4) + r]
                    if constexpr (__is_same(TX, f16_t))
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, fb), __builtin_bit_cast(f16x8, fa),
                                                                        acc[i], 0, 0, 0);
                    else
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fb),
                                                                         __builtin_bit_cast(bf16x8, fa), acc[i], 0, 0, 0);
                }
            }
            __syncthreads();
        };
        u32x4 rw0[4], rh0[MT], rw1[4], rh1[MT];
        load(rw0, rh0, 0);
        load(rw1, rh1, 1);
        for (int64_t t = 0; t < nt; t += 2) {
            step(rw0, rh0, t);
            if (t + 1 < nt) step(rw1, rh1, t + 1);
        }
        // this wave's [ROWS, 16] logits -> one pair per row
        const int64_t nl = n0 + wid * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int64_t m = m0 + i * 16 + (lane & 15);
            float bv = -INFINITY;
            int bi = (int)n0;                             // (n0 < V: an index inside the problem whatever the values are)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = acc[i][r];
                if (nl + r < p.V) {
                    if (p.logits && m < p.M) p.logits[m * p.V + nl + r] = v;
                    if (v > bv) {
                        bv = v;
                        bi = (int)(nl + r);
                    }
                }
            }
            lh_wave_best(bv, bi, 16);                     // lanes l, l ^ 16, l ^ 32, l ^ 48 hold the same row
            if (lane < 16) {
                red_v[wid][i * 16 + lane] = bv;
                red_i[wid][i * 16 + lane] = bi;
            }
        }
        __syncthreads();
        if (tid < ROWS && m0 + tid < p.M) {
            float bv = red_v[0][tid];
            int bi = red_i[0][tid];
#pragma unroll
            for (int w = 1; w < 4; ++w) lh_take(bv, bi, red_v[w][tid], red_i[w][tid]);
            p.part[(m0 + tid) * p.ns + blockIdx.x] = make_int2(__builtin_bit_cast(int, bv), bi);
        }
        // (the next tile's first barrier separates these reads from its writes of red_*)
    }
}

__global__ void __launch_bounds__(256) lm_head_combine_kernel(const int2* part, int64_t M, int64_t ns, int32_t* idx, float* val) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    float v;
    int i;
    lh_fold_row(part + m * ns, ns, lane, v, i);
    if (lane == 0) {
        idx[m] = i;
        val[m] = v;
    }
}

struct TvP {
    const int2* part;
    int64_t ns;
    int Tq;
    const int32_t* anc;
    int64_t anc_bs;
    const int32_t* draft;
    const int32_t* expect;
    int32_t* accept;
    int32_t* counts;
    int32_t* next_token;
    int32_t* target;
    float* target_val;
};

constexpr int TV_WAVES = 16;

__global__ void __launch_bounds__(64 * TV_WAVES) tree_verify_kernel(TvP p) {
    __shared__ float tgt_v[64];
    __shared__ int tgt_i[64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, Tq = p.Tq;
    const int64_t b = blockIdx.x;
    for (int t = wid; t < Tq; t += TV_WAVES) {            // the waves share the folds; wave 0 alone decides
        float v;
        int i;
        lh_fold_row(p.part + (b * Tq + t) * p.ns, p.ns, lane, v, i);
        if (lane == 0) {
            tgt_v[t] = v;
            tgt_i[t] = i;
        }
    }
    __syncthreads();
    if (wid != 0) return;
    const bool node = lane < Tq;
    const float tv = node ? tgt_v[lane] : -INFINITY;
    const int ti = node ? tgt_i[lane] : 0;
    uint64_t a = 0;
    int d = -1;
    if (node) {
        const int32_t* an = p.anc + ((p.anc_bs == 1 ? 0 : b) * Tq + lane) * 2;
        a = (uint64_t)(uint32_t)an[0] | ((uint64_t)(uint32_t)an[1] << 32);
        a = (a & ((2ull << lane) - 1ull)) | (1ull << lane);          // bits above t are ignored, as in the tree attention
        d = p.draft[b * Tq + lane];
        p.target[b * Tq + lane] = ti;
        p.target_val[b * Tq + lane] = tv;
    }
    const uint64_t above = a & ~(1ull << lane);
    const int parent = above ? 63 - __builtin_clzll(above) : -1;
    const int ptarget = __shfl(ti, parent < 0 ? 0 : parent, 64);
    const int want = p.expect ? p.expect[b] : -1;
    const bool ok = node && d >= 0 && (parent < 0 ? (p.expect == nullptr || d == want) : d == ptarget);
    const uint64_t okmask = __ballot(ok);
    const bool accepted = node && (a & ~okmask) == 0;
    int key = accepted ? __builtin_popcountll(a) * 64 + (63 - lane) : -1;       // deepest first, then the lowest id
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_xor(key, s, 64);
        key = o > key ? o : key;
    }
    uint64_t path = 0;
    int next = want;
    if (key >= 0) {
        const int best = 63 - (key & 63);
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)a, best, 64);
        const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(a >> 32), best, 64);
        path = (uint64_t)lo | ((uint64_t)hi << 32);
        next = __shfl(ti, best, 64);
    }
    const int cnt = __builtin_popcountll(path);
    if (node) {
        if (path >> lane & 1) p.accept[b * Tq + __builtin_popcountll(path & ((1ull << lane) - 1ull))] = lane;
        if (lane >= cnt) p.accept[b * Tq + lane] = -1;
    }
    if (lane == 0) {
        p.counts[b] = cnt;
        p.next_token[b] = next;
    }
}

int64_t lh_strips(int64_t V) { return (V + LH_SN - 1) / LH_SN; }

template <typename TX>
void launch_strips(const LmP& p, hipStream_t st) {
    const dim3 grid((unsigned)p.ns);
    if (p.M <= 16) hipLaunchKernelGGL((lm_head_strip_kernel<TX, 1>), grid, dim3(256), 0, st, p);
    else if (p.M <= 32) hipLaunchKernelGGL((lm_head_strip_kernel<TX, 2>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((lm_head_strip_kernel<TX, 4>), grid, dim3(256), 0, st, p);
}

// what both entry points check alike; fills p
int head_args(const char* fn, const void* h, const void* w, int dtype, int64_t M, int64_t V, int64_t H, int64_t ld_h, int64_t ld_w,
              float* logits, void* workspace, int64_t workspace_bytes, LmP& p) {
    if (dtype != OQ_BF16 && dtype != OQ_F16) {
        oq_set_error("%s: dtype %d (bf16 or fp16, the same for h and the head)", fn, dtype);
        return OQ_E_UNSUPPORTED;
    }
    if (H < 64 || H > 16384 || H % 64 != 0) {
        oq_set_error("%s: H %lld (a multiple of 64 from 64 to 16384)", fn, (long long)H);
        return OQ_E_UNSUPPORTED;
    }
    OQ_CHECK_ARG(h && w && workspace, "%s: null pointer", fn);
    OQ_CHECK_ARG(M >= 1 && V >= 1 && V <= 0x7fffffffLL - LH_SN, "%s: M %lld, V %lld", fn, (long long)M, (long long)V);
    OQ_CHECK_ARG(ld_h >= H && ld_w >= H && ld_h % 8 == 0 && ld_w % 8 == 0, "%s: ld_h %lld / ld_w %lld (multiples of 8, >= H %lld)", fn,
                 (long long)ld_h, (long long)ld_w, (long long)H);
    OQ_CHECK_ARG(oq_aligned16(h) && oq_aligned16(w) && (uintptr_t)workspace % 8 == 0 && (uintptr_t)logits % 4 == 0,
                 "%s: h / w must be 16-byte, the workspace 8-byte aligned", fn);
    const int64_t need = oq_lm_head_workspace(M, V);
    OQ_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %lld bytes needed (oq_lm_head_workspace), %lld given", fn, (long long)need,
                 (long long)workspace_bytes);
    p = LmP{h, w, M, V, H, ld_h, ld_w, lh_strips(V), logits, (int2*)workspace};
    return OQ_OK;
}

}  // namespace

extern "C" int64_t oq_lm_head_workspace(int64_t M, int64_t V) {
    if (M <= 0 || V <= 0) return 0;
    return M * lh_strips(V) * (int64_t)sizeof(int2);
}

extern "C" int oq_lm_head_argmax(const void* h, const void* w, int dtype, int64_t M, int64_t V, int64_t H, int64_t ld_h, int64_t ld_w,
                                 int32_t* idx, float* val, float* logits, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "oq_lm_head_argmax";
    LmP p;
    if (int rc = head_args(fn, h, w, dtype, M, V, H, ld_h, ld_w, logits, workspace, workspace_bytes, p)) return rc;
    OQ_CHECK_ARG(idx && val, "%s: null idx / val", fn);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == OQ_F16) launch_strips<f16_t>(p, st);
    else launch_strips<bf16_t>(p, st);
    hipLaunchKernelGGL(lm_head_combine_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, p.part, M, p.ns, idx, val);
    OQ_CHECK_LAUNCH(fn);
    return OQ_OK;
}

extern "C" int oq_tree_verify_greedy(const void* h, const void* w, int dtype, int64_t bs, int Tq, int64_t V, int64_t H, int64_t ld_h,
                                     int64_t ld_w, const int32_t* anc, int64_t anc_bs, const int32_t* draft, const int32_t* expect,
                                     int32_t* accept, int32_t* counts, int32_t* next_token, int32_t* target, float* target_val,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "oq_tree_verify_greedy";
    if (Tq > 64) {
        oq_set_error("%s: Tq %d (a token tree has at most 64 nodes: one 64-bit ancestor set per node)", fn, Tq);
        return OQ_E_UNSUPPORTED;
    }
    OQ_CHECK_ARG(Tq >= 1 && bs >= 1 && bs <= 0x7fffffffLL, "%s: bs %lld, Tq %d", fn, (long long)bs, Tq);
    LmP p;
    if (int rc = head_args(fn, h, w, dtype, bs * Tq, V, H, ld_h, ld_w, nullptr, workspace, workspace_bytes, p)) return rc;
    OQ_CHECK_ARG(anc && (uintptr_t)anc % 4 == 0, "%s: anc (int32 [1 | bs, Tq, 2] on the device)", fn);
    OQ_CHECK_ARG(anc_bs == 1 || anc_bs == bs, "%s: anc_bs %lld (1 or bs = %lld)", fn, (long long)anc_bs, (long long)bs);
    OQ_CHECK_ARG(draft && accept && counts && next_token && target && target_val, "%s: null pointer", fn);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == OQ_F16) launch_strips<f16_t>(p, st);
    else launch_strips<bf16_t>(p, st);
    TvP t{p.part, p.ns, Tq, anc, anc_bs, draft, expect, accept, counts, next_token, target, target_val};
    hipLaunchKernelGGL(tree_verify_kernel, dim3((unsigned)bs), dim3(64 * TV_WAVES), 0, st, t);
    OQ_CHECK_LAUNCH(fn);
    return OQ_OK;
}
