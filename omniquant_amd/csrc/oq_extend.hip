// Chunked-prefill ("extend") attention of the packed (real-quant) blocks on gfx950: MANY query rows of a step meet a cache that
// already has a past -- a prompt fed in chunks, the suffix behind a forked prefix, a new turn of a conversation, a block of
// draft tokens.  It computes what the ragged decode kernel (oq_decode.hip, attn_decode_kernel<RAGGED>) defines: query row t of
// sequence b attends cache rows j <= lens[b] + t, lens[b] clamped to [0, L - Tq], L the host's bound of lens[b] + Tq.  That
// kernel walks the K/V range once per 8 query rows on scalar FMAs; this one contracts on v_mfma_f32_16x16x32_bf16 and reads
// each K/V tile once per 64 or 128 query rows.
// Reference lines: models/int_llama_layer.py:121-135,143-163,177 (past_key_value, scores, mask, softmax, PV).
//
// One workgroup of 4 waves per (query tile, kv head, sequence, split of the L rows).  A query tile holds rows r = t * rep + i
// of ONE kv head (rep = nh / nkv, the decode kernel's row order), 16 * NQB per wave: all query heads of a GQA group share each
// K/V tile.  K and V tiles of 64 cached rows go through LDS, double-buffered, in oq_attn.hip's layout and with its S^T operand
// trick (oq_attn_dev.h); scores, running maximum, row sum and the O accumulator stay in fp32, in the log2 domain.
// Storage: a ragged slab [bs, nkv, cap, hd] or page pools [num_pages, nkv, PS, hd] found through the page table, each as bf16
// rows or as 4-bit or 8-bit codes plus (scale, zero-point).  A code row enters LDS as code - zp (small integers, exact in bf16
// up to 256; an 8-bit row's zp lies in [0, 255]); its scale multiplies the score (K) and the probability (V) once per row, which is CodeKV's contract in oq_decode.hip.
// Rows no query of the workgroup may see (beyond lens[b] + t of its last row, or with a table entry outside [0, num_pages))
// are never loaded: they enter LDS as zeros and are masked to -inf, so scratch rows holding NaN cannot reach a result.
// Launch grid, split plan and workspace depend on shapes and L only.  Partials go to the decode workspace layout and are
// merged by attn_decode_combine_kernel in split order; with one split the output is stored directly.  No atomics, and paging
// changes addresses only: bit-identical run to run, and paged == slab bit for bit.
#include "oq_common.h"
#include "oq_attn_dev.h"
#include "oq_kv_dev.h"
#include <type_traits>

namespace {

constexpr int EXT_THREADS = 256;
constexpr int EXT_TARGET_WG = 512;      // 2 workgroups (of up to 66 KiB LDS) per CU
constexpr int EXT_MAX_SPLIT = 64;
constexpr int EXT_MIN_TILES = 4;        // a split covers at least this many 64-row key tiles

// query rows per workgroup: 64 (one 16-row block per wave) up to R = 64, else 128
inline int ext_nqb(int64_t R) { return R > 64 ? 2 : 1; }

// The split plan depends on the problem shape only: enough workgroups to fill the chip, every split a multiple of the key tile.
inline int ext_splits(int64_t bs, int64_t nkv, int64_t R, int64_t L, int64_t* chunk) {
    const int64_t qt = 64 * ext_nqb(R), base = bs * nkv * ((R + qt - 1) / qt), tiles = (L + 63) / 64;
    int64_t ns = (EXT_TARGET_WG + base - 1) / base;
    if (ns > EXT_MAX_SPLIT) ns = EXT_MAX_SPLIT;
    const int64_t by_len = (tiles + EXT_MIN_TILES - 1) / EXT_MIN_TILES;
    if (ns > by_len) ns = by_len;
    if (ns < 1) ns = 1;
    const int64_t per = (tiles + ns - 1) / ns;
    *chunk = per * 64;
    return (int)((tiles + per - 1) / per);
}

struct ExtP {
    const bf16_t* q;
    bf16_t* o;
    float* ws;
    const void *k, *v;                  // bf16 rows, or code rows of hd / 2 (4-bit) or hd (8-bit) bytes
    const f32x2 *km, *vm;               // (scale, zero-point) per code row
    const int32_t* lens;
    PageMap pm;
    int64_t Tq, cap, L, chunk;
    int nh, nkv, ns, nqt;
    float zs;                           // scale * log2(e)
};

// The TREE form (oq_attn_tree): the step's Tq <= 64 rows are the nodes of a token tree instead of a causal chunk.  anc holds
// one 64-bit set per node as (low, high) words, bit u set iff node u is the node itself or one of its ancestors (so only bits
// <= t are set for node t); cache row j is visible to node t iff j < len, or bit j - len of the node's set is set.
struct TreeP : ExtP {
    const uint2* anc;                   // [1 | bs][Tq]
    int64_t anc_bstride;                // Tq, or 0 when one tree serves the batch
};

// LDS image of a [64 rows][HD] bf16 tile: 16-byte chunks, XOR-swizzled per row (HD 128: oq_attn.hip's swz; HD 64: rows of 8
// chunks, two rows per 256-byte line)
template <int HD>
__device__ __forceinline__ int lds_off(int row, int chunk) {
    if constexpr (HD == 128) return row * 256 + ((chunk ^ swz(row)) << 4);
    else return row * 128 + ((chunk ^ (row & 7)) << 4);
}

// k-contiguous fragment: lane's 8 bf16 = X[row0 + (lane&15)][32*ks + 8*(lane>>4) .. +8]
template <int HD>
__device__ __forceinline__ bf16x8 frag_row(const char* lds, int row0, int ks, int lane) {
    return *reinterpret_cast<const bf16x8*>(lds + lds_off<HD>(row0 + (lane & 15), ks * 4 + (lane >> 4)));
}

// transposed fragment with the permuted k-slots (oq_attn.hip, frag_tr): element j<4 = X[r0 + 4g + j][col0 + (lane&15)],
// element 4+j = X[r0 + 16 + 4g + j][col0 + (lane&15)]
template <int HD>
__device__ __forceinline__ bf16x8 frag_tr(const char* lds, int r0, int col0, int lane) {
    typedef __attribute__((address_space(3))) s16x4 lds_s4;
    const int g = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
    const int ra = r0 + 4 * g + qq, rb = ra + 16;
    const int c = (col0 >> 3) + (pp >> 1), sub = (pp & 1) * 8;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(lds + lds_off<HD>(ra, c) + sub));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(lds + lds_off<HD>(rb, c) + sub));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// ---- a thread's share of a key tile on its way from memory to LDS: 64 / NP rows x one 16-byte chunk (8 dims) each.  bf16
//      rows: the chunk itself; code rows: the chunk's 8 codes (4-bit: one word, 8-bit: two) plus the row's (scale, zero-point),
//      unpacked to code - zp when it is stored.  The same registers serve K and then V of a tile.  CODES: 0, 4 or 8. ---------
template <int HD, int CODES>
struct Staged {
    static constexpr int CPR = HD / 8, RPP = EXT_THREADS / CPR, NP = 64 / RPP;
    typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
    u32x4 r[CODES ? 1 : NP];
    uint32_t w[CODES == 4 ? NP : 1];
    u32x2 w8[CODES == 8 ? NP : 1];
    f32x2 mt[CODES ? NP : 1];

    // idx[p]: the buffer row of the thread's p-th row, or -1 (not loaded: zeros)
    __device__ __forceinline__ void load(const void* buf, const f32x2* meta, const int64_t (&idx)[NP], int chunk) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if constexpr (CODES == 4) {
                w[p] = 0u;
                mt[p] = f32x2{0.f, 0.f};
                if (idx[p] >= 0) {
                    w[p] = *reinterpret_cast<const uint32_t*>((const uint8_t*)buf + idx[p] * (HD / 2) + chunk * 4);
                    mt[p] = meta[idx[p]];
                }
            } else if constexpr (CODES == 8) {
                w8[p] = u32x2{0u, 0u};
                mt[p] = f32x2{0.f, 0.f};
                if (idx[p] >= 0) {
                    w8[p] = *reinterpret_cast<const u32x2*>((const uint8_t*)buf + idx[p] * HD + chunk * 8);
                    mt[p] = meta[idx[p]];
                }
            } else {
                r[p] = u32x4{0u, 0u, 0u, 0u};
                if (idx[p] >= 0) r[p] = *reinterpret_cast<const u32x4*>((const bf16_t*)buf + idx[p] * HD + chunk * 8);
            }
        }
    }
    // sc: the tile's 64 row scales (code rows); ok: its 64 loaded-row flags (written with K when ok != NULL)
    __device__ __forceinline__ void store(char* lds, float* sc, float* ok, const int64_t (&idx)[NP], int row0, int chunk) const {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int row = row0 + RPP * p;
            if constexpr (CODES != 0) {
                bf16x8 x;
                if constexpr (CODES == 4) {
                    // dim d of the row in nibble d % 8 of word d / 8: this chunk is one word
                    const uint32_t lo = w[p] & 0x0F0F0F0Fu, hi = (w[p] >> 4) & 0x0F0F0F0Fu;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        x[2 * i] = (bf16_t)((float)((lo >> (8 * i)) & 0xFFu) - mt[p][1]);
                        x[2 * i + 1] = (bf16_t)((float)((hi >> (8 * i)) & 0xFFu) - mt[p][1]);
                    }
                } else {
                    // dim d of the row in byte d: this chunk is two words
#pragma unroll
                    for (int i = 0; i < 8; ++i) x[i] = (bf16_t)((float)((w8[p][i >> 2] >> (8 * (i & 3))) & 0xFFu) - mt[p][1]);
                }
                if (idx[p] < 0) x = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
                *reinterpret_cast<bf16x8*>(lds + lds_off<HD>(row, chunk)) = x;
                if (chunk == 0) sc[row] = idx[p] >= 0 ? mt[p][0] : 0.f;
            } else {
                *reinterpret_cast<u32x4*>(lds + lds_off<HD>(row, chunk)) = r[p];
            }
            if (ok && chunk == 0) ok[row] = idx[p] >= 0 ? 1.f : 0.f;
        }
    }
};

// One key tile for one wave.  DIAG: some (query, key) pair of the tile is masked for this wave: key 16kb + 4g + i of the tile
// is masked for the lane's query of block qb iff 16kb + i > dq[qb] (dq = last visible row - first row of the tile - 4g), and,
// PAGED, when the row was not loaded.  A query row with no visible key yet keeps m = -inf, l = 0, o = 0.
// TREE: dq[qb] is instead the 64-bit visibility set of the lane's query over the tile's keys, shifted down by 4g: key
// 16kb + 4g + i is masked iff bit 16kb + i is clear.
// meta: the tile's [K scale | V scale | loaded flag] x 64.  MID: called between the S^T MFMAs and the softmax.
template <int HD, int NQB, bool DIAG, int CODES, bool PAGED, bool TREE, typename DQ, typename MID>
__device__ __forceinline__ void ext_tile(const char* Ks, const char* Vs, const float* meta, const bf16x8 (&qf)[NQB][HD / 32],
                                         f32x4 (&o)[NQB][HD / 16], float (&m)[NQB], float (&l)[NQB], const DQ (&dq)[NQB],
                                         float zs, int lane, MID&& mid) {
    static_assert(std::is_same<DQ, typename std::conditional<TREE, uint64_t, int>::type>::value, "dq: int, or the TREE bit sets");
    constexpr int KS = HD / 32, DB = HD / 16;
    const int g = lane >> 4;
    f32x4 st[4][NQB];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) st[kb][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
    // d-step outermost: the accumulators are independent, so consecutive MFMAs never wait on each other
    bf16x8 kf[2];
    kf[0] = frag_row<HD>(Ks, 0, 0, lane);
#pragma unroll
    for (int it = 0; it < 4 * KS; ++it) {
        const int ks = it >> 2, kb = it & 3, nx = it + 1;
        if (nx < 4 * KS) kf[nx & 1] = frag_row<HD>(Ks, 16 * (nx & 3), nx >> 2, lane);
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) st[kb][qb] = MFMA(kf[it & 1], qf[qb][ks], st[kb][qb]);   // S^T: row = key, col = query
    }
    mid();
    bf16x8 vf[2];
    vf[0] = frag_tr<HD>(Vs, 0, 0, lane);             // in flight under the softmax arithmetic
    // scores in the log2 domain (code rows: times the key's scale), masked ones -inf.  Only compiler-generated instructions
    // read the MFMA accumulators (oq_attn.hip, hazard note).
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        f32x4 f = {zs, zs, zs, zs}, ok = {1.f, 1.f, 1.f, 1.f};
        if constexpr (CODES != 0) {
            const f32x4 skk = *reinterpret_cast<const f32x4*>(meta + 16 * kb + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) f[i] = skk[i] * zs;
        }
        if constexpr (PAGED) ok = *reinterpret_cast<const f32x4*>(meta + 128 + 16 * kb + 4 * g);
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float z = st[kb][qb][i] * f[i];
                bool hid;
                if constexpr (TREE) hid = ((dq[qb] >> (16 * kb + i)) & 1u) == 0;
                else hid = 16 * kb + i > dq[qb];
                if (DIAG && (hid || (PAGED && ok[i] == 0.f))) z = -INFINITY;
                st[kb][qb][i] = z;
            }
    }
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) mx = fmaxf(mx, st[kb][qb][i]);
        mx = fmaxf(mx, xor16(mx));
        mx = fmaxf(mx, xor32(mx));
        mx = fmaxf(m[qb], mx);
        const float sh = mx == -INFINITY ? 0.f : mx;                 // no visible key so far: exp2(-inf - 0) = 0 everywhere
        const float alpha = __builtin_amdgcn_exp2f(m[qb] - sh);
        m[qb] = mx;
        float ls = 0.f;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float pv = __builtin_amdgcn_exp2f(st[kb][qb][i] - sh);     // masked: exactly 0
                st[kb][qb][i] = pv;
                ls += pv;
            }
        l[qb] = fmaf(l[qb], alpha, ls);
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {       // wave-uniform: most late tiles leave the maxima alone
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int i = 0; i < 4; ++i) o[qb][db][i] *= alpha;
        }
    }
    if constexpr (CODES != 0) {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const f32x4 svk = *reinterpret_cast<const f32x4*>(meta + 64 + 16 * kb + 4 * g);
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
                for (int i = 0; i < 4; ++i) st[kb][qb][i] *= svk[i];
        }
    }
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
        bf16x8 pf[NQB];
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) pf[qb] = pack8(st[2 * kc][qb], st[2 * kc + 1][qb]);
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const int nx = kc * DB + db + 1;
            if (nx < 2 * DB) vf[nx & 1] = frag_tr<HD>(Vs, 32 * (nx / DB), 16 * (nx % DB), lane);   // V^T: row = d 16db+(lane&15)
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb) o[qb][db] = MFMA(vf[(nx - 1) & 1], pf[qb], o[qb][db]);   // O^T: row = d, col = query
        }
    }
}

template <int HD, int NQB, int CODES, bool PAGED, bool TREE = false>
__global__ void __launch_bounds__(EXT_THREADS, 2) attn_extend_kernel(typename std::conditional<TREE, TreeP, ExtP>::type p) {
    constexpr int TILE = 64 * HD * 2, KS = HD / 32, DB = HD / 16, QT = 64 * NQB;
    using St = Staged<HD, CODES>;
    constexpr int NP = St::NP;
    __shared__ __attribute__((aligned(16))) char smem[4 * TILE + 2 * 192 * 4];      // [stage][K | V], [stage][sk | sv | loaded]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
    // later query tiles see more rows: heaviest first
    const int split = (int)(blockIdx.x % p.ns), qt = p.nqt - 1 - (int)(blockIdx.x / p.ns);
    const int kvh = blockIdx.y, nkv = p.nkv;
    const int64_t b = blockIdx.z, Tq = p.Tq;
    const int rep = p.nh / nkv;
    const int64_t R = (int64_t)rep * Tq;
    int64_t len = p.lens[b];
    len = len < 0 ? 0 : (len > p.L - Tq ? p.L - Tq : len);

    // the lane's query rows (rows past R repeat the last one and are never stored)
    const int64_t q0 = (int64_t)qt * QT, qw0 = q0 + 16 * NQB * w;
    bf16x8 qf[NQB][KS];
    int64_t tq[NQB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
        int64_t r = qw0 + 16 * qb + c;
        r = r < R ? r : R - 1;
        tq[qb] = r / rep;
        const bf16_t* qp = p.q + ((b * Tq + tq[qb]) * p.nh + (int64_t)kvh * rep + (r % rep)) * HD;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[qb][ks] = *reinterpret_cast<const bf16x8*>(qp + 32 * ks + 8 * g);
    }
    // TREE: the query node's ancestor set, read once next to its q fragments; bits above the node itself are dropped, so the
    // causal bounds below (jend, vis_hi) stay upper bounds of what a row sees whatever the buffer holds
    uint64_t am[NQB];
    if constexpr (TREE) {
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) {
            const uint2 wd = p.anc[b * p.anc_bstride + tq[qb]];
            am[qb] = (((uint64_t)wd.y << 32) | wd.x) & (~uint64_t(0) >> (63 - (int)tq[qb]));     // Tq <= 64
        }
    }
    const bool live = qw0 < R;                                       // wave-uniform: the wave holds a real query row
    const int64_t vis_lo = len + (qw0 < R ? qw0 : R - 1) / rep;      // last row its first / last query row sees
    const int64_t vis_hi = len + (qw0 + 16 * NQB - 1 < R ? qw0 + 16 * NQB - 1 : R - 1) / rep;

    f32x4 o[NQB][DB];
    float m[NQB], l[NQB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
        m[qb] = -INFINITY;
        l[qb] = 0.f;
#pragma unroll
        for (int db = 0; db < DB; ++db) o[qb][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // rows [js, jend) of this split that some query row of the workgroup sees; uniform over the workgroup
    const int64_t js = split * p.chunk;
    int64_t jend = js + p.chunk < p.L ? js + p.chunk : p.L;
    {
        const int64_t last = (q0 + QT - 1 < R ? q0 + QT - 1 : R - 1) / rep;
        if (jend > len + last + 1) jend = len + last + 1;
    }
    const int ntiles = jend > js ? (int)((jend - js + 63) / 64) : 0;

    float* meta = reinterpret_cast<float*>(smem + 4 * TILE);
    const int row0 = tid / St::CPR, chunk = tid % St::CPR;
    const int64_t slab0 = (b * nkv + kvh) * p.cap;
    const int32_t* tab = PAGED ? p.pm.table + b * p.pm.max_pages : nullptr;
    St sg;
    int64_t idx[NP];
    // where the thread's rows of the tile at j0 live; -1: not loaded (at or beyond jend, or no page)
    auto locate = [&](int64_t j0) {
#pragma unroll
        for (int pp = 0; pp < NP; ++pp) {
            const int64_t j = j0 + row0 + St::RPP * pp;
            idx[pp] = -1;
            if (j < jend) {
                if constexpr (PAGED) {
                    const int64_t page = tab[j >> p.pm.lg];
                    if (page >= 0 && page < p.pm.num_pages)
                        idx[pp] = ((page * nkv + kvh) << p.pm.lg) + (j & ((int64_t(1) << p.pm.lg) - 1));
                } else {
                    idx[pp] = slab0 + j;
                }
            }
        }
    };
    if (ntiles > 0) {
        locate(js);
        sg.load(p.k, p.km, idx, chunk);
        sg.store(smem, meta, PAGED ? meta + 128 : nullptr, idx, row0, chunk);
        sg.load(p.v, p.vm, idx, chunk);
        sg.store(smem + TILE, meta + 64, nullptr, idx, row0, chunk);
        __syncthreads();
    }
    // staging registers are shared by K and V: K(j+1) is loaded before the S^T MFMAs of tile j and stored behind them, V(j+1)
    // is loaded then and stored behind the P V MFMAs; one barrier per tile
    for (int jt = 0; jt < ntiles; ++jt) {
        const int cur = jt & 1;
        const bool more = jt + 1 < ntiles;
        const int64_t j0 = js + 64 * (int64_t)jt;
        if (more) {
            locate(j0 + 64);
            sg.load(p.k, p.km, idx, chunk);
        }
        const char* Ks = smem + cur * 2 * TILE;
        const char* Vs = Ks + TILE;
        char* nxt = smem + (cur ^ 1) * 2 * TILE;
        float* nmeta = meta + (cur ^ 1) * 192;
        auto mid = [&]() {
            if (more) {
                sg.store(nxt, nmeta, PAGED ? nmeta + 128 : nullptr, idx, row0, chunk);
                sg.load(p.v, p.vm, idx, chunk);
            }
        };
        if (live && j0 <= vis_hi) {      // wave-uniform: this wave has at least one unmasked (query, key) pair in the tile
            if constexpr (TREE) {
                // the tile's keys are tree rows j0 - len + 0 .. 63: the set shifted to the tile, rows of the past (below len)
                // all visible.  A tile needs the per-element mask as soon as it reaches row len, not only on the diagonal; the
                // TREE form runs the masked body on every tile, as the PAGED forms do (a tile of the past has all bits set).
                // A second, unmasked body inlined next to it costs the slab forms 40 to 50 VGPRs and makes head_dim 128 spill.
                const int64_t s = j0 - len;
                uint64_t tv[NQB];
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) {
                    uint64_t vv = ~uint64_t(0);
                    if (s >= 64) vv = 0;
                    else if (s >= 0) vv = am[qb] >> s;
                    else if (s > -64) vv = (am[qb] << -s) | (~uint64_t(0) >> (64 + s));
                    tv[qb] = vv >> (4 * g);
                }
                ext_tile<HD, NQB, true, CODES, PAGED, true>(Ks, Vs, meta + cur * 192, qf, o, m, l, tv, p.zs, lane, mid);
            } else {
                int dq[NQB];
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) dq[qb] = (int)(len + tq[qb] - j0) - 4 * g;
                if (PAGED || j0 + 63 > vis_lo)
                    ext_tile<HD, NQB, true, CODES, PAGED, false>(Ks, Vs, meta + cur * 192, qf, o, m, l, dq, p.zs, lane, mid);
                else
                    ext_tile<HD, NQB, false, CODES, PAGED, false>(Ks, Vs, meta + cur * 192, qf, o, m, l, dq, p.zs, lane, mid);
            }
        } else {
            mid();
        }
        if (more) sg.store(nxt + TILE, nmeta + 64, nullptr, idx, row0, chunk);
        __syncthreads();
    }

    // epilogue: one split stores o; else [m, l, acc[HD]] partials per (b, kv head, split, r) for the combine kernel (a split
    // with no visible row: (-inf, 0) and zeros)
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
        float ls = l[qb];
        ls += xor16(ls);
        ls += xor32(ls);
        const int64_t r = qw0 + 16 * qb + c;
        if (r >= R) continue;
        if (p.ns == 1) {
            const float inv = 1.0f / ls;
            bf16_t* op = p.o + ((b * Tq + tq[qb]) * p.nh + (int64_t)kvh * rep + (r % rep)) * HD;
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                typedef __attribute__((ext_vector_type(4))) __bf16 bf4;
                bf4 ov;
#pragma unroll
                for (int i = 0; i < 4; ++i) ov[i] = (bf16_t)(o[qb][db][i] * inv);
                *reinterpret_cast<bf4*>(op + 16 * db + 4 * g) = ov;
            }
        } else {
            float* wr = p.ws + (((b * nkv + kvh) * p.ns + split) * R + r) * (HD + 2);
            if (g == 0) *reinterpret_cast<f32x2*>(wr) = f32x2{m[qb], ls};
#pragma unroll
            for (int db = 0; db < DB; ++db) {            // rows of HD + 2 floats: 8-byte aligned
                *reinterpret_cast<f32x2*>(wr + 2 + 16 * db + 4 * g) = f32x2{o[qb][db][0], o[qb][db][1]};
                *reinterpret_cast<f32x2*>(wr + 4 + 16 * db + 4 * g) = f32x2{o[qb][db][2], o[qb][db][3]};
            }
        }
    }
}

template <int HD, int NQB, int CODES, bool PAGED, bool TREE, typename P>
void launch_extend(const P& p, int64_t bs, hipStream_t st) {
    hipLaunchKernelGGL((attn_extend_kernel<HD, NQB, CODES, PAGED, TREE>), dim3((unsigned)(p.nqt * p.ns), p.nkv, bs), dim3(EXT_THREADS), 0, st, p);
    if (p.ns > 1)
        hipLaunchKernelGGL((attn_decode_combine_kernel<bf16_t, HD>), dim3(bs * (int64_t)p.nh * p.Tq), dim3(HD), 0, st,
                           (const float*)p.ws, p.o, p.Tq, p.nh, p.nkv, p.ns);
}

template <int HD, int NQB, bool TREE, typename P>
void launch_extend_kv(int codes, const P& p, int64_t bs, hipStream_t st) {
    if (codes == 8) {
        if (p.pm.table) launch_extend<HD, NQB, 8, true, TREE>(p, bs, st);
        else launch_extend<HD, NQB, 8, false, TREE>(p, bs, st);
    } else if (codes) {
        if (p.pm.table) launch_extend<HD, NQB, 4, true, TREE>(p, bs, st);
        else launch_extend<HD, NQB, 4, false, TREE>(p, bs, st);
    } else {
        if (p.pm.table) launch_extend<HD, NQB, 0, true, TREE>(p, bs, st);
        else launch_extend<HD, NQB, 0, false, TREE>(p, bs, st);
    }
}

template <bool TREE, typename P>
void launch_extend_hd(int hd, int nqb, int codes, const P& p, int64_t bs, hipStream_t st) {
    if (hd == 64) {
        if (nqb == 1) launch_extend_kv<64, 1, TREE>(codes, p, bs, st);
        else launch_extend_kv<64, 2, TREE>(codes, p, bs, st);
    } else {
        if (nqb == 1) launch_extend_kv<128, 1, TREE>(codes, p, bs, st);
        else launch_extend_kv<128, 2, TREE>(codes, p, bs, st);
    }
}

// codes (0, 4 or 8): k / v are the code buffers of a cache of that width and k_meta / v_meta its (scale, zero-point) pairs; 0: a
// bf16 cache's buffers.  pm.table: the buffers are page pools and cap = max_pages * page size.  anc (oq_attn_tree): the TREE form
// with the nodes' ancestor sets, anc_bs (1 or bs) of them.
int extend(const char* fn, int codes, const void* q, const void* k, const void* v, const float* k_meta, const float* v_meta, void* o,
           int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap, int64_t L, const int32_t* lens, const PageMap& pm,
           float scale, void* workspace, int64_t workspace_bytes, void* stream, const int32_t* anc = nullptr, int64_t anc_bs = 0) {
    if (!oq_attn_extend_supported(dtype, Tq, hd)) {
        oq_set_error("%s: dtype %d, head_dim %d (bf16 with head_dim 64 or 128; oq_attn_decode_* serves the rest)", fn, dtype, hd);
        return OQ_E_UNSUPPORTED;
    }
    OQ_CHECK_ARG(q && k && v && o && lens && (!codes || (k_meta && v_meta)), "%s: null pointer", fn);
    OQ_CHECK_ARG(bs > 0 && bs <= 65535 && nkv > 0 && nkv <= 65535 && nh > 0 && nh % nkv == 0, "%s: bad heads %d / %d or batch %lld", fn,
                 nh, nkv, (long long)bs);
    OQ_CHECK_ARG(Tq > 0 && L >= Tq && L <= cap && L < (int64_t(1) << 30), "%s: need 1 <= Tq (%lld) <= L (%lld) <= cap (%lld), L < 2^30", fn,
                 (long long)Tq, (long long)L, (long long)cap);
    OQ_CHECK_ARG(oq_aligned16(q) && oq_aligned16(k) && oq_aligned16(v) && oq_aligned16(o) && oq_aligned16(workspace) &&
                     oq_aligned16(k_meta) && oq_aligned16(v_meta) && (uintptr_t)lens % 4 == 0,
                 "%s: q, o, the cache buffers and the workspace must be 16-byte aligned (lens: 4)", fn);
    const int64_t R = (int64_t)(nh / nkv) * Tq;
    const int nqb = ext_nqb(R);
    const int64_t nqt = (R + 64 * nqb - 1) / (64 * nqb);
    int64_t chunk = 0;
    const int ns = ext_splits(bs, nkv, R, L, &chunk);
    OQ_CHECK_ARG(nqt * ns < (int64_t(1) << 30), "%s: too many workgroups", fn);
    if (ns > 1) {
        const int64_t need = oq_attn_extend_workspace(bs, nh, nkv, Tq, L, hd);
        OQ_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace %lld < %lld bytes", fn, (long long)workspace_bytes,
                     (long long)need);
    }
    const ExtP p{(const bf16_t*)q, (bf16_t*)o, (float*)workspace, k, v, (const f32x2*)k_meta, (const f32x2*)v_meta, lens, pm, Tq, cap, L,
                 chunk, nh, nkv, ns, (int)nqt, scale * 1.4426950408889634f};
    hipStream_t st = (hipStream_t)stream;
    if (anc) {
        TreeP tp;
        static_cast<ExtP&>(tp) = p;
        tp.anc = reinterpret_cast<const uint2*>(anc);
        tp.anc_bstride = anc_bs > 1 ? Tq : 0;
        launch_extend_hd<true>(hd, nqb, codes, tp, bs, st);
    } else {
        launch_extend_hd<false>(hd, nqb, codes, p, bs, st);
    }
    OQ_CHECK_LAUNCH(fn);
    return OQ_OK;
}

}  // namespace

extern "C" int64_t oq_attn_extend_supported(int dtype, int64_t Tq, int hd) { return dtype == OQ_BF16 && Tq > 0 && (hd == 64 || hd == 128); }

extern "C" int64_t oq_attn_extend_workspace(int64_t bs, int nh, int nkv, int64_t Tq, int64_t L, int hd) {
    if (bs <= 0 || nkv <= 0 || nh <= 0 || nh % nkv || Tq <= 0 || L <= 0 || hd <= 0) return 0;
    int64_t chunk = 0;
    const int ns = ext_splits(bs, nkv, (int64_t)(nh / nkv) * Tq, L, &chunk);
    return ns > 1 ? (int64_t)ns * bs * nh * Tq * (hd + 2) * (int64_t)sizeof(float) : 0;
}

extern "C" int oq_attn_extend(const void* q, const void* k_cache, const void* v_cache, void* o, int dtype, int64_t bs, int64_t Tq,
                              int nh, int nkv, int hd, int64_t cap, const int32_t* lens, int64_t L_bound, float scale, void* workspace,
                              int64_t workspace_bytes, void* stream) {
    return extend("oq_attn_extend", 0, q, k_cache, v_cache, nullptr, nullptr, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound, lens,
                  NO_PAGES, scale, workspace, workspace_bytes, stream);
}

extern "C" int oq_attn_extend_codes(const void* q, const void* k_codes, const void* v_codes, const float* k_meta, const float* v_meta,
                                    void* o, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap,
                                    const int32_t* lens, int64_t L_bound, float scale, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
    return extend("oq_attn_extend_codes", 4, q, k_codes, v_codes, k_meta, v_meta, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound, lens,
                  NO_PAGES, scale, workspace, workspace_bytes, stream);
}

extern "C" int oq_attn_extend_paged(const void* q, const void* k_pool, const void* v_pool, void* o, int dtype, int64_t bs, int64_t Tq,
                                    int nh, int nkv, int hd, const int32_t* table, int64_t max_pages, int64_t num_pages,
                                    int page_size, const int32_t* lens, int64_t L_bound, float scale, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    OQ_PAGE_MAP("oq_attn_extend_paged");
    return extend("oq_attn_extend_paged", 0, q, k_pool, v_pool, nullptr, nullptr, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound, lens,
                  pm, scale, workspace, workspace_bytes, stream);
}

extern "C" int oq_attn_extend_codes_paged(const void* q, const void* k_codes, const void* v_codes, const float* k_meta,
                                          const float* v_meta, void* o, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd,
                                          const int32_t* table, int64_t max_pages, int64_t num_pages, int page_size,
                                          const int32_t* lens, int64_t L_bound, float scale, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
    OQ_PAGE_MAP("oq_attn_extend_codes_paged");
    return extend("oq_attn_extend_codes_paged", 4, q, k_codes, v_codes, k_meta, v_meta, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound,
                  lens, pm, scale, workspace, workspace_bytes, stream);
}

extern "C" int oq_attn_extend_codes8(const void* q, const void* k_codes, const void* v_codes, const float* k_meta, const float* v_meta,
                                     void* o, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap,
                                     const int32_t* lens, int64_t L_bound, float scale, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
    return extend("oq_attn_extend_codes8", 8, q, k_codes, v_codes, k_meta, v_meta, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound, lens,
                  NO_PAGES, scale, workspace, workspace_bytes, stream);
}

extern "C" int oq_attn_extend_codes8_paged(const void* q, const void* k_codes, const void* v_codes, const float* k_meta,
                                           const float* v_meta, void* o, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd,
                                           const int32_t* table, int64_t max_pages, int64_t num_pages, int page_size,
                                           const int32_t* lens, int64_t L_bound, float scale, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
    OQ_PAGE_MAP("oq_attn_extend_codes8_paged");
    return extend("oq_attn_extend_codes8_paged", 8, q, k_codes, v_codes, k_meta, v_meta, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound,
                  lens, pm, scale, workspace, workspace_bytes, stream);
}

extern "C" int oq_attn_tree(const void* q, const void* k, const void* v, const float* k_meta, const float* v_meta, void* o, int dtype,
                            int code_bits, int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap, const int32_t* table,
                            int64_t max_pages, int64_t num_pages, int page_size, const int32_t* lens, int64_t L_bound,
                            const int32_t* anc, int64_t anc_bs, float scale, void* workspace, int64_t workspace_bytes,
                            void* stream) {
    const char* fn = "oq_attn_tree";
    if (Tq > 64) {
        oq_set_error("%s: Tq %lld (a token tree has at most 64 nodes: one 64-bit ancestor set per node)", fn, (long long)Tq);
        return OQ_E_UNSUPPORTED;
    }
    OQ_CHECK_ARG(code_bits == 0 || code_bits == 4 || code_bits == 8, "%s: code_bits %d (0: bf16 rows, 4 or 8)", fn, code_bits);
    OQ_CHECK_ARG(anc && (uintptr_t)anc % 8 == 0, "%s: anc (int32 [1 | bs, Tq, 2] on the device, 8-byte aligned)", fn);
    OQ_CHECK_ARG(anc_bs == 1 || anc_bs == bs, "%s: anc_bs %lld (1 or bs = %lld)", fn, (long long)anc_bs, (long long)bs);
    OQ_CHECK_ARG(lens, "%s: null lens", fn);
    PageMap pm = NO_PAGES;
    if (table) {
        if (const int rc = page_map(fn, table, max_pages, num_pages, page_size, &pm, &cap)) return rc;
    }
    return extend(fn, code_bits, q, k, v, code_bits ? k_meta : nullptr, code_bits ? v_meta : nullptr, o, dtype, bs, Tq, nh, nkv, hd, cap,
                  L_bound, lens, pm, scale, workspace, workspace_bytes, stream, anc, anc_bs);
}
