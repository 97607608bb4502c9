// Incremental-decoding kernels of the packed (real-quant) blocks on gfx950: the KV-cache append with RoPE at arbitrary
// positions (one kernel template; its QUANT instantiations add the W4A4 head quantisers and serve oq_kv_append_quant, its
// CODES instantiations also store the 4-bit codes: oq_kv_append_quant_codes; CODES = 8 quantises k and v alone, on a 255-level
// grid whose range contains zero, for the weight-only blocks: oq_kv_append_codes8), and attention of 1..Tq query rows against
// the cached K/V, held as floats (oq_attn_decode), as 4-bit codes (oq_attn_decode_codes) or as 8-bit codes
// (oq_attn_decode_codes8).
// Reference lines: models/int_llama_layer.py:121-135,177 (rotary embedding gathered at position_ids, torch.cat with
// past_key_value, present_key_value) and :143-163 (scores, mask, softmax, PV); models/int_opt_layer.py:110-121,151-170.
//
// Decode attention is HBM-bound streaming: few query rows meet a long K/V.  One workgroup per (batch, kv head, split of
// the L cached rows) serves every query row that reads that kv head (rep = nh / nkv query heads times Tq queries), so each
// K/V byte leaves HBM once per step.  Each key row is read by hd/8 lanes with 16-byte loads straight into VGPRs; scores are
// reduced across those lanes with DPP, the softmax is online (fp32, exp2 with log2(e) folded in), and each split writes its
// (max, sum, accumulator) partials to a workspace that a second launch combines in split order.  No atomics: for one
// problem the bits do not change from launch to launch, nor with the cache capacity.
#include "oq_common.h"
#include "oq_quant_dev.h"
#include "oq_kv_dev.h"

namespace {

// ---- KV append: q [bs,Tq,nh,hd], k / v [bs,Tq,nkv,hd] -> rotated q (q_out), rotated k (cache rows past.., and k_out),
//      plain v (cache, and v_out).  One work item = 8 elements of a head's first half and the 8 partners of its second half.
//      QUANT (W4A4 packed blocks): the rotation runs on the fp32 inputs, then the per-(token, head) asymmetric quantiser over
//      hd (quantize/quantizer.py:122-147, oq_quant_dev.h arithmetic) on the fp32 result.  The hd / 16 work items of one
//      (token, head) are consecutive lanes of one wave, so min / max reduce with DPP inside that lane group.  The plain
//      append is the TIN == T, QUANT = false instantiation: it carries none of the quantiser.  Cache pointers may be NULL
//      (no-cache forward: q_out / k_out / v_out only); so may k_out / v_out. ------------------------------------------------
struct AppendP {
    const void *q, *k, *v;
    void *q_out, *k_out, *v_out, *kc, *vc;
    int64_t bs, Tq;
    int nh, nkv, hd;
    int64_t cap, past;
    const float *cs, *sn;
    int64_t P;
    const int64_t* pos;
    int64_t pos_bs;
    int nbits;
    float inv_q;
    // code destination (CODES instantiations): 4-bit rows of hd / 2 bytes, dim d in nibble d % 8 of the little-endian
    // 32-bit word d / 8, or 8-bit rows of hd bytes, dim d in byte d; and one (scale, rounded zero-point) pair per row;
    // value = (code - zp) * scale
    uint8_t *k_codes, *v_codes;
    float *k_meta, *v_meta;
    // RAGGED instantiations: the rows before this step, per sequence, int32 [bs] on the device (`past` is not read)
    const int32_t* lens;
    // PAGED instantiations: where logical row lens[b] + t lives (cap = max_pages * PS)
    PageMap pm;
};

// RAGGED: sequence b's row t goes to cache row lens[b] + t (and rotates at that position when pos == NULL).  The host cannot
// see lens, so the kernel guards the range itself: a row outside [0, cap) is not stored to the cache / codes / meta (skipped,
// never clamped onto another row); its q_out / k_out / v_out rows are written like any other.
// PAGED (a form of RAGGED): that logical row goes through the page table; a row whose table entry is outside [0, num_pages)
// is skipped in the same way (the entry of a row outside [0, cap) is not read).
// CODES: 0 (float rows), 4 or 8, the width of the codes stored.  CODES == 8 (weight-only blocks; QUANT is set): the q slot takes
// the plain path, and the k / v slots pass the 8-bit asymmetric quantiser with the row range widened to contain zero (zp in
// [0, 255]); a row whose scale comes out as 0 (all zeros) is stored as codes 0 under meta (0, 0) and reads back as zeros.
template <typename TIN, typename T, bool QUANT, int CODES, bool RAGGED, bool PAGED>
__global__ void __launch_bounds__(256) kv_append_kernel(AppendP p) {
    static_assert(RAGGED || !PAGED, "paged storage is always ragged");
    const int hd = p.hd, nh = p.nh, nkv = p.nkv;
    const int64_t Tq = p.Tq, cap = p.cap;
    int64_t past = p.past;
    const TIN* q = (const TIN*)p.q;
    const TIN* k = (const TIN*)p.k;
    const TIN* v = (const TIN*)p.v;
    T *q_out = (T*)p.q_out, *k_out = (T*)p.k_out, *v_out = (T*)p.v_out, *kc = (T*)p.kc, *vc = (T*)p.vc;
    const int half = hd / 2, hv = hd / 16;
    const int cbytes = CODES == 8 ? hd : half;                       // bytes of a code row
    const int nslot = nh + 2 * nkv;
    const int64_t n = p.bs * Tq * nslot * hv;
    for (int64_t it = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; it < n; it += (int64_t)gridDim.x * blockDim.x) {
        const int d0 = (int)(it % hv) * 8;
        int64_t r = it / hv;
        const int slot = (int)(r % nslot);
        r /= nslot;
        const int64_t t = r % Tq, b = r / Tq;
        bool fits = true;
        int64_t page = 0;
        if constexpr (RAGGED) {
            past = p.lens[b];
            fits = past + t >= 0 && past + t < cap;
        }
        if constexpr (PAGED) {
            if (fits) {
                page = p.pm.table[b * p.pm.max_pages + ((past + t) >> p.pm.lg)];
                fits = page >= 0 && page < p.pm.num_pages;
            }
            if (!fits) page = 0;
        }
        // the buffer row of kv head h that this step row goes to
        auto crow = [&](int h) -> int64_t {
            if constexpr (PAGED) return ((page * nkv + h) << p.pm.lg) + ((past + t) & ((int64_t(1) << p.pm.lg) - 1));
            else return (b * nkv + h) * cap + past + t;
        };
        const TIN* src;
        T* dst;
        T* dst2;
        uint8_t* cdst = nullptr;
        float* mdst = nullptr;
        bool rot = p.cs != nullptr;
        if (slot < nh) {
            src = q + ((b * Tq + t) * nh + slot) * hd;
            dst = q_out + ((b * Tq + t) * nh + slot) * hd;
            dst2 = nullptr;
        } else if (slot < nh + nkv) {
            const int h = slot - nh;
            src = k + ((b * Tq + t) * nkv + h) * hd;
            dst = kc && fits ? kc + crow(h) * hd : nullptr;
            dst2 = k_out ? k_out + ((b * Tq + t) * nkv + h) * hd : nullptr;
            if constexpr (CODES != 0) {
                cdst = fits ? p.k_codes + crow(h) * cbytes : nullptr;
                mdst = p.k_meta + crow(h) * 2;
            }
        } else {
            const int h = slot - nh - nkv;
            src = v + ((b * Tq + t) * nkv + h) * hd;
            dst = vc && fits ? vc + crow(h) * hd : nullptr;
            dst2 = v_out ? v_out + ((b * Tq + t) * nkv + h) * hd : nullptr;
            if constexpr (CODES != 0) {
                cdst = fits ? p.v_codes + crow(h) * cbytes : nullptr;
                mdst = p.v_meta + crow(h) * 2;
            }
            rot = false;
        }
        float a[8], c[8];
        Vec8<TIN>::load(src + d0, a);
        Vec8<TIN>::load(src + half + d0, c);
        if (rot) {
            // positions outside [0, P) are clamped to the table, never read out of bounds (the host sizes P >= past + Tq)
            int64_t ps = p.pos ? p.pos[b * p.pos_bs + t] : past + t;
            ps = ps < 0 ? 0 : (ps >= p.P ? p.P - 1 : ps);
            float c1[8], s1[8], c2[8], s2[8], oa[8], ob[8];
            Vec8<float>::load(p.cs + ps * hd + d0, c1);
            Vec8<float>::load(p.sn + ps * hd + d0, s1);
            Vec8<float>::load(p.cs + ps * hd + half + d0, c2);
            Vec8<float>::load(p.sn + ps * hd + half + d0, s2);
            oq_rope_fwd8(a, c, c1, s1, c2, s2, oa, ob);
#pragma unroll
            for (int i = 0; i < 8; ++i) { a[i] = oa[i]; c[i] = ob[i]; }
        }
        if constexpr (CODES == 8) {
            // every lane of the (token, head) group reduces; the q slot then leaves its values alone
            float hi = 0.f, lo = 0.f, bad = 0.f;                    // the range contains zero
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                hi = fmaxf(hi, fmaxf(a[i], c[i]));
                lo = fminf(lo, fminf(a[i], c[i]));
                if (a[i] != a[i] || c[i] != c[i]) bad = 1.f;
            }
            hi = wave_max(hi, hv);
            lo = wave_min(lo, hv);
            bad = wave_max(bad, hv);
            if (slot >= nh) {
                if (bad != 0.f) { hi = NAN; lo = NAN; }
                float inv_s = 0.f;
                const QP qp = make_qp(hi, lo, false, 0.f, 0.f, 8, 0, p.inv_q, &inv_s);
                const bool zero = qp.s == 0.f;                      // an all-zero row (or a range that underflows): exact zeros
                const bool finite = fabsf(qp.s) <= 3.4028234663852886e38f;
                const bool regular = !zero && finite && bad == 0.f && fabsf(inv_s) <= 3.4028234663852886e38f;
                float ca[8], cc[8];                                 // the lane's 16 codes
                float nan_row = finite ? 0.f : 1.f;                 // a NaN / inf element or an overflowing range
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float& x = i < 8 ? a[i] : c[i - 8];
                    float code = 0.f;
                    if (regular) {
                        float tq;
                        const float rq = rne_div(x, qp.s, inv_s, &tq);
                        code = __builtin_amdgcn_fmed3f(rq + qp.z, 0.f, 255.f);
                        x = (code - qp.z) * qp.s;
                    } else if (zero) {
                        x = 0.f;
                    } else {                                        // a subnormal scale: the exact division
                        float u = rne_ste(x / qp.s) + qp.z;
                        u = (u != u) ? u : fminf(fmaxf(u, 0.f), 255.f);
                        x = (u - qp.z) * qp.s;
                        if (u != u) nan_row = 1.f;
                        else code = u;
                    }
                    (i < 8 ? ca[i] : cc[i - 8]) = code;
                }
                nan_row = wave_max(nan_row, hv);
                if (nan_row != 0.f) {                               // codes 0 under a NaN scale, as the 4-bit rows
#pragma unroll
                    for (int i = 0; i < 8; ++i) { a[i] = NAN; c[i] = NAN; ca[i] = 0.f; cc[i] = 0.f; }
                }
                if (cdst) {
                    oq_store_codes8(reinterpret_cast<int8_t*>(cdst + d0), ca, false);
                    oq_store_codes8(reinterpret_cast<int8_t*>(cdst + half + d0), cc, false);
                    if (d0 == 0) *reinterpret_cast<f32x2*>(mdst) = f32x2{nan_row != 0.f ? NAN : qp.s, zero ? 0.f : qp.z};
                }
            }
        } else if constexpr (QUANT) {
            const float Q = (float)((1 << p.nbits) - 1);
            float hi = -INFINITY, lo = INFINITY, bad = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                hi = fmaxf(hi, fmaxf(a[i], c[i]));
                lo = fminf(lo, fminf(a[i], c[i]));
                if (a[i] != a[i] || c[i] != c[i]) bad = 1.f;
            }
            hi = wave_max(hi, hv);
            lo = wave_min(lo, hv);
            bad = wave_max(bad, hv);
            if (bad != 0.f) { hi = NAN; lo = NAN; }
            float inv_s = 0.f;
            const QP qp = make_qp(hi, lo, false, 0.f, 0.f, p.nbits, 0, p.inv_q, &inv_s);
            // (a subnormal scale whose reciprocal overflows takes the exact-division branch too: x * inf would turn a zero
            // element into NaN)
            const bool regular = qp.s != 0.f && fabsf(qp.s) <= 3.4028234663852886e38f && bad == 0.f &&
                                 fabsf(inv_s) <= 3.4028234663852886e38f;
            uint32_t wa = 0, wc = 0;            // CODES: the lane's two words of 8 codes
            float nan_row = 0.f;                // CODES: an element of the row came out as NaN
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float& x = i < 8 ? a[i] : c[i - 8];
                if (regular) {
                    float tq;
                    const float rq = rne_div(x, qp.s, inv_s, &tq);
                    const float code = __builtin_amdgcn_fmed3f(rq + qp.z, 0.f, Q);
                    x = (code - qp.z) * qp.s;
                    if constexpr (CODES != 0) (i < 8 ? wa : wc) |= (uint32_t)code << (4 * (i & 7));
                } else {
                    float u = rne_ste(x / qp.s) + qp.z;
                    u = (u != u) ? u : fminf(fmaxf(u, 0.f), Q);
                    x = (u - qp.z) * qp.s;
                    if constexpr (CODES != 0) {
                        if (u != u) nan_row = 1.f;
                        else (i < 8 ? wa : wc) |= (uint32_t)u << (4 * (i & 7));
                    }
                }
            }
            if constexpr (CODES != 0) {
                // a row of scale 0, inf or NaN (constant rows, overflowing ranges, NaN inputs) comes out of the branch above as
                // NaN in every element: codes 0 under a NaN scale hold exactly that.  Every other row has no NaN at all.
                nan_row = wave_max(nan_row, hv);
                if (cdst) {
                    uint32_t* w = reinterpret_cast<uint32_t*>(cdst);
                    w[d0 / 8] = nan_row != 0.f ? 0u : wa;
                    w[(half + d0) / 8] = nan_row != 0.f ? 0u : wc;
                    if (d0 == 0) *reinterpret_cast<f32x2*>(mdst) = f32x2{nan_row != 0.f ? NAN : qp.s, qp.z};
                }
            }
        }
        if (dst) {
            Vec8<T>::store(dst + d0, a);
            Vec8<T>::store(dst + half + d0, c);
        }
        if (dst2) {
            Vec8<T>::store(dst2 + d0, a);
            Vec8<T>::store(dst2 + half + d0, c);
        }
    }
}

template <typename TIN, typename T, bool QUANT, int CODES, bool RAGGED, bool PAGED>
void launch_append(const AppendP& p, hipStream_t st) {
    const int64_t n = p.bs * p.Tq * (p.nh + 2 * p.nkv) * (p.hd / 16);
    const int64_t grid = (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096;
    hipLaunchKernelGGL((kv_append_kernel<TIN, T, QUANT, CODES, RAGGED, PAGED>), dim3(grid), dim3(256), 0, st, p);
}

// The checks, the grid and the dtype dispatch both ABI entry points share (fn: the entry point's name for the messages).
// The caller has checked what is its own: which pointers it requires, head_dim, nbits and the dtype pairs it admits.
template <bool QUANT, int CODES = 0, bool RAGGED = false, bool PAGED = false>
int kv_append(const char* fn, const AppendP& p, int in_dtype, int dtype, void* stream) {
    OQ_CHECK_ARG(!p.q || p.q_out, "%s: q without q_out", fn);
    OQ_CHECK_ARG(p.bs > 0 && p.Tq > 0 && p.nkv > 0 && p.nh >= 0 && (p.q || p.nh == 0), "%s: bad shape", fn);
    if constexpr (RAGGED) {
        OQ_CHECK_ARG(p.lens && (uintptr_t)p.lens % 4 == 0 && p.cap >= 0, "%s: lens (int32 [bs] on the device), cap >= 0", fn);
        OQ_CHECK_ARG(PAGED == (p.pm.table != nullptr), "%s: page table", fn);
    } else {
        OQ_CHECK_ARG(!(p.kc || p.k_codes) || (p.past >= 0 && p.past + p.Tq <= p.cap), "%s: rows [%lld, %lld) exceed the capacity %lld", fn,
                     (long long)p.past, (long long)(p.past + p.Tq), (long long)p.cap);
    }
    OQ_CHECK_ARG(!p.cs == !p.sn, "%s: cos and sin go together", fn);
    OQ_CHECK_ARG(!p.cs || (p.P > 0 && oq_aligned16(p.cs) && oq_aligned16(p.sn)), "%s: cos/sin tables must be 16-byte aligned, P > 0", fn);
    OQ_CHECK_ARG(p.pos_bs >= 0, "%s: pos_bstride", fn);
    const void* ptrs[] = {p.q, p.k, p.v, p.q_out, p.k_out, p.v_out, p.kc, p.vc, p.k_codes, p.v_codes, p.k_meta, p.v_meta};
    for (const void* ptr : ptrs) OQ_CHECK_ARG(!ptr || oq_aligned16(ptr), "%s: tensors must be 16-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == OQ_F32 && in_dtype == OQ_F32) {
        launch_append<float, float, QUANT, CODES, RAGGED, PAGED>(p, st);
    } else if (dtype == OQ_BF16 && in_dtype == OQ_BF16) {
        launch_append<bf16_t, bf16_t, QUANT, CODES, RAGGED, PAGED>(p, st);
    } else if constexpr (QUANT) {
        launch_append<float, bf16_t, true, CODES, RAGGED, PAGED>(p, st);      // f32 -> bf16: the only other pair the quantising entry admits
    } else {
        oq_set_error("%s: dtype %d unsupported", fn, dtype);
        return OQ_E_UNSUPPORTED;
    }
    OQ_CHECK_LAUNCH(fn);
    return OQ_OK;
}

// ---- decode attention ----------------------------------------------------------------------------------------------------
constexpr int DEC_THREADS = 256;
inline int dec_qb(int64_t R) { return R >= 8 ? 8 : (R >= 3 ? 4 : (R == 2 ? 2 : 1)); }

__device__ __forceinline__ float ld_mask(const void* m, int mdt, int64_t i) {
    if (mdt == OQ_F32) return reinterpret_cast<const float*>(m)[i];
    if (mdt == OQ_BF16) return (float)reinterpret_cast<const bf16_t*>(m)[i];
    return (float)reinterpret_cast<const f16_t*>(m)[i];
}

// ---- where the cached rows come from: the kernel's K / V argument and its per-row loads ---------------------------------
// A policy gives DPL (dims of a row one lane holds; HD / DPL lanes make a lane group), SCALED (a row carries a scale that
// multiplies its score and its probability once per row), at(b, kvh, nkv, cap, d0) (the lane's view of one (b, kv head)),
// load(k, v, j) of that view's logical row j into Row registers -- false: the row has no storage and counts as invisible, which
// only a paged cache can say -- and Row::unpack / Row::scale.
template <typename T, int HD>
struct FloatKV {                        // [bs, nkv, cap, HD] of T: 16-byte loads, 8 dims per lane
    static constexpr int DPL = 8;
    static constexpr bool SCALED = false;
    static constexpr bool PAGED = false;
    const T *k, *v;
    struct Row {
        Raw8<T> r;
        __device__ __forceinline__ void unpack(float (&o)[8]) const { r.unpack(o); }
        __device__ __forceinline__ float scale() const { return 1.f; }
    };
    __device__ __forceinline__ FloatKV at(int64_t b, int kvh, int nkv, int64_t cap, int d0) const {
        const int64_t row0 = (b * nkv + kvh) * cap;
        return {k + row0 * HD + d0, v + row0 * HD + d0};
    }
    __device__ __forceinline__ bool load(Row& kr, Row& vr, int64_t j) const {
        kr.r.load(k + j * HD);
        vr.r.load(v + j * HD);
        return true;
    }
};

// 4-bit code cache: rows of HD / 2 code bytes (dim d in nibble d % 8 of word d / 8) plus one (scale, zero-point) pair, value
// = (code - zp) * scale.  A lane holds DPL dims: DPL / 8 words, one 4- or 8-byte load.  unpack gives code - zp (exact: small
// integers held in floats, or a NaN zero-point); the scale is applied per row, so scores are s_k * sum q (c - z_k) and the PV
// term (p s_v) (c - z_v).
template <int HD, int DPL_>
struct CodeKV {
    static constexpr int DPL = DPL_;
    static constexpr bool SCALED = true;
    static constexpr bool PAGED = false;
    static constexpr int W = DPL / 8;
    const uint8_t *k, *v;
    const f32x2 *km, *vm;
    struct Row {
        uint32_t w[W];
        f32x2 m;
        __device__ __forceinline__ void load(const uint8_t* p) {
            if constexpr (W == 2) {
                typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
                const u32x2 r = *reinterpret_cast<const u32x2*>(p);
                w[0] = r[0];
                w[1] = r[1];
            } else {
                w[0] = *reinterpret_cast<const uint32_t*>(p);
            }
        }
        __device__ __forceinline__ void unpack(float (&o)[DPL]) const {
#pragma unroll
            for (int n = 0; n < W; ++n) {
                const uint32_t lo = w[n] & 0x0F0F0F0Fu, hi = (w[n] >> 4) & 0x0F0F0F0Fu;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    o[8 * n + 2 * i] = (float)((lo >> (8 * i)) & 0xFFu) - m[1];          // v_cvt_f32_ubyte<i>
                    o[8 * n + 2 * i + 1] = (float)((hi >> (8 * i)) & 0xFFu) - m[1];
                }
            }
        }
        __device__ __forceinline__ float scale() const { return m[0]; }
    };
    __device__ __forceinline__ CodeKV at(int64_t b, int kvh, int nkv, int64_t cap, int d0) const {
        const int64_t row0 = (b * nkv + kvh) * cap;
        return {k + row0 * (HD / 2) + d0 / 2, v + row0 * (HD / 2) + d0 / 2, km + row0, vm + row0};
    }
    __device__ __forceinline__ bool load(Row& kr, Row& vr, int64_t j) const {
        kr.load(k + j * (HD / 2));
        vr.load(v + j * (HD / 2));
        kr.m = km[j];
        vr.m = vm[j];
        return true;
    }
};

// 8-bit code cache: rows of HD code bytes (dim d in byte d) plus the (scale, zero-point) pair, value = (code - zp) * scale with
// zp in [0, 255].  A lane holds DPL dims: DPL / 4 words, one 8- or 16-byte load; unpack and scale are CodeKV's contract.
template <int HD, int DPL_>
struct Code8KV {
    static constexpr int DPL = DPL_;
    static constexpr bool SCALED = true;
    static constexpr bool PAGED = false;
    static constexpr int W = DPL / 4;
    const uint8_t *k, *v;
    const f32x2 *km, *vm;
    struct Row {
        uint32_t w[W];
        f32x2 m;
        __device__ __forceinline__ void load(const uint8_t* p) {
            if constexpr (W == 4) {
                const u32x4 r = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
                for (int n = 0; n < 4; ++n) w[n] = r[n];
            } else {
                typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
                const u32x2 r = *reinterpret_cast<const u32x2*>(p);
                w[0] = r[0];
                w[1] = r[1];
            }
        }
        __device__ __forceinline__ void unpack(float (&o)[DPL]) const {
#pragma unroll
            for (int n = 0; n < W; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) o[4 * n + i] = (float)((w[n] >> (8 * i)) & 0xFFu) - m[1];      // v_cvt_f32_ubyte<i>
        }
        __device__ __forceinline__ float scale() const { return m[0]; }
    };
    __device__ __forceinline__ Code8KV at(int64_t b, int kvh, int nkv, int64_t cap, int d0) const {
        const int64_t row0 = (b * nkv + kvh) * cap;
        return {k + row0 * HD + d0, v + row0 * HD + d0, km + row0, vm + row0};
    }
    __device__ __forceinline__ bool load(Row& kr, Row& vr, int64_t j) const {
        kr.load(k + j * HD);
        vr.load(v + j * HD);
        kr.m = km[j];
        vr.m = vm[j];
        return true;
    }
};

// Any of the three over a page pool [num_pages, nkv, PS, ...]: the same rows, registers and arithmetic, found through the
// page table.  at() moves the inner view to this kv head's rows of page 0 and the table to sequence b's row; load() reads
// the lane group's own table entry (a vector load: the groups of a wave hold different rows j) and then the row, PS
// contiguous rows per (page, kv head).  Callers keep j below the bound L <= max_pages * PS, so the entry exists.
template <typename Inner>
struct PagedKV {
    static constexpr int DPL = Inner::DPL;
    static constexpr bool SCALED = Inner::SCALED;
    static constexpr bool PAGED = true;
    using Row = typename Inner::Row;
    Inner in;
    PageMap pm;
    int64_t page_rows;                  // rows from one page to the next: nkv << lg (set by at())
    __device__ __forceinline__ PagedKV at(int64_t b, int kvh, int nkv, int64_t, int d0) const {
        return {in.at(0, kvh, nkv, int64_t(1) << pm.lg, d0), {pm.table + b * pm.max_pages, pm.max_pages, pm.num_pages, pm.lg},
                (int64_t)nkv << pm.lg};
    }
    __device__ __forceinline__ bool load(Row& kr, Row& vr, int64_t j) const {
        const int64_t page = pm.table[j >> pm.lg];
        if (page < 0 || page >= pm.num_pages) return false;
        return in.load(kr, vr, page * page_rows + (j & ((int64_t(1) << pm.lg) - 1)));
    }
};

// Split kernel: grid (ns, nkv, bs).  Lane group `grp` (HD / DPL lanes) handles rows j0 + grp, j0 + grp + G, ... of the split,
// U rows in flight; query rows are processed QB at a time (rows r = t*rep + i of this kv head).  Workspace per
// (b, kv head, split, r): [m, l, acc[HD]] with m in the log2 domain.
// RAGGED: every sequence has its own length.  lens[b] rows precede this step (negative: 0; clamped to L - Tq, so that a length
// beyond the bound the host planned with can neither read past row L nor leave a query without a key), L is the host's upper
// bound of lens[b] + Tq (the split plan depends on it alone) and query row t sees rows j <= lens[b] + t: causal within the
// step, no mask tensor.  Rows >= lens[b] + Tq are never loaded; a split that starts there writes (m, l) = (-inf, 0) partials,
// which the combine kernel weighs with 0.  lens[b] is the same for the whole workgroup, so the trip counts stay uniform.  With
// every lens[b] == L - Tq and Tq == 1 the loops and the order of every sum are those of the plain instantiation.
// A paged cache (PagedKV<>, RAGGED only) changes where load() finds row j and nothing else: the same loops and sums, hence the
// bits of the contiguous cache holding the same rows, for every page size and page order.
template <typename T, int HD, int QB, typename KV, bool RAGGED>
__global__ void __launch_bounds__(DEC_THREADS) attn_decode_kernel(const T* q, const KV kv_all, float* ws, int64_t Tq, int nh,
                                                                  int nkv, int64_t cap, int64_t L, float scale, const void* mask,
                                                                  int mdt, int64_t m_bs, int64_t m_ld, int ns,
                                                                  const int32_t* lens) {
    constexpr int DPL = KV::DPL;
    constexpr int LPK = HD / DPL;
    constexpr int GPW = 64 / LPK;
    constexpr int G = GPW * (DEC_THREADS / 64);
    constexpr int U = QB >= 8 ? 2 : 4;
    const float log2e = 1.4426950408889634f, lowest = -3.4028234663852886e38f;
    __shared__ float red_m[G], red_l[G];
    __shared__ float red_acc[G][HD];

    const int split = blockIdx.x, kvh = blockIdx.y;
    const int64_t b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63;
    const int grp = (tid >> 6) * GPW + lane / LPK, d0 = (lane % LPK) * DPL;
    const int rep = nh / nkv;
    const int64_t R = (int64_t)rep * Tq;
    const int64_t chunk = (L + ns - 1) / ns;
    const int64_t j0 = split * chunk;
    int64_t j1 = (j0 + chunk < L) ? j0 + chunk : L;
    int64_t len = 0;
    if constexpr (RAGGED) {
        len = lens[b];
        len = len < 0 ? 0 : (len > L - Tq ? L - Tq : len);
        if (j1 > len + Tq) j1 = len + Tq;
    }
    const KV kv = kv_all.at(b, kvh, nkv, cap, d0);
    float* wsb = ws + ((b * nkv + kvh) * ns + split) * R * (HD + 2);
    const float zs = scale * log2e;

    for (int64_t r0 = 0; r0 < R; r0 += QB) {
        float qv[QB][DPL], m[QB], l[QB], acc[QB][DPL];
        int64_t moff[QB];
        int64_t vis[QB];                                            // RAGGED: the last cache row the query row sees
#pragma unroll
        for (int rr = 0; rr < QB; ++rr) {
            const int64_t r = r0 + rr < R ? r0 + rr : R - 1;        // padding rows repeat the last one (never stored)
            const int64_t t = r / rep;
            const T* qp = q + ((b * Tq + t) * nh + (int64_t)kvh * rep + (r % rep)) * HD + d0;
#pragma unroll
            for (int n = 0; n < DPL / 8; ++n) {
                float t8[8];
                Vec8<T>::load(qp + 8 * n, t8);
#pragma unroll
                for (int i = 0; i < 8; ++i) qv[rr][8 * n + i] = t8[i];
            }
            moff[rr] = b * m_bs + t * m_ld;
            vis[rr] = len + t;
            m[rr] = -INFINITY;
            l[rr] = 0.f;
#pragma unroll
            for (int i = 0; i < DPL; ++i) acc[rr][i] = 0.f;
        }
        // the trip count is uniform over the workgroup; rows past j1 are masked per lane group (and never loaded)
        for (int64_t jb = j0; jb < j1; jb += (int64_t)G * U) {
            typename KV::Row kr[U], vr[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t j = jb + u * G + grp;
                ok[u] = j < j1 && kv.load(kr[u], vr[u], j);      // (a paged cache: and the row's page exists)
            }
            float z[U][QB];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float kf[DPL];
                if (ok[u]) kr[u].unpack(kf);
                else {
#pragma unroll
                    for (int i = 0; i < DPL; ++i) kf[i] = 0.f;
                }
                const int64_t j = jb + u * G + grp;
#pragma unroll
                for (int rr = 0; rr < QB; ++rr) {
                    float s = 0.f;
#pragma unroll
                    for (int i = 0; i < DPL; ++i) s = __builtin_fmaf(qv[rr][i], kf[i], s);
                    s = wave_sum(s, LPK);                       // every lane of the group holds q . k_j
                    if constexpr (KV::SCALED) s *= ok[u] ? kr[u].scale() : 0.f;
                    float zz;
                    if (!RAGGED && mask) {
                        const float mv = ok[u] ? ld_mask(mask, mdt, moff[rr] + j) : 0.f;
                        zz = fmaxf((s * scale + mv) * log2e, lowest);   // max(z, -FLT_MAX) as oq_softmax_fwd, in log2 units
                    } else {
                        zz = s * zs;
                    }
                    z[u][rr] = (RAGGED ? ok[u] && j <= vis[rr] : ok[u]) ? zz : -INFINITY;
                }
            }
#pragma unroll
            for (int rr = 0; rr < QB; ++rr) {
                float mx = m[rr];
#pragma unroll
                for (int u = 0; u < U; ++u) mx = fmaxf(mx, z[u][rr]);
                // (a lane group with no row yet keeps m = -inf: no rescale)
                const float c = mx == -INFINITY ? 1.f : __builtin_amdgcn_exp2f(m[rr] - mx);
                m[rr] = mx;
                l[rr] *= c;
#pragma unroll
                for (int i = 0; i < DPL; ++i) acc[rr][i] *= c;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool sees = RAGGED ? ok[u] && jb + u * G + grp <= vis[rr] : ok[u];
                    z[u][rr] = sees ? __builtin_amdgcn_exp2f(z[u][rr] - mx) : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float vf[DPL];
                if (ok[u]) vr[u].unpack(vf);
                else {
#pragma unroll
                    for (int i = 0; i < DPL; ++i) vf[i] = 0.f;
                }
#pragma unroll
                for (int rr = 0; rr < QB; ++rr) {
                    l[rr] += z[u][rr];
                    float pw = z[u][rr];
                    if constexpr (KV::SCALED) pw *= ok[u] ? vr[u].scale() : 0.f;
#pragma unroll
                    for (int i = 0; i < DPL; ++i) acc[rr][i] = __builtin_fmaf(pw, vf[i], acc[rr][i]);
                }
            }
        }
        // combine the G lane groups of the workgroup in group order, one query row at a time
#pragma unroll
        for (int rr = 0; rr < QB; ++rr) {
            const int64_t r = r0 + rr;
            if (r >= R) break;                                       // uniform over the workgroup
            if (lane % LPK == 0) red_m[grp] = m[rr];
            __syncthreads();
            float M = -INFINITY;
            for (int g = 0; g < G; ++g) M = fmaxf(M, red_m[g]);
            const float w = m[rr] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[rr] - M);
#pragma unroll
            for (int i = 0; i < DPL; ++i) red_acc[grp][d0 + i] = acc[rr][i] * w;
            if (lane % LPK == 0) red_l[grp] = l[rr] * w;
            __syncthreads();
            float* wr = wsb + r * (HD + 2);
            if (tid < HD) {
                float s = 0.f;
                for (int g = 0; g < G; ++g) s += red_acc[g][tid];
                wr[2 + tid] = s;
            } else if (tid == HD) {
                float s = 0.f;
                for (int g = 0; g < G; ++g) s += red_l[g];
                wr[0] = M;
                wr[1] = s;
            }
            __syncthreads();
        }
    }
}

struct DecP {
    const void* q;
    void* o;
    float* ws;
    int64_t bs, Tq;
    int nh, nkv;
    int64_t cap, L;
    float scale;
    const void* mask;
    int mdt;
    int64_t m_bs, m_ld;
    int ns;
    const int32_t* lens;                // per-sequence lengths (the RAGGED instantiations), or NULL
    PageMap pm;                         // table != NULL: the buffers are page pools (PagedKV<>; lens required)
};

template <typename T, int HD, int QB, typename KV>
void launch_decode(const DecP& p, const KV& kv, hipStream_t st) {
    const dim3 grid(p.ns, p.nkv, p.bs);
    if constexpr (KV::PAGED)
        hipLaunchKernelGGL((attn_decode_kernel<T, HD, QB, KV, true>), grid, dim3(DEC_THREADS), 0, st, (const T*)p.q, kv, p.ws, p.Tq,
                           p.nh, p.nkv, p.cap, p.L, p.scale, nullptr, 0, 0, 0, p.ns, p.lens);
    else if (p.lens)
        hipLaunchKernelGGL((attn_decode_kernel<T, HD, QB, KV, true>), grid, dim3(DEC_THREADS), 0, st, (const T*)p.q, kv, p.ws, p.Tq,
                           p.nh, p.nkv, p.cap, p.L, p.scale, nullptr, 0, 0, 0, p.ns, p.lens);
    else
        hipLaunchKernelGGL((attn_decode_kernel<T, HD, QB, KV, false>), grid, dim3(DEC_THREADS), 0, st, (const T*)p.q, kv, p.ws, p.Tq,
                           p.nh, p.nkv, p.cap, p.L, p.scale, p.mask, p.mdt, p.m_bs, p.m_ld, p.ns, nullptr);
    const int64_t rows = p.bs * (int64_t)p.nh * p.Tq;
    hipLaunchKernelGGL((attn_decode_combine_kernel<T, HD>), dim3(rows), dim3(HD), 0, st, (const float*)p.ws, (T*)p.o, p.Tq, p.nh,
                       p.nkv, p.ns);
}

template <typename T, int HD, typename KV>
void launch_decode_qb(int qb, const DecP& p, const KV& kv, hipStream_t st) {
    switch (qb) {
        case 1: launch_decode<T, HD, 1>(p, kv, st); break;
        case 2: launch_decode<T, HD, 2>(p, kv, st); break;
        case 4: launch_decode<T, HD, 4>(p, kv, st); break;
        default: launch_decode<T, HD, 8>(p, kv, st); break;
    }
}

template <typename T, int HD>
void launch_decode_float(int qb, const DecP& p, const void* kc, const void* vc, hipStream_t st) {
    const FloatKV<T, HD> kv{(const T*)kc, (const T*)vc};
    if (p.pm.table) return launch_decode_qb<T, HD>(qb, p, PagedKV<FloatKV<T, HD>>{kv, p.pm, 0}, st);
    launch_decode_qb<T, HD>(qb, p, kv, st);
}

// One or two query rows per pass leave the registers for 16 dims per lane (4-bit: 8-byte loads, 8-bit: 16-byte loads); four or
// eight keep 8 dims.  CKV: CodeKV or Code8KV.
template <typename T, int HD, template <int, int> class CKV>
void launch_decode_codes(int qb, const DecP& p, const void* kc, const void* vc, const float* km, const float* vm, hipStream_t st) {
    const CKV<HD, 16> wide{(const uint8_t*)kc, (const uint8_t*)vc, (const f32x2*)km, (const f32x2*)vm};
    const CKV<HD, 8> narrow{wide.k, wide.v, wide.km, wide.vm};
    if (p.pm.table) {
        if (qb <= 2) launch_decode_qb<T, HD>(qb, p, PagedKV<CKV<HD, 16>>{wide, p.pm, 0}, st);
        else launch_decode_qb<T, HD>(qb, p, PagedKV<CKV<HD, 8>>{narrow, p.pm, 0}, st);
    } else if (qb <= 2) {
        launch_decode_qb<T, HD>(qb, p, wide, st);
    } else {
        launch_decode_qb<T, HD>(qb, p, narrow, st);
    }
}

// ---- what an entry point and its ragged form share: the entry's own checks, then kv_append<> / the decode launch.  lens ==
//      NULL: the uniform form (`past`, resp. L and the mask); else the ragged one (fn carries the entry point's name). ------------
int append_plain(const char* fn, const void* q, const void* k, const void* v, void* q_out, void* k_out, void* k_cache, void* v_cache,
                 int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap, int64_t past, const int32_t* lens,
                 const PageMap& pm, const float* cos, const float* sin, int64_t P, const int64_t* pos, int64_t pos_bstride,
                 void* stream) {
    OQ_CHECK_ARG(k && v && k_cache && v_cache, "%s: null pointer", fn);
    OQ_CHECK_ARG(hd > 0 && hd % 16 == 0, "%s: head_dim %d must be a multiple of 16", fn, hd);
    const AppendP p{q, k, v, q_out, k_out, nullptr, k_cache, v_cache, bs, Tq, nh, nkv, hd, cap, past, cos, sin, P, pos, pos_bstride,
                    0, 0.f, nullptr, nullptr, nullptr, nullptr, lens, pm};
    if (pm.table) return kv_append<false, 0, true, true>(fn, p, dtype, dtype, stream);
    return lens ? kv_append<false, 0, true>(fn, p, dtype, dtype, stream) : kv_append<false>(fn, p, dtype, dtype, stream);
}

int append_quant(const char* fn, const void* q, const void* k, const void* v, int in_dtype, void* q_out, void* k_out, void* v_out,
                 void* k_cache, void* v_cache, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap, int64_t past,
                 const int32_t* lens, const PageMap& pm, const float* cos, const float* sin, int64_t P, const int64_t* pos,
                 int64_t pos_bstride, int nbits, void* stream) {
    OQ_CHECK_ARG(k && v, "%s: null k / v", fn);
    OQ_CHECK_ARG(!k_cache == !v_cache, "%s: the k and v caches go together", fn);
    OQ_CHECK_ARG(k_cache || (k_out && v_out), "%s: no destination for k / v (caches or k_out / v_out)", fn);
    // (the DPP reduction over the hd / 16 lanes of a head needs a power-of-two lane group inside one row of 16)
    OQ_CHECK_ARG(hd == 64 || hd == 128, "%s: head_dim %d (64 or 128)", fn, hd);
    OQ_CHECK_ARG(nbits >= 2 && nbits <= 8, "%s: %d-bit head quantiser (2..8)", fn, nbits);
    OQ_CHECK_ARG(dtype == OQ_F32 || dtype == OQ_BF16, "%s: dtype %d (f32 or bf16)", fn, dtype);
    OQ_CHECK_ARG(in_dtype == OQ_F32 || in_dtype == dtype, "%s: input dtype %d (f32 or the output dtype)", fn, in_dtype);
    const AppendP p{q, k, v, q_out, k_out, v_out, k_cache, v_cache, bs, Tq, nh, nkv, hd, cap, past, cos, sin, P, pos, pos_bstride,
                    nbits, 1.0f / (float)((1 << nbits) - 1), nullptr, nullptr, nullptr, nullptr, lens, pm};
    if (pm.table) return kv_append<true, 0, true, true>(fn, p, in_dtype, dtype, stream);
    return lens ? kv_append<true, 0, true>(fn, p, in_dtype, dtype, stream) : kv_append<true>(fn, p, in_dtype, dtype, stream);
}

int append_codes(const char* fn, const void* q, const void* k, const void* v, int in_dtype, void* q_out, void* k_out, void* v_out,
                 void* k_codes, void* v_codes, float* k_meta, float* v_meta, int dtype, int64_t bs, int64_t Tq, int nh, int nkv,
                 int hd, int64_t cap, int64_t past, const int32_t* lens, const PageMap& pm, const float* cos, const float* sin,
                 int64_t P, const int64_t* pos, int64_t pos_bstride, int cbits, int nbits, void* stream) {
    OQ_CHECK_ARG(k && v && k_codes && v_codes && k_meta && v_meta, "%s: null pointer", fn);
    OQ_CHECK_ARG(hd == 64 || hd == 128, "%s: head_dim %d (64 or 128)", fn, hd);
    OQ_CHECK_ARG(nbits == cbits, "%s: %d-bit codes (%d)", fn, nbits, cbits);
    OQ_CHECK_ARG(dtype == OQ_F32 || dtype == OQ_BF16, "%s: dtype %d (f32 or bf16)", fn, dtype);
    OQ_CHECK_ARG(in_dtype == OQ_F32 || in_dtype == dtype, "%s: input dtype %d (f32 or the output dtype)", fn, in_dtype);
    OQ_CHECK_ARG(!k_out == !v_out, "%s: k_out and v_out go together", fn);
    const AppendP p{q, k, v, q_out, k_out, v_out, nullptr, nullptr, bs, Tq, nh, nkv, hd, cap, past, cos, sin, P, pos, pos_bstride,
                    nbits, cbits == 8 ? 1.0f / 255.0f : 1.0f / 15.0f, (uint8_t*)k_codes, (uint8_t*)v_codes, k_meta, v_meta, lens, pm};
    if (cbits == 8) {
        if (pm.table) return kv_append<true, 8, true, true>(fn, p, in_dtype, dtype, stream);
        return lens ? kv_append<true, 8, true>(fn, p, in_dtype, dtype, stream) : kv_append<true, 8>(fn, p, in_dtype, dtype, stream);
    }
    if (pm.table) return kv_append<true, 4, true, true>(fn, p, in_dtype, dtype, stream);
    return lens ? kv_append<true, 4, true>(fn, p, in_dtype, dtype, stream) : kv_append<true, 4>(fn, p, in_dtype, dtype, stream);
}

// codes (0, 4 or 8): k / v are the code buffers of a cache of that width and k_meta / v_meta its (scale, zero-point) pairs; 0: a
// float cache's buffers (no meta).  ragged: lens is required and there is no mask; L is then the bound.  pm.table: the buffers are page
// pools and cap = max_pages * page size (ragged only).
int decode(const char* fn, int codes, const void* q, const void* k, const void* v, const float* k_meta, const float* v_meta, void* o,
           int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap, int64_t L, const int32_t* lens, bool ragged,
           const PageMap& pm, float scale, const void* mask, int mask_dtype, int64_t mask_bstride, int64_t mask_ld, void* workspace,
           int64_t workspace_bytes, void* stream) {
    OQ_CHECK_ARG(q && k && v && o && workspace && (!codes || (k_meta && v_meta)) && (!ragged || lens), "%s: null pointer", fn);
    OQ_CHECK_ARG(hd == 64 || hd == 128, "%s: head_dim %d (64 or 128)", fn, hd);
    OQ_CHECK_ARG(bs > 0 && bs <= 65535 && nkv > 0 && nkv <= 65535 && nh > 0 && nh % nkv == 0, "%s: bad heads %d / %d or batch %lld", fn,
                 nh, nkv, (long long)bs);
    OQ_CHECK_ARG(Tq > 0 && L >= Tq && L <= cap, "%s: need 1 <= Tq (%lld) <= L (%lld) <= cap (%lld)", fn, (long long)Tq, (long long)L,
                 (long long)cap);
    OQ_CHECK_ARG(!mask || mask_dtype == OQ_F32 || mask_dtype == OQ_F16 || mask_dtype == OQ_BF16, "%s: mask dtype %d", fn, mask_dtype);
    OQ_CHECK_ARG(mask_bstride >= 0 && mask_ld >= 0, "%s: negative mask strides", fn);
    OQ_CHECK_ARG(oq_aligned16(q) && oq_aligned16(k) && oq_aligned16(v) && oq_aligned16(o) && oq_aligned16(workspace) &&
                     oq_aligned16(k_meta) && oq_aligned16(v_meta) && (uintptr_t)lens % 4 == 0,
                 "%s: q, o, the cache buffers and the workspace must be 16-byte aligned (lens: 4)", fn);
    const int64_t need = oq_attn_decode_workspace(bs, nh, nkv, Tq, L, hd);
    OQ_CHECK_ARG(workspace_bytes >= need, "%s: workspace %lld < %lld bytes", fn, (long long)workspace_bytes, (long long)need);
    const int qb = dec_qb((int64_t)(nh / nkv) * Tq);
    const DecP p{q, o, (float*)workspace, bs, Tq, nh, nkv, cap, L, scale, mask, mask_dtype, mask_bstride, mask_ld, dec_splits(bs, nkv, L),
                 lens, pm};
    hipStream_t st = (hipStream_t)stream;
    if (dtype != OQ_F32 && dtype != OQ_BF16) {
        oq_set_error("%s: dtype %d unsupported", fn, dtype);
        return OQ_E_UNSUPPORTED;
    }
    const bool f32 = dtype == OQ_F32;
    if (codes == 8) {
        if (f32 && hd == 64) launch_decode_codes<float, 64, Code8KV>(qb, p, k, v, k_meta, v_meta, st);
        else if (f32) launch_decode_codes<float, 128, Code8KV>(qb, p, k, v, k_meta, v_meta, st);
        else if (hd == 64) launch_decode_codes<bf16_t, 64, Code8KV>(qb, p, k, v, k_meta, v_meta, st);
        else launch_decode_codes<bf16_t, 128, Code8KV>(qb, p, k, v, k_meta, v_meta, st);
    } else if (codes) {
        if (f32 && hd == 64) launch_decode_codes<float, 64, CodeKV>(qb, p, k, v, k_meta, v_meta, st);
        else if (f32) launch_decode_codes<float, 128, CodeKV>(qb, p, k, v, k_meta, v_meta, st);
        else if (hd == 64) launch_decode_codes<bf16_t, 64, CodeKV>(qb, p, k, v, k_meta, v_meta, st);
        else launch_decode_codes<bf16_t, 128, CodeKV>(qb, p, k, v, k_meta, v_meta, st);
    } else {
        if (f32 && hd == 64) launch_decode_float<float, 64>(qb, p, k, v, st);
        else if (f32) launch_decode_float<float, 128>(qb, p, k, v, st);
        else if (hd == 64) launch_decode_float<bf16_t, 64>(qb, p, k, v, st);
        else launch_decode_float<bf16_t, 128>(qb, p, k, v, st);
    }
    OQ_CHECK_LAUNCH(fn);
    return OQ_OK;
}

}  // namespace

extern "C" int oq_kv_append(const void* q, const void* k, const void* v, void* q_out, void* k_out, void* k_cache, void* v_cache,
                            int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap, int64_t past,
                            const float* cos, const float* sin, int64_t P, const int64_t* pos, int64_t pos_bstride,
                            void* stream) {
    return append_plain("oq_kv_append", q, k, v, q_out, k_out, k_cache, v_cache, dtype, bs, Tq, nh, nkv, hd, cap, past, nullptr, NO_PAGES,
                        cos, sin, P, pos, pos_bstride, stream);
}

extern "C" int oq_kv_append_ragged(const void* q, const void* k, const void* v, void* q_out, void* k_out, void* k_cache,
                                   void* v_cache, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap,
                                   const int32_t* lens, const float* cos, const float* sin, int64_t P, const int64_t* pos,
                                   int64_t pos_bstride, void* stream) {
    OQ_CHECK_ARG(lens, "oq_kv_append_ragged: null lens");
    return append_plain("oq_kv_append_ragged", q, k, v, q_out, k_out, k_cache, v_cache, dtype, bs, Tq, nh, nkv, hd, cap, 0, lens, NO_PAGES,
                        cos, sin, P, pos, pos_bstride, stream);
}

extern "C" int64_t oq_attn_decode_workspace(int64_t bs, int nh, int nkv, int64_t Tq, int64_t L, int hd) {
    if (bs <= 0 || nkv <= 0 || nh <= 0 || nh % nkv || Tq <= 0 || L <= 0 || hd <= 0) return 0;
    return (int64_t)dec_splits(bs, nkv, L) * bs * nh * Tq * (hd + 2) * (int64_t)sizeof(float);
}

extern "C" int oq_attn_decode(const void* q, const void* k_cache, const void* v_cache, void* o, int dtype, int64_t bs, int64_t Tq,
                              int nh, int nkv, int hd, int64_t cap, int64_t L, float scale, const void* mask, int mask_dtype,
                              int64_t mask_bstride, int64_t mask_ld, void* workspace, int64_t workspace_bytes, void* stream) {
    return decode("oq_attn_decode", 0, q, k_cache, v_cache, nullptr, nullptr, o, dtype, bs, Tq, nh, nkv, hd, cap, L, nullptr, false,
                  NO_PAGES, scale, mask, mask_dtype, mask_bstride, mask_ld, workspace, workspace_bytes, stream);
}

extern "C" int oq_attn_decode_ragged(const void* q, const void* k_cache, const void* v_cache, void* o, int dtype, int64_t bs,
                                     int64_t Tq, int nh, int nkv, int hd, int64_t cap, const int32_t* lens, int64_t L_bound,
                                     float scale, void* workspace, int64_t workspace_bytes, void* stream) {
    return decode("oq_attn_decode_ragged", 0, q, k_cache, v_cache, nullptr, nullptr, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound, lens,
                  true, NO_PAGES, scale, nullptr, 0, 0, 0, workspace, workspace_bytes, stream);
}

extern "C" int oq_kv_append_quant(const void* q, const void* k, const void* v, int in_dtype, void* q_out, void* k_out, void* v_out,
                                  void* k_cache, void* v_cache, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd,
                                  int64_t cap, int64_t past, const float* cos, const float* sin, int64_t P, const int64_t* pos,
                                  int64_t pos_bstride, int nbits, void* stream) {
    return append_quant("oq_kv_append_quant", q, k, v, in_dtype, q_out, k_out, v_out, k_cache, v_cache, dtype, bs, Tq, nh, nkv, hd, cap,
                        past, nullptr, NO_PAGES, cos, sin, P, pos, pos_bstride, nbits, stream);
}

extern "C" int oq_kv_append_quant_ragged(const void* q, const void* k, const void* v, int in_dtype, void* q_out, void* k_out,
                                         void* v_out, void* k_cache, void* v_cache, int dtype, int64_t bs, int64_t Tq, int nh,
                                         int nkv, int hd, int64_t cap, const int32_t* lens, const float* cos, const float* sin,
                                         int64_t P, const int64_t* pos, int64_t pos_bstride, int nbits, void* stream) {
    OQ_CHECK_ARG(lens, "oq_kv_append_quant_ragged: null lens");
    return append_quant("oq_kv_append_quant_ragged", q, k, v, in_dtype, q_out, k_out, v_out, k_cache, v_cache, dtype, bs, Tq, nh, nkv, hd,
                        cap, 0, lens, NO_PAGES, cos, sin, P, pos, pos_bstride, nbits, stream);
}

extern "C" int oq_kv_append_quant_codes(const void* q, const void* k, const void* v, int in_dtype, void* q_out, void* k_out,
                                        void* v_out, void* k_codes, void* v_codes, float* k_meta, float* v_meta, int dtype,
                                        int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap, int64_t past,
                                        const float* cos, const float* sin, int64_t P, const int64_t* pos, int64_t pos_bstride,
                                        int nbits, void* stream) {
    return append_codes("oq_kv_append_quant_codes", q, k, v, in_dtype, q_out, k_out, v_out, k_codes, v_codes, k_meta, v_meta, dtype, bs,
                        Tq, nh, nkv, hd, cap, past, nullptr, NO_PAGES, cos, sin, P, pos, pos_bstride, 4, nbits, stream);
}

extern "C" int oq_kv_append_quant_codes_ragged(const void* q, const void* k, const void* v, int in_dtype, void* q_out, void* k_out,
                                               void* v_out, void* k_codes, void* v_codes, float* k_meta, float* v_meta, int dtype,
                                               int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap, const int32_t* lens,
                                               const float* cos, const float* sin, int64_t P, const int64_t* pos,
                                               int64_t pos_bstride, int nbits, void* stream) {
    OQ_CHECK_ARG(lens, "oq_kv_append_quant_codes_ragged: null lens");
    return append_codes("oq_kv_append_quant_codes_ragged", q, k, v, in_dtype, q_out, k_out, v_out, k_codes, v_codes, k_meta, v_meta, dtype,
                        bs, Tq, nh, nkv, hd, cap, 0, lens, NO_PAGES, cos, sin, P, pos, pos_bstride, 4, nbits, stream);
}

extern "C" int oq_attn_decode_codes(const void* q, const void* k_codes, const void* v_codes, const float* k_meta,
                                    const float* v_meta, void* o, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd,
                                    int64_t cap, int64_t L, float scale, const void* mask, int mask_dtype, int64_t mask_bstride,
                                    int64_t mask_ld, void* workspace, int64_t workspace_bytes, void* stream) {
    return decode("oq_attn_decode_codes", 4, q, k_codes, v_codes, k_meta, v_meta, o, dtype, bs, Tq, nh, nkv, hd, cap, L, nullptr, false,
                  NO_PAGES, scale, mask, mask_dtype, mask_bstride, mask_ld, workspace, workspace_bytes, stream);
}

extern "C" int oq_attn_decode_codes_ragged(const void* q, const void* k_codes, const void* v_codes, const float* k_meta,
                                           const float* v_meta, void* o, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd,
                                           int64_t cap, const int32_t* lens, int64_t L_bound, float scale, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
    return decode("oq_attn_decode_codes_ragged", 4, q, k_codes, v_codes, k_meta, v_meta, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound,
                  lens, true, NO_PAGES, scale, nullptr, 0, 0, 0, workspace, workspace_bytes, stream);
}

// ---- paged storage: the ragged entry points with (table, max_pages, num_pages, page_size) in the place of cap ------------------
extern "C" int oq_kv_append_paged(const void* q, const void* k, const void* v, void* q_out, void* k_out, void* k_pool, void* v_pool,
                                  int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd, const int32_t* table,
                                  int64_t max_pages, int64_t num_pages, int page_size, const int32_t* lens, const float* cos,
                                  const float* sin, int64_t P, const int64_t* pos, int64_t pos_bstride, void* stream) {
    OQ_PAGE_MAP("oq_kv_append_paged");
    return append_plain("oq_kv_append_paged", q, k, v, q_out, k_out, k_pool, v_pool, dtype, bs, Tq, nh, nkv, hd, cap, 0, lens, pm, cos,
                        sin, P, pos, pos_bstride, stream);
}

extern "C" int oq_kv_append_quant_paged(const void* q, const void* k, const void* v, int in_dtype, void* q_out, void* k_out,
                                        void* v_out, void* k_pool, void* v_pool, int dtype, int64_t bs, int64_t Tq, int nh, int nkv,
                                        int hd, const int32_t* table, int64_t max_pages, int64_t num_pages, int page_size,
                                        const int32_t* lens, const float* cos, const float* sin, int64_t P, const int64_t* pos,
                                        int64_t pos_bstride, int nbits, void* stream) {
    OQ_PAGE_MAP("oq_kv_append_quant_paged");
    OQ_CHECK_ARG(k_pool && v_pool, "oq_kv_append_quant_paged: null pool");
    return append_quant("oq_kv_append_quant_paged", q, k, v, in_dtype, q_out, k_out, v_out, k_pool, v_pool, dtype, bs, Tq, nh, nkv, hd,
                        cap, 0, lens, pm, cos, sin, P, pos, pos_bstride, nbits, stream);
}

extern "C" int oq_kv_append_quant_codes_paged(const void* q, const void* k, const void* v, int in_dtype, void* q_out, void* k_out,
                                              void* v_out, void* k_codes, void* v_codes, float* k_meta, float* v_meta, int dtype,
                                              int64_t bs, int64_t Tq, int nh, int nkv, int hd, const int32_t* table,
                                              int64_t max_pages, int64_t num_pages, int page_size, const int32_t* lens,
                                              const float* cos, const float* sin, int64_t P, const int64_t* pos,
                                              int64_t pos_bstride, int nbits, void* stream) {
    OQ_PAGE_MAP("oq_kv_append_quant_codes_paged");
    return append_codes("oq_kv_append_quant_codes_paged", q, k, v, in_dtype, q_out, k_out, v_out, k_codes, v_codes, k_meta, v_meta, dtype,
                        bs, Tq, nh, nkv, hd, cap, 0, lens, pm, cos, sin, P, pos, pos_bstride, 4, nbits, stream);
}

extern "C" int oq_attn_decode_paged(const void* q, const void* k_pool, const void* v_pool, void* o, int dtype, int64_t bs, int64_t Tq,
                                    int nh, int nkv, int hd, const int32_t* table, int64_t max_pages, int64_t num_pages,
                                    int page_size, const int32_t* lens, int64_t L_bound, float scale, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    OQ_PAGE_MAP("oq_attn_decode_paged");
    return decode("oq_attn_decode_paged", 0, q, k_pool, v_pool, nullptr, nullptr, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound, lens,
                  true, pm, scale, nullptr, 0, 0, 0, workspace, workspace_bytes, stream);
}

extern "C" int oq_attn_decode_codes_paged(const void* q, const void* k_codes, const void* v_codes, const float* k_meta,
                                          const float* v_meta, void* o, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd,
                                          const int32_t* table, int64_t max_pages, int64_t num_pages, int page_size,
                                          const int32_t* lens, int64_t L_bound, float scale, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
    OQ_PAGE_MAP("oq_attn_decode_codes_paged");
    return decode("oq_attn_decode_codes_paged", 4, q, k_codes, v_codes, k_meta, v_meta, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound,
                  lens, true, pm, scale, nullptr, 0, 0, 0, workspace, workspace_bytes, stream);
}

// ---- 8-bit code cache of the weight-only blocks: the entry points of the 4-bit one without nbits --------------------------------
extern "C" int oq_kv_append_codes8(const void* q, const void* k, const void* v, int in_dtype, void* q_out, void* k_out, void* v_out,
                                   void* k_codes, void* v_codes, float* k_meta, float* v_meta, int dtype, int64_t bs, int64_t Tq,
                                   int nh, int nkv, int hd, int64_t cap, int64_t past, const float* cos, const float* sin, int64_t P,
                                   const int64_t* pos, int64_t pos_bstride, void* stream) {
    return append_codes("oq_kv_append_codes8", q, k, v, in_dtype, q_out, k_out, v_out, k_codes, v_codes, k_meta, v_meta, dtype, bs, Tq, nh,
                        nkv, hd, cap, past, nullptr, NO_PAGES, cos, sin, P, pos, pos_bstride, 8, 8, stream);
}

extern "C" int oq_kv_append_codes8_ragged(const void* q, const void* k, const void* v, int in_dtype, void* q_out, void* k_out,
                                          void* v_out, void* k_codes, void* v_codes, float* k_meta, float* v_meta, int dtype,
                                          int64_t bs, int64_t Tq, int nh, int nkv, int hd, int64_t cap, const int32_t* lens,
                                          const float* cos, const float* sin, int64_t P, const int64_t* pos, int64_t pos_bstride,
                                          void* stream) {
    OQ_CHECK_ARG(lens, "oq_kv_append_codes8_ragged: null lens");
    return append_codes("oq_kv_append_codes8_ragged", q, k, v, in_dtype, q_out, k_out, v_out, k_codes, v_codes, k_meta, v_meta, dtype, bs,
                        Tq, nh, nkv, hd, cap, 0, lens, NO_PAGES, cos, sin, P, pos, pos_bstride, 8, 8, stream);
}

extern "C" int oq_kv_append_codes8_paged(const void* q, const void* k, const void* v, int in_dtype, void* q_out, void* k_out,
                                         void* v_out, void* k_codes, void* v_codes, float* k_meta, float* v_meta, int dtype,
                                         int64_t bs, int64_t Tq, int nh, int nkv, int hd, const int32_t* table, int64_t max_pages,
                                         int64_t num_pages, int page_size, const int32_t* lens, const float* cos, const float* sin,
                                         int64_t P, const int64_t* pos, int64_t pos_bstride, void* stream) {
    OQ_PAGE_MAP("oq_kv_append_codes8_paged");
    return append_codes("oq_kv_append_codes8_paged", q, k, v, in_dtype, q_out, k_out, v_out, k_codes, v_codes, k_meta, v_meta, dtype, bs,
                        Tq, nh, nkv, hd, cap, 0, lens, pm, cos, sin, P, pos, pos_bstride, 8, 8, stream);
}

extern "C" int oq_attn_decode_codes8(const void* q, const void* k_codes, const void* v_codes, const float* k_meta,
                                     const float* v_meta, void* o, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd,
                                     int64_t cap, int64_t L, float scale, const void* mask, int mask_dtype, int64_t mask_bstride,
                                     int64_t mask_ld, void* workspace, int64_t workspace_bytes, void* stream) {
    return decode("oq_attn_decode_codes8", 8, q, k_codes, v_codes, k_meta, v_meta, o, dtype, bs, Tq, nh, nkv, hd, cap, L, nullptr, false,
                  NO_PAGES, scale, mask, mask_dtype, mask_bstride, mask_ld, workspace, workspace_bytes, stream);
}

extern "C" int oq_attn_decode_codes8_ragged(const void* q, const void* k_codes, const void* v_codes, const float* k_meta,
                                            const float* v_meta, void* o, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd,
                                            int64_t cap, const int32_t* lens, int64_t L_bound, float scale, void* workspace,
                                            int64_t workspace_bytes, void* stream) {
    return decode("oq_attn_decode_codes8_ragged", 8, q, k_codes, v_codes, k_meta, v_meta, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound,
                  lens, true, NO_PAGES, scale, nullptr, 0, 0, 0, workspace, workspace_bytes, stream);
}

extern "C" int oq_attn_decode_codes8_paged(const void* q, const void* k_codes, const void* v_codes, const float* k_meta,
                                           const float* v_meta, void* o, int dtype, int64_t bs, int64_t Tq, int nh, int nkv, int hd,
                                           const int32_t* table, int64_t max_pages, int64_t num_pages, int page_size,
                                           const int32_t* lens, int64_t L_bound, float scale, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
    OQ_PAGE_MAP("oq_attn_decode_codes8_paged");
    return decode("oq_attn_decode_codes8_paged", 8, q, k_codes, v_codes, k_meta, v_meta, o, dtype, bs, Tq, nh, nkv, hd, cap, L_bound,
                  lens, true, pm, scale, nullptr, 0, 0, 0, workspace, workspace_bytes, stream);
}
