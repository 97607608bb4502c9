// W4A4 real-quant inference on gfx950: integer contraction of 4-bit per-token activation codes with the packed 4-bit
// AutoGPTQ weight words (quantize/omniquant.py:255-278 packs the weight; quantize/int_linear.py:59-62 quantises the input
// per token with quantize/quantizer.py:84-147).
//
// Value contract, for output row t and column n (per-channel weight: one scale / zero per column):
//     y[t][n] = s_a[t] * s_w[n] * sum_k (q_a[t][k] - z_a[t]) * (q_w[k][n] - z_w[n])  + bias[n]  (+ addend[t][n])
//   q_a, s_a, z_a  the per-token asymmetric quantiser's codes (0..15 as int8), scale and rounded zero-point, as the
//                  quantiser kernels write them (ops.IntCodes; csum Ca[t] = sum_k q_a[t][k], NaN for a degenerate row)
//   q_w            the 4-bit codes of qweight (nibble j of word w = input channel 8w + j, word row w, column n)
//   z_w            the unpacked qzeros + 1, decoded as PackedLinear.dequantize() decodes it (a stored zero of -1 wraps to 16)
//   s_w            the fp16 scale widened to fp32
// The integer sum is exact; the epilogue is oq_i8_epilogue (oq_common.h), the expression oq_gemm_i8 uses, so a row's result
// does not depend on M nor on the kernel that served it.  This is the exact product of the two fake-quant grids, NOT the
// value of dequantize(), which rounds s_w * (q - z) to fp16 first.
//
//   oq_packed_gemv_a4  decode (1 <= M <= 16): each workgroup packs its K slice of the activation codes into nibble words
//                      in LDS once (the qweight word order), then every weight word meets every row's word in ONE
//                      v_dot8_u32_u4; a second dot8 against 0x11111111 gives the column code sums Cw on the way.  The
//                      packed words go from global memory to VGPRs (16-B loads, 4 columns per lane, the next rows in flight).
//                      K is split over the 4 waves (reduced through LDS) and over workgroups (int32 partials in a workspace,
//                      summed by a second launch): integer partials, so any order is exact and the result deterministic.
//   oq_packed_codes    prefill: qweight -> int8 codes [out, in] (k-contiguous, oq_gemm_i8's B operand) plus fp32 s_w, z_w
//                      and Cw [out], a complete ops.IntCodes of the weight; the caller then runs oq_gemm_i8.
//   oq_quant_codes     the per-token quantiser with integer codes for rows the fused quantiser kernels do not take (they
//                      need 512+ columns): one wave per row, the same oq_quant_dev.h arithmetic.
// zero4_at, the layout checks, the GEMV split plan and the M -> MM dispatch are oq_packed_dev.h's, shared with oq_packed.hip.
#include "oq_common.h"
#include "oq_packed_dev.h"
#include "oq_quant_dev.h"

namespace {

// 8 int8 codes (0..15) -> one nibble word, nibble j = byte j
__device__ __forceinline__ uint32_t pack_nibbles(uint32_t lo, uint32_t hi) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        w |= ((lo >> (8 * j)) & 15u) << (4 * j);
        w |= ((hi >> (8 * j)) & 15u) << (4 * (j + 4));
    }
    return w;
}

// one nibble word -> 8 int8 codes (byte j = nibble j)
__device__ __forceinline__ void unpack_nibbles(uint32_t w, uint32_t& lo, uint32_t& hi) {
    lo = 0;
    hi = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lo |= ((w >> (4 * j)) & 15u) << (8 * j);
        hi |= ((w >> (4 * (j + 4))) & 15u) << (8 * j);
    }
}

__device__ __forceinline__ uint32_t dot8(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot8(a, b, c, false); }

// ---------------------------------------------------------------------------------------------------------------------
// GEMV (1 <= M <= 16)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int A4_COLS = PK_COLS;          // output columns per workgroup: 64 lanes x 4
constexpr int A4_WMAX = 256;              // packed activation words per row and workgroup (a K slice of 2048 channels)
constexpr int A4_KBMAX = A4_WMAX / 4;     // the same in 32-channel blocks of 4 words: packed_splits' unit

struct A4P {
    const int8_t* codes;
    const float *sa, *za, *ca;
    const uint32_t* qw;
    const uint32_t* qz;
    const f16_t* scales;
    const f16_t* bias;
    const void* addend;
    void* y;
    int32_t* ws;                          // split partials [splits][M + 1][N] (row M: the column code sums)
    int64_t M, K, N;
    int w_per, splits, add_f32, y_f32;
};

__device__ __forceinline__ void a4_store(const A4P& p, int64_t m, int64_t n, uint32_t acc, uint32_t cw) {
    const float s_a = p.sa[m], z_a = p.za[m];
    const float a2 = oq_i8_a2(p.ca[m], (float)p.K, z_a);
    const float s_w = (float)p.scales[n];
    const float z_w = (float)(zero4_at(p.qz, n) + 1);
    const float b = p.bias ? (float)p.bias[n] : 0.f;
    float v = oq_i8_epilogue((float)(int)acc, z_a, a2, s_a, z_w, (float)(int)cw, s_w, b);
    if (p.addend) v += p.add_f32 ? reinterpret_cast<const float*>(p.addend)[m * p.N + n]
                                 : (float)reinterpret_cast<const bf16_t*>(p.addend)[m * p.N + n];
    if (p.y_f32) reinterpret_cast<float*>(p.y)[m * p.N + n] = v;
    else reinterpret_cast<bf16_t*>(p.y)[m * p.N + n] = (bf16_t)v;
}

template <int MM>
__global__ void __launch_bounds__(256) packed_gemv_a4_kernel(A4P p) {
    __shared__ __attribute__((aligned(16))) uint32_t act[MM * A4_WMAX];
    __shared__ __attribute__((aligned(16))) uint32_t red[4 * A4_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n = (int64_t)blockIdx.x * A4_COLS + lane * 4;
    const int64_t KW = p.K / 8;
    const int64_t w0 = (int64_t)blockIdx.y * p.w_per;
    const int64_t w1 = w0 + p.w_per < KW ? w0 + p.w_per : KW;
    const int nw = (int)(w1 - w0);
    // activation codes of rows < M, channels [8 w0, 8 w1) -> nibble words in LDS (rows >= M: zero, never stored)
    for (int i = tid; i < MM * nw; i += 256) {
        const int m = i / nw, j = i - m * nw;
        uint32_t w = 0;
        if (m < p.M) {
            typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
            const u32x2 c = *reinterpret_cast<const u32x2*>(p.codes + m * p.K + (w0 + j) * 8);
            w = pack_nibbles(c[0], c[1]);
        }
        act[m * A4_WMAX + j] = w;
    }
    __syncthreads();
    uint32_t acc[MM][4], cw[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        cw[c] = 0;
#pragma unroll
        for (int m = 0; m < MM; ++m) acc[m][c] = 0;
    }
    if (n < p.N) {
        // wave wv takes word rows w0 + 4 wv + 16 i .. + 4: four 16-B loads per lane, the next four in flight
        int64_t w = w0 + 4 * wv;
        u32x4 nxt[4];
        if (w < w1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) nxt[r] = *reinterpret_cast<const u32x4*>(p.qw + (w + r) * p.N + n);
        }
        for (; w < w1; w += 16) {
            u32x4 cur[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) cur[r] = nxt[r];
            if (w + 16 < w1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) nxt[r] = *reinterpret_cast<const u32x4*>(p.qw + (w + 16 + r) * p.N + n);
            }
            u32x4 a[MM];
#pragma unroll
            for (int m = 0; m < MM; ++m) a[m] = *reinterpret_cast<const u32x4*>(act + m * A4_WMAX + (w - w0));
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    cw[c] = dot8(cur[r][c], 0x11111111u, cw[c]);
#pragma unroll
                    for (int m = 0; m < MM; ++m) acc[m][c] = dot8(cur[r][c], a[m][r], acc[m][c]);
                }
        }
    }
    // wave partials -> LDS -> one sum per column (integers: exact in any order); the code sums first, then row by row
    const int64_t col = (int64_t)blockIdx.x * A4_COLS + tid;
    uint32_t cws = 0;
#pragma unroll
    for (int m = -1; m < MM; ++m) {
        if (m >= (int)p.M) continue;                        // uniform (rows >= M: nothing to store)
        __syncthreads();
        u32x4 v;
        if (m < 0) v = u32x4{cw[0], cw[1], cw[2], cw[3]};
        else v = u32x4{acc[m < 0 ? 0 : m][0], acc[m < 0 ? 0 : m][1], acc[m < 0 ? 0 : m][2], acc[m < 0 ? 0 : m][3]};
        *reinterpret_cast<u32x4*>(red + wv * A4_COLS + lane * 4) = v;
        __syncthreads();
        const uint32_t s = (red[tid] + red[A4_COLS + tid]) + (red[2 * A4_COLS + tid] + red[3 * A4_COLS + tid]);
        if (col >= p.N) continue;
        if (m < 0) {
            cws = s;
            if (p.splits > 1) p.ws[((int64_t)blockIdx.y * (p.M + 1) + p.M) * p.N + col] = (int32_t)s;
        } else if (p.splits == 1) {
            a4_store(p, m, col, s, cws);
        } else {
            p.ws[((int64_t)blockIdx.y * (p.M + 1) + m) * p.N + col] = (int32_t)s;
        }
    }
}

// split partials -> y: one thread per (row, column)
__global__ void __launch_bounds__(256) packed_gemv_a4_reduce_kernel(A4P p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.M * p.N) return;
    const int64_t m = idx / p.N, n = idx - m * p.N;
    uint32_t acc = 0, cw = 0;
#pragma unroll 8
    for (int s = 0; s < p.splits; ++s) {                    // (integers: the unrolled loads overlap, the sum is exact)
        acc += (uint32_t)p.ws[((int64_t)s * (p.M + 1) + m) * p.N + n];
        cw += (uint32_t)p.ws[((int64_t)s * (p.M + 1) + p.M) * p.N + n];
    }
    a4_store(p, m, n, acc, cw);
}

// ---------------------------------------------------------------------------------------------------------------------
// weight codes (prefill): 32 word rows x 64 columns per workgroup, transposed through LDS so that both the qweight reads
// (256 B per row) and the code writes (256 B per column) are contiguous
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PC_ROWS = 32, PC_COLS = 64;

// s_w, z_w per column; the code sums start at 0 (int32 bits in the float buffer until packed_codes_finish)
__global__ void __launch_bounds__(256) packed_codes_vec_kernel(const uint32_t* qz, const f16_t* scales, int64_t N, float* sw,
                                                               float* zw, float* cw) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    sw[n] = (float)scales[n];
    zw[n] = (float)(zero4_at(qz, n) + 1);
    reinterpret_cast<int32_t*>(cw)[n] = 0;
}

__global__ void __launch_bounds__(256) packed_codes_kernel(const uint32_t* qw, int64_t K, int64_t N, int8_t* codes, float* cw) {
    __shared__ uint32_t tile[PC_ROWS][PC_COLS + 1];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * PC_ROWS, n0 = (int64_t)blockIdx.x * PC_COLS;
    const int64_t KW = K / 8;
#pragma unroll
    for (int i = 0; i < PC_ROWS * PC_COLS / 256; ++i) {
        const int r = i * 4 + (tid >> 6), c = tid & 63;
        uint32_t v = 0;
        if (r0 + r < KW && n0 + c < N) v = qw[(r0 + r) * N + n0 + c];
        tile[r][c] = v;
    }
    __syncthreads();
    // thread -> column tid / 4, word rows (tid % 4) * 8 .. + 8: 64 codes = four 16-B stores
    const int c = tid >> 2, rb = (tid & 3) * 8;
    const int64_t n = n0 + c;
    uint32_t sum = 0;
    if (n < N) {
        int8_t* dst = codes + n * K + (r0 + rb) * 8;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            u32x4 o;
            uint32_t lo, hi;
            unpack_nibbles(tile[rb + 2 * h][c], lo, hi);
            o[0] = lo; o[1] = hi;
            unpack_nibbles(tile[rb + 2 * h + 1][c], lo, hi);
            o[2] = lo; o[3] = hi;
            sum = dot8(tile[rb + 2 * h][c], 0x11111111u, sum);
            sum = dot8(tile[rb + 2 * h + 1][c], 0x11111111u, sum);
            if (r0 + rb + 2 * h + 1 < KW) *reinterpret_cast<u32x4*>(dst + h * 16) = o;      // KW % 4 == 0: pairs stay whole
        }
    }
    // the four threads of a column: one integer atomic per column and workgroup (exact, order-free)
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    if ((tid & 3) == 0 && n < N) atomicAdd(reinterpret_cast<int32_t*>(cw) + n, (int32_t)sum);
}

__global__ void __launch_bounds__(256) packed_codes_finish_kernel(int64_t N, float* cw) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    cw[n] = (float)reinterpret_cast<const int32_t*>(cw)[n];
}

// ---------------------------------------------------------------------------------------------------------------------
// per-token quantiser with codes, one wave per row (any row length that is a multiple of 8)
// ---------------------------------------------------------------------------------------------------------------------
template <typename TIN, typename TOUT>
__global__ void __launch_bounds__(256) quant_codes_kernel(const TIN* x, int64_t rows, int64_t cols, int nbits, float inv_q,
                                                          TOUT* y, float* scale, float* zp, int8_t* codes, float* csum) {
    const int lane = threadIdx.x & 63;
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= rows) return;                                  // whole waves
    const TIN* xr = x + r * cols;
    const float Q = (float)((1 << nbits) - 1);
    float hi = -INFINITY, lo = INFINITY, bad = 0.f;
    for (int64_t c0 = lane * 8; c0 < cols; c0 += 512) {
        float v[8];
        Vec8<TIN>::load(xr + c0, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            hi = fmaxf(hi, v[i]);
            lo = fminf(lo, v[i]);
            if (v[i] != v[i]) bad = 1.f;
        }
    }
    hi = wave_max(hi);
    lo = wave_min(lo);
    bad = wave_max(bad);
    if (bad != 0.f) { hi = NAN; lo = NAN; }
    float inv_s = 0.f;
    const QP q = make_qp(hi, lo, false, 0.f, 0.f, nbits, 0, inv_q, &inv_s);
    const bool regular = q.s != 0.f && fabsf(q.s) <= 3.4028234663852886e38f && bad == 0.f;
    float cs = 0.f;
    for (int64_t c0 = lane * 8; c0 < cols; c0 += 512) {
        float v[8], yv[8], qv[8];
        Vec8<TIN>::load(xr + c0, v);
        if (regular) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float tq;
                const float rq = rne_div(v[i], q.s, inv_s, &tq);
                qv[i] = __builtin_amdgcn_fmed3f(rq + q.z, 0.f, Q);
                yv[i] = (qv[i] - q.z) * q.s;
                cs += qv[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float t = rne_ste(v[i] / q.s) + q.z;
                t = (t != t) ? t : fminf(fmaxf(t, 0.f), Q);
                yv[i] = (t - q.z) * q.s;
                qv[i] = 0.f;
            }
        }
        if (y) Vec8<TOUT>::store(y + r * cols + c0, yv);
        oq_store_codes8(codes + r * cols + c0, qv, false);
    }
    cs = wave_sum(cs);
    if (lane == 0) {
        scale[r] = q.s;
        zp[r] = q.z;
        csum[r] = regular ? cs : NAN;                       // a degenerate row poisons its own output row (quirk Q1)
    }
}

}  // namespace

extern "C" int64_t oq_packed_gemv_a4_workspace(int64_t M, int64_t in, int64_t out) {
    if (M <= 0 || in <= 0 || out <= 0 || in % 32 != 0) return 0;
    int per;
    const int s = packed_splits(in, out, A4_KBMAX, &per);
    return s > 1 ? (int64_t)s * (M + 1) * out * 4 : 0;
}

// the 4-bit per-channel layout (check_layout) plus what the integer kernels need
static int check_a4(const char* fn, const int32_t* qweight, const int32_t* qzeros, const void* scales, int64_t in, int64_t out) {
    if (int rc = check_layout(fn, qweight, qzeros, scales, in, out, in, 4)) return rc;
    OQ_CHECK_ARG(in <= (1ll << 16), "%s: in=%lld too long for the integer accumulation", fn, (long long)in);
    OQ_CHECK_ARG(oq_aligned16(qweight), "%s: qweight must be 16-byte aligned", fn);
    return OQ_OK;
}

extern "C" int oq_packed_gemv_a4(const void* codes, const float* a_scale, const float* a_zp, const float* a_csum, int64_t M,
                                 int64_t in, int64_t out, const int32_t* qweight, const int32_t* qzeros, const void* scales,
                                 const void* bias, const void* addend, int addend_dtype, void* y, int y_dtype, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    if (int rc = check_a4("oq_packed_gemv_a4", qweight, qzeros, scales, in, out)) return rc;
    OQ_CHECK_ARG(codes && a_scale && a_zp && a_csum && y, "oq_packed_gemv_a4: null activation operand / output");
    OQ_CHECK_ARG(M >= 1 && M <= 16, "oq_packed_gemv_a4: M=%lld (1..16; larger M: oq_packed_codes + oq_gemm_i8)", (long long)M);
    OQ_CHECK_ARG(y_dtype == OQ_F32 || y_dtype == OQ_BF16, "oq_packed_gemv_a4: output dtype %d (f32 or bf16)", y_dtype);
    OQ_CHECK_ARG(!addend || addend_dtype == OQ_F32 || addend_dtype == OQ_BF16, "oq_packed_gemv_a4: addend dtype %d", addend_dtype);
    OQ_CHECK_ARG(oq_aligned16(codes), "oq_packed_gemv_a4: codes must be 16-byte aligned");
    A4P p{};
    p.codes = (const int8_t*)codes; p.sa = a_scale; p.za = a_zp; p.ca = a_csum;
    p.qw = (const uint32_t*)qweight; p.qz = (const uint32_t*)qzeros; p.scales = (const f16_t*)scales; p.bias = (const f16_t*)bias;
    p.addend = addend; p.add_f32 = addend_dtype == OQ_F32; p.y = y; p.y_f32 = y_dtype == OQ_F32;
    p.ws = (int32_t*)workspace; p.M = M; p.K = in; p.N = out;
    p.splits = packed_splits(in, out, A4_KBMAX, &p.w_per);
    p.w_per *= 4;                             // whole blocks: a multiple of 4 words, as the kernel's 16-B activation reads need
    const int64_t need = p.splits > 1 ? (int64_t)p.splits * (M + 1) * out * 4 : 0;
    OQ_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace != nullptr),
                 "oq_packed_gemv_a4: workspace of %lld bytes needed (oq_packed_gemv_a4_workspace), %lld given", (long long)need,
                 (long long)workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((out + A4_COLS - 1) / A4_COLS), (unsigned)p.splits);
    OQ_MM_SWITCH(M, hipLaunchKernelGGL((packed_gemv_a4_kernel<MM_>), grid, dim3(256), 0, st, p))
    if (p.splits > 1)
        hipLaunchKernelGGL(packed_gemv_a4_reduce_kernel, dim3((unsigned)((M * out + 255) / 256)), dim3(256), 0, st, p);
    OQ_CHECK_LAUNCH("oq_packed_gemv_a4");
    return OQ_OK;
}

extern "C" int oq_packed_codes(const int32_t* qweight, const int32_t* qzeros, const void* scales, int64_t in, int64_t out,
                               void* codes, float* w_scale, float* w_zp, float* w_csum, void* stream) {
    if (int rc = check_a4("oq_packed_codes", qweight, qzeros, scales, in, out)) return rc;
    OQ_CHECK_ARG(codes && w_scale && w_zp && w_csum, "oq_packed_codes: null output");
    OQ_CHECK_ARG(oq_aligned16(codes), "oq_packed_codes: codes must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 vgrid((unsigned)((out + 255) / 256));
    hipLaunchKernelGGL(packed_codes_vec_kernel, vgrid, dim3(256), 0, st, (const uint32_t*)qzeros, (const f16_t*)scales, out, w_scale,
                       w_zp, w_csum);
    const dim3 grid((unsigned)((out + PC_COLS - 1) / PC_COLS), (unsigned)((in / 8 + PC_ROWS - 1) / PC_ROWS));
    hipLaunchKernelGGL(packed_codes_kernel, grid, dim3(256), 0, st, (const uint32_t*)qweight, in, out, (int8_t*)codes, w_csum);
    hipLaunchKernelGGL(packed_codes_finish_kernel, vgrid, dim3(256), 0, st, out, w_csum);
    OQ_CHECK_LAUNCH("oq_packed_codes");
    return OQ_OK;
}

extern "C" int oq_quant_codes(const void* x, int dtype, int64_t rows, int64_t cols, int nbits, void* y, int y_dtype, float* scale,
                              float* zp, void* codes, float* csum, void* stream) {
    OQ_CHECK_ARG(x && scale && zp && codes && csum, "oq_quant_codes: null pointer");
    OQ_CHECK_ARG(rows > 0 && cols > 0 && cols % 8 == 0, "oq_quant_codes: rows %lld cols %lld (cols a multiple of 8)", (long long)rows,
                 (long long)cols);
    OQ_CHECK_ARG(nbits >= 2 && nbits <= 7, "oq_quant_codes: %d-bit grid (2..7: plain codes in an int8)", nbits);
    OQ_CHECK_ARG(dtype == OQ_F32 || dtype == OQ_BF16, "oq_quant_codes: input dtype %d (f32 or bf16)", dtype);
    OQ_CHECK_ARG(!y || y_dtype == OQ_F32 || y_dtype == OQ_BF16, "oq_quant_codes: output dtype %d", y_dtype);
    OQ_CHECK_ARG(oq_aligned16(x) && oq_aligned16(y) && ((uintptr_t)codes & 7) == 0, "oq_quant_codes: alignment");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((rows + 3) / 4));
    const float inv_q = 1.0f / (float)((1 << nbits) - 1);
    int8_t* c8 = (int8_t*)codes;
    if (dtype == OQ_F32) {
        if (!y || y_dtype == OQ_F32)
            hipLaunchKernelGGL((quant_codes_kernel<float, float>), grid, dim3(256), 0, st, (const float*)x, rows, cols, nbits, inv_q,
                               (float*)y, scale, zp, c8, csum);
        else
            hipLaunchKernelGGL((quant_codes_kernel<float, bf16_t>), grid, dim3(256), 0, st, (const float*)x, rows, cols, nbits, inv_q,
                               (bf16_t*)y, scale, zp, c8, csum);
    } else {
        if (y && y_dtype == OQ_F32)
            hipLaunchKernelGGL((quant_codes_kernel<bf16_t, float>), grid, dim3(256), 0, st, (const bf16_t*)x, rows, cols, nbits, inv_q,
                               (float*)y, scale, zp, c8, csum);
        else
            hipLaunchKernelGGL((quant_codes_kernel<bf16_t, bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)x, rows, cols, nbits,
                               inv_q, (bf16_t*)y, scale, zp, c8, csum);
    }
    OQ_CHECK_LAUNCH("oq_quant_codes");
    return OQ_OK;
}
