// Real-quant inference on the packed AutoGPTQ buffers that oq_pack_weights writes (quantize/omniquant.py:255-278; the
// reference evaluates the packed model at main.py:364 through AutoGPTQ's qlinear_cuda.QuantLinear.forward -- a fused
// dequant-matmul kernel below a row threshold, dequantise + dense matmul above it.  PARITY UNPINNED like the pack: the
// library is third-party and not vendored).
//
// Layout (csrc/oq_pack.hip): qweight [in/32*bits, out] int32, 32 input channels of one output column as ONE little-endian
// bit stream over `bits` consecutive word rows (the 3-bit straddle words are simply the stream crossing a word boundary);
// qzeros [in/group, out/32*bits] int32, (zero - 1) packed the same way along the output channels; scales [in/group, out]
// fp16; g_idx = arange(in) / group (act-order is refused by the caller); bias fp16, optional.
//
// Value contract = realquant.PackedLinear.dequantize():  w[o][i] = fp16( f32(scales[g][o]) * f32(q - (zq + 1)) ), codes
// masked to `bits`, one f32 multiply, one RNE rounding to fp16.  Every kernel here computes exactly that value; the bf16
// paths then round it once more, to bf16 (the operand the bf16 MFMA takes: a documented deviation).
//
//   oq_packed_dequant  packed -> W [out, in] in f32 / fp16 / bf16 (bit-exact with dequantize() for fp16).
//   oq_packed_gemv     y[M, out] = x[M, in] W^T (+ bias) (+ addend), M <= 16 (decode): the packed words go straight from
//                      global memory to VGPRs (16-B loads, 4 consecutive output columns per lane), no LDS for the weight;
//                      x is staged once per block in LDS as f32 and read as broadcasts.  K is split over the 4 waves of a
//                      block (reduced through LDS in wave order) and over `splits` blocks (fp32 partials in a workspace,
//                      summed in split order by a second launch): deterministic, no atomics.
//   oq_packed_gemm     the same contract for any M (prefill): 128x128x32 MFMA tile GEMM, 4 waves of 64x64; the x tile is
//                      staged through LDS (16-B chunks, XOR-swizzled rows), the weight tile is loaded packed, dequantised in
//                      registers and written to LDS as MFMA fragments; v_mfma_f32_16x16x32_f16 (fp16 x, exact fp16 weight)
//                      or _bf16 (bf16 x, bf16-rounded weight).  Double-buffered LDS, next tile's loads in flight under the
//                      MFMAs, one barrier per K-step.  fp32 epilogue: + bias + addend, one rounding to x's dtype.
// The qzeros field decode, the layout checks, the GEMV split plan and the M -> MM dispatch are oq_packed_dev.h's, shared
// with oq_packed_a4.hip.
#include "oq_common.h"
#include "oq_packed_dev.h"

namespace {

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// code j (0..31) of the 32 * BITS-bit stream held in w[0 .. BITS-1]; j is a compile-time constant after unrolling
template <int BITS>
__device__ __forceinline__ int code_at(const uint32_t (&w)[BITS], int j) {
    const int bp = j * BITS, wi = bp >> 5, off = bp & 31;
    uint32_t v = w[wi] >> off;
    if (off + BITS > 32) v |= w[wi + 1] << (32 - off);
    return (int)(v & ((1u << BITS) - 1u));
}

// the contract value (fp16, returned widened to f32 exactly); BF: rounded once more to bf16
template <bool BF>
__device__ __forceinline__ float dq(int q, int z, float s) {
    const float v = (float)(f16_t)(s * (float)(q - z));
    return BF ? (float)(bf16_t)v : v;
}

__device__ __forceinline__ float half_at(const void* p, int64_t i) { return (float)reinterpret_cast<const f16_t*>(p)[i]; }

// ---------------------------------------------------------------------------------------------------------------------
// dequant: one thread per (output column n, 32-channel block kb); consecutive threads = consecutive kb of ONE column, so
// the 32-element runs they write (the bulk of the traffic) are contiguous
// ---------------------------------------------------------------------------------------------------------------------
template <int BITS, typename TO>
__global__ void __launch_bounds__(256) packed_dequant_kernel(const uint32_t* qw, const uint32_t* qz, const void* scales,
                                                             int64_t in, int64_t out, int64_t group, TO* w) {
    const int64_t KB = in / 32;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= KB * out) return;
    const int64_t n = idx / KB, kb = idx % KB;
    uint32_t wd[BITS];
#pragma unroll
    for (int r = 0; r < BITS; ++r) wd[r] = qw[(kb * BITS + r) * out + n];
    const int64_t g = kb * 32 / group;
    const float s = half_at(scales, g * out + n);
    const int z = zero_at(qz + g * (out / 32 * BITS), n, BITS) + 1;
    TO* dst = w + n * in + kb * 32;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = dq<false>(code_at<BITS>(wd, c * 8 + j), z, s);
        Vec8<TO>::store(dst + c * 8, v);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// GEMV (M <= 16)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int GV_COLS = PK_COLS;     // output columns per block: 64 lanes x 4
constexpr int GV_KMAX = 512;         // input channels per block (x slice in LDS as f32: 16 rows x 512 x 4 B = 32 KiB)

struct GemvP {
    const void* x;
    const uint32_t* qw;
    const uint32_t* qz;
    const void* scales;
    const void* bias;
    const void* addend;
    void* y;
    float* ws;
    int64_t M, K, N, group;
    int kb_per, splits;
};

template <typename TX>
__device__ __forceinline__ void store_out(const GemvP& p, int64_t m, int64_t n, float v) {
    if (p.bias) v += half_at(p.bias, n);
    if (p.addend) v += (float)reinterpret_cast<const TX*>(p.addend)[m * p.N + n];
    reinterpret_cast<TX*>(p.y)[m * p.N + n] = (TX)v;
}

template <int BITS, typename TX, int MM>
__global__ void __launch_bounds__(256) packed_gemv_kernel(GemvP p) {
    constexpr bool BF = sizeof(TX) == 2 && !__is_same(TX, f16_t);
    constexpr int XS = MM * GV_KMAX, RS = 4 * MM * GV_COLS;
    __shared__ __attribute__((aligned(16))) float smem[XS > RS ? XS : RS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n = (int64_t)blockIdx.x * GV_COLS + lane * 4;
    const int64_t KB = p.K / 32;
    const int64_t kb0 = (int64_t)blockIdx.y * p.kb_per;
    const int64_t kb1 = kb0 + p.kb_per < KB ? kb0 + p.kb_per : KB;
    const int ks = (int)(kb1 - kb0) * 32;
    // x[:, kb0*32 .. kb1*32) -> LDS f32 [MM][ks] (rows >= M are zero)
    const TX* x = reinterpret_cast<const TX*>(p.x);
    for (int i = tid * 8; i < MM * ks; i += 256 * 8) {
        const int m = i / ks, k = i % ks;        // ks % 32 == 0: the 8 elements stay in one row
        float v[8];
        if (m < p.M) Vec8<TX>::load(x + m * p.K + kb0 * 32 + k, v);
        else
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) smem[m * ks + k + j] = v[j];
    }
    __syncthreads();
    float acc[MM][4];
#pragma unroll
    for (int m = 0; m < MM; ++m)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[m][c] = 0.f;
    if (n < p.N) {
        const int64_t zrow = p.N / 32 * BITS;
        int64_t gcur = -1;
        float sc[4];
        int zc[4];
        u32x4 nxt[BITS];
        int64_t kb = kb0 + wv;
        if (kb < kb1) {
#pragma unroll
            for (int r = 0; r < BITS; ++r) nxt[r] = *reinterpret_cast<const u32x4*>(p.qw + (kb * BITS + r) * p.N + n);
        }
        for (; kb < kb1; kb += 4) {
            u32x4 cur[BITS];
#pragma unroll
            for (int r = 0; r < BITS; ++r) cur[r] = nxt[r];
            if (kb + 4 < kb1) {               // next block's words in flight under this block's arithmetic
#pragma unroll
                for (int r = 0; r < BITS; ++r)
                    nxt[r] = *reinterpret_cast<const u32x4*>(p.qw + ((kb + 4) * BITS + r) * p.N + n);
            }
            const int64_t g = kb * 32 / p.group;
            if (g != gcur) {
                gcur = g;
                const f16x4 s4 = *reinterpret_cast<const f16x4*>(reinterpret_cast<const f16_t*>(p.scales) + g * p.N + n);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    sc[c] = (float)s4[c];
                    zc[c] = zero_at(p.qz + g * zrow, n + c, BITS) + 1;
                }
            }
            const float* xs = smem + (kb - kb0) * 32;
#pragma unroll
            for (int j4 = 0; j4 < 8; ++j4) {
                f32x4 xv[MM];
#pragma unroll
                for (int m = 0; m < MM; ++m) xv[m] = *reinterpret_cast<const f32x4*>(xs + m * ks + j4 * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    uint32_t wc[BITS];
#pragma unroll
                    for (int r = 0; r < BITS; ++r) wc[r] = cur[r][c];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const float w = dq<BF>(code_at<BITS>(wc, j4 * 4 + jj), zc[c], sc[c]);
#pragma unroll
                        for (int m = 0; m < MM; ++m) acc[m][c] = __builtin_fmaf(w, xv[m][jj], acc[m][c]);
                    }
                }
            }
        }
    }
    __syncthreads();                          // x slice no longer read: the LDS becomes the wave-reduction buffer
#pragma unroll
    for (int m = 0; m < MM; ++m)
        *reinterpret_cast<f32x4*>(smem + (wv * MM + m) * GV_COLS + lane * 4) = f32x4{acc[m][0], acc[m][1], acc[m][2], acc[m][3]};
    __syncthreads();
    const int64_t col = (int64_t)blockIdx.x * GV_COLS + tid;
    if (col >= p.N) return;
    for (int m = 0; m < MM && m < p.M; ++m) {
        float v = smem[m * GV_COLS + tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) v += smem[(w * MM + m) * GV_COLS + tid];     // fixed wave order
        if (p.splits == 1) store_out<TX>(p, m, col, v);
        else p.ws[((int64_t)blockIdx.y * p.M + m) * p.N + col] = v;
    }
}

// split-K partials [splits][M][N] -> y, summed in split order
template <typename TX>
__global__ void __launch_bounds__(256) packed_gemv_reduce_kernel(GemvP p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.M * p.N) return;
    float v = p.ws[idx];
    for (int s = 1; s < p.splits; ++s) v += p.ws[(int64_t)s * p.M * p.N + idx];
    store_out<TX>(p, idx / p.N, idx % p.N, v);
}

// ---------------------------------------------------------------------------------------------------------------------
// GEMM (any M)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PG_BM = 128, PG_BN = 128, PG_BK = 32;
constexpr int PG_TILE = 128 * PG_BK * 2;     // 8 KiB: [128 rows][32 k] 16-bit, 64-B rows

// byte offset of 16-B chunk kc (0..3) of row `row` in a [128][32] tile; the XOR with (row >> 2) & 3 puts the 16 rows a
// fragment read touches on 16 distinct 16-B bank slots
__device__ __forceinline__ int pg_off(int row, int kc) { return row * 64 + ((kc ^ ((row >> 2) & 3)) << 4); }

struct PGemmP {
    const void* x;
    const uint32_t* qw;
    const uint32_t* qz;
    const void* scales;
    const void* bias;
    const void* addend;
    void* y;
    int64_t M, K, N, group;
};

template <int BITS>
struct PackedB {
    uint32_t w[BITS];
    float s;
    int z;
};

template <int BITS>
__device__ __forceinline__ void load_b(const PGemmP& p, int64_t n, int64_t kt, PackedB<BITS>& b) {
#pragma unroll
    for (int r = 0; r < BITS; ++r) b.w[r] = p.qw[(kt * BITS + r) * p.N + n];
    const int64_t g = kt * PG_BK / p.group;
    b.s = half_at(p.scales, g * p.N + n);
    b.z = zero_at(p.qz + g * (p.N / 32 * BITS), n, BITS) + 1;
}

// dequantise this thread's 16 channels (half H of the 32) of its column into the B tile as two 16-B chunks (H is a template
// parameter so that every code index folds to a constant: a run-time index into b.w would put the words in scratch)
template <int BITS, typename TX, int H>
__device__ __forceinline__ void store_b_half(char* lds, int nl, const PackedB<BITS>& b) {
    constexpr bool BF = !__is_same(TX, f16_t);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        s16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = dq<BF>(code_at<BITS>(b.w, H * 16 + c * 8 + j), b.z, b.s);
            o[j] = __builtin_bit_cast(short, (TX)v);
        }
        *reinterpret_cast<s16x8*>(lds + pg_off(nl, 2 * H + c)) = o;
    }
}

template <int BITS, typename TX>
__device__ __forceinline__ void store_b(char* lds, int nl, int h, const PackedB<BITS>& b) {
    if (h) store_b_half<BITS, TX, 1>(lds, nl, b);      // (wave-uniform: h = tid >> 7)
    else store_b_half<BITS, TX, 0>(lds, nl, b);
}

template <int BITS, typename TX>
__global__ void __launch_bounds__(256, 2) packed_gemm_kernel(PGemmP p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * PG_TILE];     // 2 stages x (A tile, B tile)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int64_t n0 = (int64_t)blockIdx.x * PG_BN, m0 = (int64_t)blockIdx.y * PG_BM;
    const TX* X = reinterpret_cast<const TX*>(p.x);
    // A staging: two 16-B chunks per thread, chunk c = tid + 256 * i -> row c >> 2, k-chunk c & 3 (rows >= M clamped)
    int64_t arow[2];
    int aoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 256 * i, row = c >> 2, kc = c & 3;
        const int64_t m = m0 + row < p.M ? m0 + row : p.M - 1;
        arow[i] = m * p.K + kc * 8;
        aoff[i] = pg_off(row, kc);
    }
    // B staging: column nl = tid & 127 (clamped to N - 1 past the edge: loaded, never stored), channel half h = tid >> 7
    const int nl = tid & 127, h = tid >> 7;
    const int64_t nb = n0 + nl < p.N ? n0 + nl : p.N - 1;
    const int64_t nt = p.K / PG_BK;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 ra[2];
    PackedB<BITS> rb;
#pragma unroll
    for (int i = 0; i < 2; ++i) ra[i] = *reinterpret_cast<const u32x4*>(X + arow[i]);
    load_b<BITS>(p, nb, 0, rb);
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(smem + aoff[i]) = ra[i];
    store_b<BITS, TX>(smem + PG_TILE, nl, h, rb);
    __syncthreads();
    int cur = 0;
    for (int64_t t = 0; t < nt; ++t) {
        const bool more = t + 1 < nt;
        if (more) {
#pragma unroll
            for (int i = 0; i < 2; ++i) ra[i] = *reinterpret_cast<const u32x4*>(X + arow[i] + (t + 1) * PG_BK);
            load_b<BITS>(p, nb, t + 1, rb);
        }
        const char* sa = smem + cur * 2 * PG_TILE;
        const char* sb = sa + PG_TILE;
        s16x8 fa[4], fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const s16x8*>(sa + pg_off(wm * 64 + i * 16 + (lane & 15), lane >> 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const s16x8*>(sb + pg_off(wn * 64 + j * 16 + (lane & 15), lane >> 4));
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // swapped operands (as oq_gemm): lane ends with C[m = lane & 15][n = 4 * (lane >> 4) + r]
                if constexpr (__is_same(TX, f16_t))
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, fb[j]),
                                                                       __builtin_bit_cast(f16x8, fa[i]), acc[i][j], 0, 0, 0);
                else
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fb[j]),
                                                                        __builtin_bit_cast(bf16x8, fa[i]), acc[i][j], 0, 0, 0);
            }
        if (more) {
            char* da = smem + (cur ^ 1) * 2 * PG_TILE;
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(da + aoff[i]) = ra[i];
            store_b<BITS, TX>(da + PG_TILE, nl, h, rb);
        }
        __syncthreads();
        cur ^= 1;
    }
    // epilogue: lane holds 4 consecutive n for one m; N % 32 == 0 keeps a lane's 4 columns all inside or all outside
    TX* Y = reinterpret_cast<TX*>(p.y);
    const TX* AD = reinterpret_cast<const TX*>(p.addend);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + wm * 64 + i * 16 + (lane & 15);
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t n = n0 + wn * 64 + j * 16 + (lane >> 4) * 4;
            if (n >= p.N) continue;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = acc[i][j][r];
                if (p.bias) v[r] += half_at(p.bias, n + r);
                if (AD) v[r] += (float)AD[m * p.N + n + r];
            }
            if constexpr (__is_same(TX, f16_t))
                *reinterpret_cast<f16x4*>(Y + m * p.N + n) = f16x4{(f16_t)v[0], (f16_t)v[1], (f16_t)v[2], (f16_t)v[3]};
            else
                *reinterpret_cast<bf16x4*>(Y + m * p.N + n) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
        }
    }
}

#define OQ_BITS_SWITCH(bits, ...)                              \
    switch (bits) {                                            \
        case 2: { constexpr int B_ = 2; __VA_ARGS__; } break;  \
        case 3: { constexpr int B_ = 3; __VA_ARGS__; } break;  \
        case 4: { constexpr int B_ = 4; __VA_ARGS__; } break;  \
        default: { constexpr int B_ = 8; __VA_ARGS__; } break; \
    }

template <int BITS, typename TX>
void launch_gemv(const GemvP& p, hipStream_t st) {
    const dim3 grid((unsigned)((p.N + GV_COLS - 1) / GV_COLS), (unsigned)p.splits);
    OQ_MM_SWITCH(p.M, hipLaunchKernelGGL((packed_gemv_kernel<BITS, TX, MM_>), grid, dim3(256), 0, st, p))
    if (p.splits > 1)
        hipLaunchKernelGGL((packed_gemv_reduce_kernel<TX>), dim3((unsigned)((p.M * p.N + 255) / 256)), dim3(256), 0, st, p);
}

}  // namespace

extern "C" int oq_packed_dequant(const int32_t* qweight, const int32_t* qzeros, const void* scales, int64_t in, int64_t out,
                                 int64_t group, int bits, void* w, int w_dtype, void* stream) {
    if (int rc = check_layout("oq_packed_dequant", qweight, qzeros, scales, in, out, group, bits)) return rc;
    OQ_CHECK_ARG(w != nullptr, "oq_packed_dequant: null output");
    OQ_CHECK_ARG(w_dtype == OQ_F32 || w_dtype == OQ_F16 || w_dtype == OQ_BF16, "oq_packed_dequant: dtype %d", w_dtype);
    OQ_CHECK_ARG(oq_aligned16(w), "oq_packed_dequant: output not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((in / 32 * out + 255) / 256));
    const uint32_t* qw = (const uint32_t*)qweight;
    const uint32_t* qz = (const uint32_t*)qzeros;
    OQ_BITS_SWITCH(bits, {
        if (w_dtype == OQ_F32)
            hipLaunchKernelGGL((packed_dequant_kernel<B_, float>), grid, dim3(256), 0, st, qw, qz, scales, in, out, group, (float*)w);
        else if (w_dtype == OQ_F16)
            hipLaunchKernelGGL((packed_dequant_kernel<B_, f16_t>), grid, dim3(256), 0, st, qw, qz, scales, in, out, group, (f16_t*)w);
        else
            hipLaunchKernelGGL((packed_dequant_kernel<B_, bf16_t>), grid, dim3(256), 0, st, qw, qz, scales, in, out, group, (bf16_t*)w);
    })
    OQ_CHECK_LAUNCH("oq_packed_dequant");
    return OQ_OK;
}

extern "C" int64_t oq_packed_gemv_workspace(int64_t M, int64_t in, int64_t out, int bits) {
    (void)bits;
    if (M <= 0 || in <= 0 || out <= 0 || in % 32 != 0) return 0;
    int per;
    const int s = packed_splits(in, out, GV_KMAX / 32, &per);
    return s > 1 ? (int64_t)s * M * out * 4 : 0;
}

extern "C" int oq_packed_gemv(const void* x, int x_dtype, int64_t M, int64_t in, int64_t out, int64_t group, int bits,
                              const int32_t* qweight, const int32_t* qzeros, const void* scales, const void* bias,
                              const void* addend, void* y, void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = check_layout("oq_packed_gemv", qweight, qzeros, scales, in, out, group, bits)) return rc;
    OQ_CHECK_ARG(x && y, "oq_packed_gemv: null x / y");
    OQ_CHECK_ARG(x_dtype == OQ_F16 || x_dtype == OQ_BF16, "oq_packed_gemv: x dtype %d (fp16 or bf16)", x_dtype);
    OQ_CHECK_ARG(M >= 1 && M <= 16, "oq_packed_gemv: M=%lld (1..16; larger M: oq_packed_gemm)", (long long)M);
    OQ_CHECK_ARG(oq_aligned16(x) && oq_aligned16(qweight) && ((uintptr_t)scales & 7) == 0,
                 "oq_packed_gemv: x / qweight must be 16-byte and scales 8-byte aligned");
    GemvP p{x, (const uint32_t*)qweight, (const uint32_t*)qzeros, scales, bias, addend, y, (float*)workspace, M, in, out, group,
            0, 0};
    p.splits = packed_splits(in, out, GV_KMAX / 32, &p.kb_per);
    const int64_t need = p.splits > 1 ? (int64_t)p.splits * M * out * 4 : 0;
    OQ_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace != nullptr),
                 "oq_packed_gemv: workspace of %lld bytes needed (oq_packed_gemv_workspace), %lld given", (long long)need,
                 (long long)workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    OQ_BITS_SWITCH(bits, {
        if (x_dtype == OQ_F16) launch_gemv<B_, f16_t>(p, st);
        else launch_gemv<B_, bf16_t>(p, st);
    })
    OQ_CHECK_LAUNCH("oq_packed_gemv");
    return OQ_OK;
}

extern "C" int oq_packed_gemm(const void* x, int x_dtype, int64_t M, int64_t in, int64_t out, int64_t group, int bits,
                              const int32_t* qweight, const int32_t* qzeros, const void* scales, const void* bias,
                              const void* addend, void* y, void* stream) {
    if (int rc = check_layout("oq_packed_gemm", qweight, qzeros, scales, in, out, group, bits)) return rc;
    OQ_CHECK_ARG(x && y, "oq_packed_gemm: null x / y");
    OQ_CHECK_ARG(x_dtype == OQ_F16 || x_dtype == OQ_BF16, "oq_packed_gemm: x dtype %d (fp16 or bf16)", x_dtype);
    OQ_CHECK_ARG(M >= 1, "oq_packed_gemm: M=%lld", (long long)M);
    OQ_CHECK_ARG((M + PG_BM - 1) / PG_BM <= 65535, "oq_packed_gemm: M=%lld too large for one launch", (long long)M);
    OQ_CHECK_ARG(oq_aligned16(x) && ((uintptr_t)y & 7) == 0 && ((uintptr_t)addend & 7) == 0,
                 "oq_packed_gemm: x must be 16-byte, y / addend 8-byte aligned");
    PGemmP p{x, (const uint32_t*)qweight, (const uint32_t*)qzeros, scales, bias, addend, y, M, in, out, group};
    const dim3 grid((unsigned)((out + PG_BN - 1) / PG_BN), (unsigned)((M + PG_BM - 1) / PG_BM));
    hipStream_t st = (hipStream_t)stream;
    OQ_BITS_SWITCH(bits, {
        if (x_dtype == OQ_F16) hipLaunchKernelGGL((packed_gemm_kernel<B_, f16_t>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((packed_gemm_kernel<B_, bf16_t>), grid, dim3(256), 0, st, p);
    })
    OQ_CHECK_LAUNCH("oq_packed_gemm");
    return OQ_OK;
}
