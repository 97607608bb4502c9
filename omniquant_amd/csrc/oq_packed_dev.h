// Packed-layout helpers shared by the two real-quant inference units (oq_packed.hip: float contraction; oq_packed_a4.hip:
// integer contraction).  Both read the AutoGPTQ buffers of oq_pack.hip and both split a skinny GEMV's contraction the same
// way, so the field decode, the layout checks, the split plan and the row-count dispatch live here once.
#pragma once
#include "oq_common.h"

// stored zero code of output column n in one qzeros row (out/32*bits words); the caller adds 1
__device__ __forceinline__ int zero_at(const uint32_t* row, int64_t n, int bits) {
    const int64_t bp = n * bits;
    const int64_t wi = bp >> 5;
    const int off = (int)(bp & 31);
    uint32_t v = row[wi] >> off;
    if (off + bits > 32) v |= row[wi + 1] << (32 - off);
    return (int)(v & ((1u << bits) - 1u));
}

// the 4-bit case (out/8 words per row: a field never straddles two words)
__device__ __forceinline__ int zero4_at(const uint32_t* row, int64_t n) { return zero_at(row, n, 4); }

static inline int check_layout(const char* fn, const void* qweight, const void* qzeros, const void* scales, int64_t in, int64_t out,
                               int64_t group, int bits) {
    OQ_CHECK_ARG(qweight && qzeros && scales, "%s: null pointer", fn);
    OQ_CHECK_ARG(bits == 2 || bits == 3 || bits == 4 || bits == 8, "%s: bits %d (2, 3, 4 or 8)", fn, bits);
    OQ_CHECK_ARG(in > 0 && out > 0 && in % 32 == 0 && out % 32 == 0, "%s: in=%lld out=%lld (multiples of 32)", fn,
                 (long long)in, (long long)out);
    OQ_CHECK_ARG(group > 0 && in % group == 0 && (group == in || group % 32 == 0),
                 "%s: group=%lld (in, or a divisor of in=%lld that is a multiple of 32)", fn, (long long)group, (long long)in);
    return OQ_OK;
}

// ---- GEMV split plan: a workgroup serves PK_COLS output columns (64 lanes x 4) and a run of kb_per 32-channel blocks of
//      the contraction.  The plan is a function of the shape only (never of the device): the float GEMV's split count fixes
//      its summation order, hence its bits.  kb_max: the longest run whose activation slice fits the kernel's LDS. -----------
constexpr int PK_COLS = 256;
constexpr int PK_TARGET_BLOCKS = 512;

static inline int packed_splits(int64_t K, int64_t N, int kb_max, int* kb_per) {
    const int64_t KB = K / 32, tiles = (N + PK_COLS - 1) / PK_COLS;
    int64_t s = (PK_TARGET_BLOCKS + tiles - 1) / tiles;
    const int64_t smin = (KB + kb_max - 1) / kb_max;
    if (s < smin) s = smin;
    if (s > KB) s = KB;
    const int64_t per = (KB + s - 1) / s;
    *kb_per = (int)per;
    return (int)((KB + per - 1) / per);
}

// rows M (1..16) of a GEMV -> the kernels' compile-time row count MM_ in {1, 2, 4, 8, 16}
#define OQ_MM_SWITCH(M, ...)                                        \
    if ((M) <= 1) { constexpr int MM_ = 1; __VA_ARGS__; }           \
    else if ((M) <= 2) { constexpr int MM_ = 2; __VA_ARGS__; }      \
    else if ((M) <= 4) { constexpr int MM_ = 4; __VA_ARGS__; }      \
    else if ((M) <= 8) { constexpr int MM_ = 8; __VA_ARGS__; }      \
    else { constexpr int MM_ = 16; __VA_ARGS__; }
