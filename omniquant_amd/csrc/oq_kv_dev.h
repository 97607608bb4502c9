// What the two attention units over the KV cache share (oq_decode.hip: scalar-FMA split-L decode; oq_extend.hip: MFMA chunked
// prefill): the page map of paged storage and its host checks, the shape-only split plan of the decode kernel, and the combine
// kernel that merges per-split (max, sum, accumulator) partials.  Both units write partials in one workspace layout, so the
// combine kernel, hence the order of the merge, lives here once.
#pragma once
#include "oq_common.h"

namespace {      // internal to each unit, like the kernels that use it

// Paged storage: the rows of a cache live in pages of PS = 1 << lg rows per kv head, pool buffers [num_pages, nkv, PS, ...],
// and logical row j of sequence b is row j & (PS - 1) of page table[b * max_pages + (j >> lg)].  table == NULL: the contiguous
// [bs, nkv, cap, ...] slab.  The host never reads the table, so the kernels guard its entries: a row whose entry lies outside
// [0, num_pages) is neither stored (append) nor loaded (attention, where it counts as invisible).
struct PageMap {
    const int32_t* table;               // int32 [bs, max_pages] on the device
    int64_t max_pages, num_pages;
    int lg;
};

const PageMap NO_PAGES{nullptr, 0, 0, 0};

// The page map of a _paged entry point, checked (the table's values stay unread); *cap = the rows a sequence can address.
inline int page_map(const char* fn, const int32_t* table, int64_t max_pages, int64_t num_pages, int page_size, PageMap* pm,
                    int64_t* cap) {
    OQ_CHECK_ARG(page_size == 16 || page_size == 32 || page_size == 64 || page_size == 128, "%s: page_size %d (16, 32, 64 or 128)", fn,
                 page_size);
    OQ_CHECK_ARG(num_pages > 0 && max_pages > 0 && max_pages <= (INT64_MAX >> 8), "%s: num_pages %lld, max_pages %lld", fn,
                 (long long)num_pages, (long long)max_pages);
    OQ_CHECK_ARG(table && (uintptr_t)table % 4 == 0, "%s: table (int32 [bs, max_pages] on the device)", fn);
    int lg = 4;
    while ((1 << lg) < page_size) ++lg;
    *pm = PageMap{table, max_pages, num_pages, lg};
    *cap = max_pages * page_size;
    return OQ_OK;
}

#define OQ_PAGE_MAP(fn)                                                                        \
    PageMap pm;                                                                                \
    int64_t cap;                                                                               \
    OQ_CHECK_ARG(lens, fn ": null lens");                                                      \
    if (const int rc = page_map(fn, table, max_pages, num_pages, page_size, &pm, &cap)) return rc

constexpr int DEC_TARGET_WG = 1024;     // 4 workgroups of 4 waves per CU
constexpr int DEC_MAX_SPLIT = 64;
constexpr int DEC_MIN_KEYS = 128;       // a split covers at least this many cached rows (L <= 128: one split)

// The split count depends on the problem shape only (never on cap or on the data): results are reproducible bit for bit.
inline int dec_splits(int64_t bs, int64_t nkv, int64_t L) {
    int64_t ns = (DEC_TARGET_WG + bs * nkv - 1) / (bs * nkv);
    if (ns > DEC_MAX_SPLIT) ns = DEC_MAX_SPLIT;
    const int64_t by_len = (L + DEC_MIN_KEYS - 1) / DEC_MIN_KEYS;
    if (ns > by_len) ns = by_len;
    return ns < 1 ? 1 : (int)ns;
}

// Combine kernel: one workgroup of HD threads per (b, kv head, r); splits merged in split order, one rounding to T.
// Workspace per (b, kv head, split, r): [m, l, acc[HD]] with m in the log2 domain; a split that saw no row holds (-inf, 0).
template <typename T, int HD>
__global__ void __launch_bounds__(HD) attn_decode_combine_kernel(const float* ws, T* o, int64_t Tq, int nh, int nkv, int ns) {
    const int rep = nh / nkv;
    const int64_t R = (int64_t)rep * Tq;
    const int64_t row = blockIdx.x;
    const int64_t r = row % R, bk = row / R;
    const int64_t kvh = bk % nkv, b = bk / nkv;
    const int tid = threadIdx.x;
    const float* w = ws + (bk * ns * R + r) * (HD + 2);
    const int64_t st = R * (HD + 2);
    float M = -INFINITY;
    for (int s = 0; s < ns; ++s) M = fmaxf(M, w[s * st]);
    float l = 0.f, a = 0.f;
    for (int s = 0; s < ns; ++s) {
        const float ms = w[s * st];
        const float f = ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(ms - M);
        l += f * w[s * st + 1];
        a += f * w[s * st + 2 + tid];
    }
    const int64_t t = r / rep;
    st1(o + ((b * Tq + t) * nh + kvh * rep + (r % rep)) * HD + tid, a / l);
}

}  // namespace
