// Page moves of the model-wide paged KV pool (kvcache.PagedKVPool): gather pages of every layer into a contiguous buffer
// (swap-out staging), scatter them back (swap-in) and copy pages inside the pool (fork's partial page, set_lengths' private
// copies).  A page of a buffer is one contiguous chunk of page_bytes per layer, layers are layer_stride_bytes apart, so a move
// is a pure 16-byte vector copy: no LDS, no atomics, no arithmetic on the data.  One launch serves all layers of a buffer kind.
// kv_tree_commit_kernel (oq_kv_tree_commit) moves ROWS instead: after a token tree was verified, the K/V rows of the accepted
// root path, scattered at lens[b] + node, become the sequence's next rows lens[b] + 0, 1, 2, ... in every layer.
#include "oq_common.h"
#include "oq_kv_dev.h"

namespace {

constexpr int MOVE_THREADS = 256;
constexpr int MOVE_UNROLL = 4;          // 16-byte vectors a lane keeps in flight per page slice
constexpr int64_t MOVE_MAX_GRID = 2048;  // 256 CUs x 8 workgroups; the rest is grid-strided

enum { MOVE_GATHER = 0, MOVE_SCATTER = 1, MOVE_COPY = 2 };

struct MoveP {
    const char* src;      // gather / copy: the pool; scatter: the contiguous [layers][n][page_bytes] buffer
    char* dst;            // gather: the contiguous buffer; scatter / copy: the pool
    const int32_t* ids;   // gather: source pages; scatter: destination pages; copy: source pages
    const int32_t* ids2;  // copy: destination pages
    int64_t num_pages, vpp, layer_stride, layers, n;
    int64_t spp;          // slices per page
    int64_t total;        // layers * n * spp page slices
    int group;            // lanes that share one page slice: a power of two, 8 .. MOVE_THREADS
};

// A page slice is `group` * MOVE_UNROLL consecutive vectors of one (layer, page): consecutive lanes take consecutive 16 bytes,
// so a wave moves 1 KiB contiguously per load.  Pages smaller than a workgroup's 4 KiB share it (MOVE_THREADS / group slices
// per workgroup).  The page id is loaded once per slice; an id outside [0, num_pages) skips the slice: nothing is loaded and
// nothing stored.  The four loads of a full slice are issued before its stores; a partial slice moves one vector at a time.
template <int MODE>
__global__ __launch_bounds__(MOVE_THREADS) void kv_pages_move_kernel(const MoveP p) {
    const int per_wg = MOVE_THREADS / p.group;
    const int sub = threadIdx.x / p.group, lane = threadIdx.x % p.group;
    const int64_t items = (p.total + per_wg - 1) / per_wg;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t ps = item * per_wg + sub;
        if (ps >= p.total) continue;
        const int64_t s = ps % p.spp, t = ps / p.spp;
        const int64_t i = t % p.n, l = t / p.n;
        const int64_t id = p.ids[i];
        if (id < 0 || id >= p.num_pages) continue;
        int64_t id2 = 0;
        if constexpr (MODE == MOVE_COPY) {
            id2 = p.ids2[i];
            if (id2 < 0 || id2 >= p.num_pages || id2 == id) continue;
        }
        const int64_t flat = (l * p.n + i) * p.vpp, pooled = l * p.layer_stride + id * p.vpp;
        const uint4* src = reinterpret_cast<const uint4*>(p.src) + (MODE == MOVE_SCATTER ? flat : pooled);
        uint4* dst = reinterpret_cast<uint4*>(p.dst) +
                     (MODE == MOVE_GATHER ? flat : (MODE == MOVE_SCATTER ? pooled : l * p.layer_stride + id2 * p.vpp));
        const int64_t v0 = s * p.group * MOVE_UNROLL + lane, g = p.group;
        src += v0;
        dst += v0;
        if (v0 + (MOVE_UNROLL - 1) * g < p.vpp) {
            // a full slice: four named registers (an indexed private array written under a condition is promoted to LDS)
            static_assert(MOVE_UNROLL == 4, "the full-slice path names four registers");
            const uint4 r0 = src[0], r1 = src[g], r2 = src[2 * g], r3 = src[3 * g];
            dst[0] = r0;
            dst[g] = r1;
            dst[2 * g] = r2;
            dst[3 * g] = r3;
        } else {
            // the tail of a page that is no multiple of the slice (and every page below group * 4 vectors): one vector at a time
            for (int64_t v = v0, o = 0; v < p.vpp; v += g, o += g) dst[o] = src[o];
        }
    }
}

template <int MODE>
int kv_pages_move(const char* fn, const void* src, void* dst, int64_t num_pages, int64_t page_bytes, int64_t layer_stride_bytes,
                  int64_t layers, const int32_t* ids, const int32_t* ids2, int64_t n, void* stream) {
    OQ_CHECK_ARG(num_pages >= 0 && page_bytes >= 0 && layer_stride_bytes >= 0 && layers >= 0 && n >= 0,
                 "%s: negative size (num_pages %lld, page_bytes %lld, layer_stride_bytes %lld, layers %lld, n %lld)", fn,
                 (long long)num_pages, (long long)page_bytes, (long long)layer_stride_bytes, (long long)layers, (long long)n);
    OQ_CHECK_ARG(page_bytes > 0 && page_bytes % 16 == 0, "%s: page_bytes %lld must be a positive multiple of 16", fn,
                 (long long)page_bytes);
    if (n == 0 || layers == 0) return OQ_OK;
    OQ_CHECK_ARG(src && dst && ids && (MODE != MOVE_COPY || ids2), "%s: null pointer with n = %lld", fn, (long long)n);
    OQ_CHECK_ARG(num_pages > 0, "%s: num_pages 0", fn);
    OQ_CHECK_ARG(layer_stride_bytes % 16 == 0 && (layers == 1 || layer_stride_bytes >= num_pages * page_bytes),
                 "%s: layer_stride_bytes %lld (a multiple of 16, at least num_pages * page_bytes = %lld)", fn,
                 (long long)layer_stride_bytes, (long long)(num_pages * page_bytes));
    OQ_CHECK_ARG(oq_aligned16(src) && oq_aligned16(dst), "%s: the pool and the buffer must be 16-byte aligned", fn);
    OQ_CHECK_ARG((uintptr_t)ids % 4 == 0 && (uintptr_t)ids2 % 4 == 0, "%s: page ids (int32 on the device)", fn);
    MoveP p;
    p.src = static_cast<const char*>(src);
    p.dst = static_cast<char*>(dst);
    p.ids = ids;
    p.ids2 = ids2;
    p.num_pages = num_pages;
    p.vpp = page_bytes / 16;
    p.layer_stride = layer_stride_bytes / 16;
    p.layers = layers;
    p.n = n;
    int group = 8;
    while (group < MOVE_THREADS && group < p.vpp) group *= 2;
    p.group = group;
    p.spp = (p.vpp + (int64_t)group * MOVE_UNROLL - 1) / ((int64_t)group * MOVE_UNROLL);
    p.total = layers * n * p.spp;
    const int per_wg = MOVE_THREADS / group;
    const int64_t items = (p.total + per_wg - 1) / per_wg;
    const int64_t grid = items < MOVE_MAX_GRID ? items : MOVE_MAX_GRID;
    hipLaunchKernelGGL((kv_pages_move_kernel<MODE>), dim3((unsigned)grid), dim3(MOVE_THREADS), 0, (hipStream_t)stream, p);
    OQ_CHECK_LAUNCH(fn);
    return OQ_OK;
}

// ---- committing the accepted path of a token tree ---------------------------------------------------------------------------
struct CommitP {
    char* buf;                          // slab [layers][bs][nkv][cap][row_bytes] or pools [layers][num_pages][nkv][PS][row_bytes]
    const int32_t* lens;                // [bs]
    const int32_t* accept;              // [bs][Tq]: accepted node ids in path order, padded with -1
    PageMap pm;
    int64_t row_bytes, layer_stride, cap, total;
    int bs, nkv, Tq, cols;              // cols: vectors of V per row
};

// One thread owns one byte column (sizeof(V) bytes) of the rows of one (layer, sequence, kv head) and does that column's moves
// row lens[b] + accept[b][i] -> row lens[b] + i in ASCENDING i.  That order is what makes the in-place compaction safe: an
// entry is valid only if i <= a < Tq and a lies strictly above the previous entry, so destination i can be the source of an
// earlier move of the same thread (already read, and a thread's own loads and stores to one address keep program order) and
// never of a later one.  No thread touches another's column, so there is no ordering between threads to keep.  The first
// invalid entry ends the walk; a source or destination row outside [0, cap), or in a page the table does not hold, skips that
// move alone (the append kernel's rule: never clamped onto another row).
template <typename V>
__global__ __launch_bounds__(MOVE_THREADS) void kv_tree_commit_kernel(const CommitP p) {
    const int64_t gid = (int64_t)blockIdx.x * MOVE_THREADS + threadIdx.x;
    if (gid >= p.total) return;
    const int col = (int)(gid % p.cols);
    int64_t t = gid / p.cols;
    const int kvh = (int)(t % p.nkv);
    t /= p.nkv;
    const int64_t b = t % p.bs, layer = t / p.bs;
    const int64_t len = p.lens[b];
    const int32_t* acc = p.accept + b * p.Tq;
    const int32_t* tab = p.pm.table ? p.pm.table + b * p.pm.max_pages : nullptr;
    char* base = p.buf + layer * p.layer_stride;
    // the buffer row of logical row j of (b, kvh), or -1
    auto locate = [&](int64_t j) -> int64_t {
        if (j < 0 || j >= p.cap) return -1;
        if (tab) {
            const int64_t page = tab[j >> p.pm.lg];
            if (page < 0 || page >= p.pm.num_pages) return -1;
            return ((page * p.nkv + kvh) << p.pm.lg) + (j & ((int64_t(1) << p.pm.lg) - 1));
        }
        return (b * p.nkv + kvh) * p.cap + j;
    };
    int prev = -1;
    for (int i = 0; i < p.Tq; ++i) {
        const int a = acc[i];
        if (a < i || a >= p.Tq || a <= prev) break;
        prev = a;
        if (a == i) continue;
        const int64_t src = locate(len + a), dst = locate(len + i);
        if (src < 0 || dst < 0) continue;
        const V x = reinterpret_cast<const V*>(base + src * p.row_bytes)[col];
        reinterpret_cast<V*>(base + dst * p.row_bytes)[col] = x;
    }
}

}  // namespace

extern "C" {

int oq_kv_tree_commit(void* buf, int64_t row_bytes, int64_t layers, int64_t layer_stride_bytes, int64_t bs, int nkv, int64_t cap,
                      const int32_t* table, int64_t max_pages, int64_t num_pages, int page_size, const int32_t* lens,
                      const int32_t* accept, int64_t Tq, void* stream) {
    const char* fn = "oq_kv_tree_commit";
    OQ_CHECK_ARG(row_bytes > 0 && row_bytes % 4 == 0 && row_bytes <= 4096, "%s: row_bytes %lld (a multiple of 4, at most 4096)", fn,
                 (long long)row_bytes);
    OQ_CHECK_ARG(layers >= 0 && layer_stride_bytes >= 0 && bs > 0 && bs <= 65535 && nkv > 0 && nkv <= 65535,
                 "%s: layers %lld, layer_stride_bytes %lld, bs %lld, nkv %d", fn, (long long)layers, (long long)layer_stride_bytes,
                 (long long)bs, nkv);
    OQ_CHECK_ARG(Tq >= 1 && Tq <= 64, "%s: Tq %lld (a token tree has 1 to 64 nodes)", fn, (long long)Tq);
    if (layers == 0) return OQ_OK;
    OQ_CHECK_ARG(buf && lens && accept, "%s: null pointer", fn);
    OQ_CHECK_ARG((uintptr_t)lens % 4 == 0 && (uintptr_t)accept % 4 == 0, "%s: lens and accept are int32 on the device", fn);
    PageMap pm = NO_PAGES;
    int64_t layer_bytes;
    if (table) {
        if (const int rc = page_map(fn, table, max_pages, num_pages, page_size, &pm, &cap)) return rc;
        layer_bytes = num_pages * nkv * page_size * row_bytes;
    } else {
        OQ_CHECK_ARG(cap > 0 && cap < (int64_t(1) << 40), "%s: cap %lld", fn, (long long)cap);
        layer_bytes = bs * nkv * cap * row_bytes;
    }
    OQ_CHECK_ARG(layers == 1 || layer_stride_bytes >= layer_bytes, "%s: layer_stride_bytes %lld below one layer (%lld bytes)", fn,
                 (long long)layer_stride_bytes, (long long)layer_bytes);
    // the widest vector the row size, the layer stride and the buffer's alignment allow
    const uint64_t al = (uint64_t)row_bytes | (layers > 1 ? (uint64_t)layer_stride_bytes : 0) | (uint64_t)(uintptr_t)buf;
    const int vw = al % 16 == 0 ? 16 : (al % 8 == 0 ? 8 : 4);
    OQ_CHECK_ARG(al % 4 == 0, "%s: buf and layer_stride_bytes must be multiples of 4 bytes", fn);
    CommitP p;
    p.buf = static_cast<char*>(buf);
    p.lens = lens;
    p.accept = accept;
    p.pm = pm;
    p.row_bytes = row_bytes;
    p.layer_stride = layer_stride_bytes;
    p.cap = cap;
    p.bs = (int)bs;
    p.nkv = nkv;
    p.Tq = (int)Tq;
    p.cols = (int)(row_bytes / vw);
    p.total = layers * bs * nkv * p.cols;
    const int64_t grid = (p.total + MOVE_THREADS - 1) / MOVE_THREADS;
    OQ_CHECK_ARG(grid < (int64_t(1) << 31), "%s: too many workgroups", fn);
    hipStream_t st = (hipStream_t)stream;
    if (vw == 16) hipLaunchKernelGGL((kv_tree_commit_kernel<uint4>), dim3((unsigned)grid), dim3(MOVE_THREADS), 0, st, p);
    else if (vw == 8) hipLaunchKernelGGL((kv_tree_commit_kernel<uint2>), dim3((unsigned)grid), dim3(MOVE_THREADS), 0, st, p);
    else hipLaunchKernelGGL((kv_tree_commit_kernel<uint32_t>), dim3((unsigned)grid), dim3(MOVE_THREADS), 0, st, p);
    OQ_CHECK_LAUNCH(fn);
    return OQ_OK;
}

int oq_kv_pages_gather(const void* pool, int64_t num_pages, int64_t page_bytes, int64_t layer_stride_bytes, int64_t layers,
                       const int32_t* page_ids, int64_t n, void* dst, void* stream) {
    return kv_pages_move<MOVE_GATHER>("oq_kv_pages_gather", pool, dst, num_pages, page_bytes, layer_stride_bytes, layers, page_ids,
                                      nullptr, n, stream);
}

int oq_kv_pages_scatter(const void* src, void* pool, int64_t num_pages, int64_t page_bytes, int64_t layer_stride_bytes,
                        int64_t layers, const int32_t* page_ids, int64_t n, void* stream) {
    return kv_pages_move<MOVE_SCATTER>("oq_kv_pages_scatter", src, pool, num_pages, page_bytes, layer_stride_bytes, layers, page_ids,
                                       nullptr, n, stream);
}

int oq_kv_pages_copy(void* pool, int64_t num_pages, int64_t page_bytes, int64_t layer_stride_bytes, int64_t layers,
                     const int32_t* src_ids, const int32_t* dst_ids, int64_t n, void* stream) {
    return kv_pages_move<MOVE_COPY>("oq_kv_pages_copy", pool, pool, num_pages, page_bytes, layer_stride_bytes, layers, src_ids, dst_ids,
                                    n, stream);
}

}  // extern "C"
