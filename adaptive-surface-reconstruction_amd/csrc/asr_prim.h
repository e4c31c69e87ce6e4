// asr_prim.h -- host helpers shared by the .hip translation units: counter flags, rocPRIM
// radix sort / scan wrappers running on the context stream with arena temporaries.
#pragma once
#include <rocprim/rocprim.hpp>

#include "asr_common.h"

namespace asr_prim {

// Device counters come in blocks of 64 ints out of a pool that is zeroed once: a pass that needs fresh counters takes the
// next block (fresh_flags) instead of clearing the one block there used to be -- twenty fill launches per geometry build,
// each a dependent launch in one of its two chains.  The pool is cleared again, on the context's stream, when it is used up.
constexpr int FLAG_BLOCK = 64, FLAG_BLOCKS = 512;
// The slots of a block, one per meaning (kernels: cnt[F_...], host: HostFlags[F_...]) and the passes that write them.
// read_flags copies the first FLAG_READ ints; the cell counts per level lie behind them and are copied by their reader.
enum Flag : int {
    F_ENTRIES = 0,         // octree / grow: entries of the node list (insert_with_ancestors, k_grow_init, k_grow_insert)
    F_OVERFLOW = 1,        // a hash table or list lost a key: octree, grow, key maps, cell table, mask set, dual-cell map
    F_MASKS = 2,           // row regrouping: number of distinct slot masks (k_rg_mask_collect)
    F_BAD_KEY = 3,         // bad location code (k_check_keys) / bad row list (k_check_rows)
    F_BAD_INDEX = 4,       // mesh: a corner index out of range (contour, components, simplify, sample, adjacency, fill_holes)
    F_BAD_LEVEL = 5,       // mesh simplify / points merge: a level out of range (k_simp_keys, k_merge_keys)
    F_LEVEL_MIN = 6,       // smallest / ...
    F_LEVEL_MAX = 7,       // ... largest query level (k_query_levels, k_attr_levels); initialised together
    F_POINT_LEVEL = 8,     // presort: finest level a point can be inserted on (k_finest_point_level)
    F_ROOT = 9,            // octree: the root was inserted (insert_with_ancestors)
    F_HEAVY = 10,          // radius search: number of heavy rows (k_radius_query)
    F_NONFINITE = 11,      // non-finite points / radii (k_octree_insert_points, k_grow_init, k_point_codes)
    F_KNN_CELLS = 12,      // kNN: occupied finest-level cells (k_cell_list) / ...
    F_KNN_FALLBACK = 13,   // ... points left to the wave-per-point kernel (k_knn_cells); cleared together
    F_MAX_CELL_POP = 14,   // kNN / nearest: largest population of a finest-level cell (k_max_cell_pop)
    F_MARGIN_PAIRS = 15,   // aligned radius search: pairs in the rounding margin (k_radius_extras, k_radius_query)
    F_DUAL_FAN = 16,       // contouring: more than 29 dual cells round an edge (k_contour_edges)
    F_DUAL_SORT = 17,      // contouring: cannot sort the duals round an edge (k_contour_edges)
    F_OUTSIDE = 18,        // mesh simplify: a vertex outside the frame or not finite (k_simp_keys)
    F_BAD_VERTEX = 19,     // mesh smooth / fill_holes: a vertex is not finite (k_smooth_load, k_fill_keys)
    F_KEY_BITS = 20,       // octree: bits of the longest key of the node list (k_list_key_bits)
    F_DUAL_KEY = 21,       // dual cells: no leaf found for a corner (k_dual_fill)
    F_CELLS = 22,          // cell table: cells of all counted levels (k_cell_bounds<true>)
    F_MERGE_DROPPED = 23,  // points merge: points that are not finite or lie outside the root cube (k_merge_keys)
    F_MERGE_SPLIT = 24,    // points merge: cells split into two sides (k_merge_cluster_heads)
    F_MERGE_CLUSTERS = 25, // points merge: clusters (k_merge_starts) / ...
    F_MERGE_LARGEST = 26,  // ... members of the largest one / ...
    F_MERGE_LONG = 27,     // ... clusters longer than ASR_MERGE_LONG_CLUSTER (k_merge_stats)
    F_ORIENT_SKIPPED = 28, // normal orientation: points with a zero normal (k_orient_init, k_orient_viewpoint)
    F_ORIENT_FLIPPED = 29, // ... flipped normals (k_orient_flips, k_orient_viewpoint)
    F_ORIENT_TREES = 30,   // ... trees of the spanning forest (k_orient_top)
    F_ORIENT_HOOKED = 31,  // ... roots hooked in all rounds so far (k_orient_hook)
    F_COUNT
};
constexpr int FLAG_READ = 32;        // ints read_flags copies to the host
constexpr int FLAG_LEVEL_CELLS = 32; // first of the ASR_MAX_LEVEL + 1 cell counts per level (k_cell_bounds<true>)
static_assert(F_COUNT <= FLAG_READ, "read_flags must cover every slot");
static_assert(FLAG_READ <= FLAG_LEVEL_CELLS && FLAG_LEVEL_CELLS + ASR_MAX_LEVEL + 1 <= FLAG_BLOCK,
              "the per-level cell counts lie behind the slots, inside the block");
static_assert(F_LEVEL_MAX == F_LEVEL_MIN + 1, "query_level_range sets both with one copy");
static_assert(F_KNN_FALLBACK == F_KNN_CELLS + 1, "asr_geom_knn clears both with one memset");
struct HostFlags {
    int v[FLAG_READ];
    int operator[](Flag f) const { return v[f]; }
};
static inline int ensure_flags(asr_hip_context* ctx) {
    if (!ctx->d_flags_base) {
        ASR_HIP_CHECK(ctx, hipMalloc((void**)&ctx->d_flags_base, (size_t)FLAG_BLOCK * FLAG_BLOCKS * sizeof(int)));
        ASR_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_flags_base, 0, (size_t)FLAG_BLOCK * FLAG_BLOCKS * sizeof(int), ctx->stream));
        ctx->d_flags = ctx->d_flags_base;
        ctx->flags_next = 1;
    }
    return ASR_HIP_OK;
}
// ctx->d_flags = a block of zeroed counters (what hipMemsetAsync(ctx->d_flags, 0, ...) used to give)
static inline int fresh_flags(asr_hip_context* ctx) {
    ASR_TRY(ensure_flags(ctx));
    if (ctx->flags_next >= FLAG_BLOCKS) {
        ASR_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_flags_base, 0, (size_t)FLAG_BLOCK * FLAG_BLOCKS * sizeof(int), ctx->stream));
        ctx->flags_next = 0;
    }
    ctx->d_flags = ctx->d_flags_base + (size_t)FLAG_BLOCK * ctx->flags_next++;
    return ASR_HIP_OK;
}
// How a _count call that keeps its work in the scratch arena starts: nothing is pending any more (asr_pending.h), the
// arena is recycled, the counters are fresh.  Before any early return, so that every count of an operator starts alike.
static inline int count_begin(asr_hip_context* ctx) {
    pending_begin(ctx->pending);
    ctx->scratch.reset();
    return fresh_flags(ctx);
}
// how a _count call that succeeded returns, the early returns for empty input included
static inline int count_done(asr_hip_context* ctx, PendingOp op) {
    pending_commit(ctx->pending, op, ctx->scratch.generation);
    return ASR_HIP_OK;
}
// _fill: false unless it completes the most recent successful count, `op`'s, in a scratch arena nobody has recycled
static inline bool fill_begin(asr_hip_context* ctx, PendingOp op) {
    return pending_claim(ctx->pending, op, ctx->scratch.generation);
}
// T* var = `count` elements of the context's scratch arena, or the function fails
#define SCRATCH_ALLOC(var, T, count)                        \
    T* var = arena_alloc<T>(ctx->scratch, (size_t)(count)); \
    if (!var) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed")
static inline int read_flags(asr_hip_context* ctx, HostFlags& host) {
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(host.v, ctx->d_flags, FLAG_READ * sizeof(int), hipMemcpyDeviceToHost,
                                      ctx->stream));
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ASR_HIP_OK;
}

static inline int sort_keys(asr_hip_context* ctx, Arena& arena, const u64* in, u64* out, i64 n, int end_bit = 64) {
    if (n <= 0) return ASR_HIP_OK;
    size_t tb = 0;
    ASR_HIP_CHECK(ctx, rocprim::radix_sort_keys(nullptr, tb, in, out, (size_t)n, 0, end_bit,
                                                ctx->stream));
    void* tmp = arena.alloc(tb ? tb : 256);
    if (!tmp) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, rocprim::radix_sort_keys(tmp, tb, in, out, (size_t)n, 0, end_bit,
                                                ctx->stream));
    return ASR_HIP_OK;
}
// stable LSD radix sort on key bits [begin_bit, end_bit)
template <class K, class V>
static inline int sort_pairs(asr_hip_context* ctx, Arena& arena, const K* kin, K* kout, const V* vin, V* vout,
               i64 n, int end_bit, int begin_bit = 0) {
    if (n <= 0) return ASR_HIP_OK;
    size_t tb = 0;
    ASR_HIP_CHECK(ctx, rocprim::radix_sort_pairs(nullptr, tb, kin, kout, vin, vout, (size_t)n, begin_bit,
                                                 end_bit, ctx->stream));
    void* tmp = arena.alloc(tb ? tb : 256);
    if (!tmp) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, rocprim::radix_sort_pairs(tmp, tb, kin, kout, vin, vout, (size_t)n, begin_bit,
                                                 end_bit, ctx->stream));
    return ASR_HIP_OK;
}
// out[0..n] = exclusive scan of in[0..n] (in has n+1 entries, in[n] ignored by callers that set it 0)
static inline int scan_counts(asr_hip_context* ctx, Arena& arena, const i64* in, i64* out, i64 n_plus_1) {
    size_t tb = 0;
    ASR_HIP_CHECK(ctx, rocprim::exclusive_scan(nullptr, tb, in, out, i64(0), (size_t)n_plus_1,
                                               rocprim::plus<i64>(), ctx->stream));
    void* tmp = arena.alloc(tb ? tb : 256);
    if (!tmp) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, rocprim::exclusive_scan(tmp, tb, in, out, i64(0), (size_t)n_plus_1,
                                               rocprim::plus<i64>(), ctx->stream));
    return ASR_HIP_OK;
}
// out[i] = in[0] + ... + in[i] in f64, summed in a fixed order (no look-back race): the same bits on every run
static inline int scan_f64_inclusive(asr_hip_context* ctx, Arena& arena, const double* in, double* out, i64 n) {
    if (n <= 0) return ASR_HIP_OK;
    size_t tb = 0;
    ASR_HIP_CHECK(ctx, rocprim::deterministic_inclusive_scan(nullptr, tb, in, out, (size_t)n, rocprim::plus<double>(),
                                                             ctx->stream));
    void* tmp = arena.alloc(tb ? tb : 256);
    if (!tmp) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, rocprim::deterministic_inclusive_scan(tmp, tb, in, out, (size_t)n, rocprim::plus<double>(),
                                                             ctx->stream));
    return ASR_HIP_OK;
}
static inline int read_i64(asr_hip_context* ctx, const i64* dev, i64* host) {
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(host, dev, sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ASR_HIP_OK;
}

static inline int bits_for(i64 n) {
    int b = 1;
    while ((i64(1) << b) < n) ++b;
    return b;
}


}  // namespace asr_prim
