// asr_common.h -- context, device arena and shared device helpers (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/asr_hip.h"
#include "asr_pending.h"

typedef uint64_t u64;
typedef int64_t i64;
typedef uint32_t u32;

// ---------------------------------------------------------------------------------------
// Device arena: a list of hipMalloc'd slabs with bump allocation.  reset() rewinds the bump
// pointers but keeps the slabs, so steady-state forwards do not call hipMalloc.
// ---------------------------------------------------------------------------------------
struct Arena {
    struct Slab {
        char* base;
        size_t size, used;
    };
    std::vector<Slab> slabs;
    size_t min_slab = size_t(256) << 20;
    size_t cap = 0;  // option "arena_cap_mb": the arena never reserves more than this many bytes (0: no limit)
    uint64_t generation = 0;  // resets and rewinds so far: older pointers may have been handed out again (asr_pending.h)

    void* alloc(size_t bytes) {
        bytes = (bytes + 255) & ~size_t(255);
        if (bytes == 0) bytes = 256;
        for (auto& s : slabs)
            if (s.size - s.used >= bytes) {
                void* p = s.base + s.used;
                s.used += bytes;
                return p;
            }
        size_t sz = bytes > min_slab ? bytes : min_slab;
        if (cap && reserved() + sz > cap) return nullptr;
        void* p = nullptr;
        if (hipMalloc(&p, sz) != hipSuccess) return nullptr;
        slabs.push_back({(char*)p, sz, bytes});
        return p;
    }
    void reset() {
        for (auto& s : slabs) s.used = 0;
        ++generation;
    }
    size_t reserved() const {
        size_t t = 0;
        for (auto& s : slabs) t += s.size;
        return t;
    }
    void release() {
        for (auto& s : slabs) (void)hipFree(s.base);
        slabs.clear();
    }
};

// mark/rewind: remembers the bump pointers of an arena
struct ArenaMark {
    std::vector<size_t> used;
};
static inline void arena_mark(const Arena& a, ArenaMark& m) {
    m.used.clear();
    for (auto& s : a.slabs) m.used.push_back(s.used);
}
static inline void arena_rewind(Arena& a, const ArenaMark& m) {
    for (size_t i = 0; i < a.slabs.size(); ++i) a.slabs[i].used = i < m.used.size() ? m.used[i] : 0;
    ++a.generation;
}

struct GridDev {
    i64 v = 0;
    u64* keys = nullptr;
    float* centers = nullptr;
    float* sizes = nullptr;
};  // its neighbour lists: asr_hip_context::same / up / down

// Tunables of one context (asr_hip_context_set_option); the defaults can also be seeded from the
// environment (ASR_SCONV_MIN_BLOCKS, ...) when the context is created, for experiments.
struct AsrOptions {
    i64 sconv_min_blocks = 2816;  // narrow the column tile until a launch has this many blocks (11 per CU)
    i64 sconv16_min_blocks = 1024;  // the same for the 16-bit kernels (4 per CU: every column chunk of a tile gathers the
                                    // features again, and these kernels are bound by the load path on the small grids)
    i64 sconv_wide_min = 2048;    // 8-wave (128-row) blocks when they still give this many blocks
    i64 row_segment = 524288;     // rows are regrouped inside segments of this many consecutive rows
    i64 search_hash_level = -1;   // >= 0: finest level of the search's cell hash table (finer: binary search); tests
    i64 knn_deep = 1;             // kNN radius: finer start levels for the points of crowded cells (0: off)
    i64 knn_cells = 1;            // kNN radius: cell-parallel fast path (0: wave per point only)
    i64 plan_arena = 0;           // asr_hip_sparse_conv_plan_create: 1 = memory from the context's plan arena (no hipMalloc /
                                  // hipFree per plan; all such plans die with asr_hip_context_plan_arena_reset)
    i64 sconv_plan = 1;           // 16-bit sparse conv: plan-driven kernel where it applies (0: table-driven)
    i64 row_ranked = 1;           // row regrouping: sort on (job, segment, rank of the slot mask) keys, all lists in one sort
    i64 row_lpt = 1;              // longest-first order of the 128-row chunks of a segment
    i64 overlap = 1;              // aggregation search on the auxiliary stream, overlapped with the grids
    i64 cconv_valu = 0;           // 1: whole-path continuous conv with the VALU contraction (k_cconv) instead of k_cconv_mfma
    i64 build_search = 1;         // 0: implicit_build stops after the grids (sharded runs search their own rows)
    i64 shard_geometry = -1;      // sharded forward: 1 = lists / plans / search for the owned voxels only, 0 = whole cloud on every rank, -1 = 1 whenever world > 1
    i64 shard_timing = 0;         // sharded forward: synchronise around every halo exchange and accumulate its wall time
    i64 search_priority = 2;      // priority of the search's stream (set before the first build): 0 lowest, 1 middle, 2 highest
                                  // (round 4: the search is the longer of the two chains; 9.6 -> 8.8 ms on its stream)
    i64 search_half = 1;          // aggregation search: 4^3 half-size cells per voxel (0: 3^3 full-size cells)
    i64 early_cells = 1;            // ... and its cell table, on the search thread
    i64 early_sort = 1;           // overlapped search: its point sort starts on the auxiliary stream beside the octree build
    // 16-bit sparse conv, 55-slot lists whose INPUT grid has between these many rows (the coarse levels: a handful of
    // tiles, the longest of which runs its 30 slots x cin / 32 steps alone on its CU): the slots are cut into five fixed
    // ranges, every (tile, range) is a block of its own, a second kernel adds the partial sums in range order.  The
    // choice depends on the input grid's size only, so that one rank of a sharded cloud makes the same one.
    i64 arena_cap_mb = 0;         // > 0: each device arena of the context (results, scratch, shard state) stops growing at this
                                  // many MiB and the call fails with "arena allocation failed" instead (memory budget per rank)
    i64 inject_failure = 0;       // fault injection for the tests of the sharded forward's error agreement: 1 = the build of this
                                  // rank fails, 2 = its network preparation fails (the call RETURNS AN ERROR, nothing is skipped)
    i64 sconv_split_min_rows = 2048;
    i64 sconv_split_rows = 32768;  // 0: never
};

// Row-group plan of a neighbour list for the plan-driven 16-bit sparse conv (asr_conv16.hip): per 16
// consecutive rows (row_perm order) the set of kernel slots in use and, slot by slot, the 16 neighbour indices.
struct asr_conv_plan_view {
    const uint4* hdr;      // [groups_pad] {slot mask lo, hi, first pool block, 0}
    const int32_t* pool;   // [blocks][16], -1: no neighbour
    i64 groups;            // ceil(num_out / 16)
    unsigned pool_bytes;
};
// the rows a convolution computes: a neighbour list and the order its rows are tiled in
struct asr_conv_rows {
    const int32_t* nidx = nullptr;
    const uint8_t* kidx = nullptr;
    const i64* rs = nullptr;
    const int32_t* perm = nullptr;  // tiling order (asr_geom_row_groups_batch): num_out rows of the list, or null
    i64 num_out = 0;
    int K = 0;
};
// ... and their plan (hdr == nullptr: none was built)
struct asr_conv_plan : asr_conv_rows {
    uint4* hdr = nullptr;
    int32_t* pool = nullptr;
    i64 groups = 0, groups_pad = 0, blocks = 0;
    i64* offs = nullptr;  // [groups_pad + 1] first pool block of every group; offs[groups_pad] = blocks (device)
    bool usable() const { return hdr && blocks * 64 < (i64(1) << 32) - 65536; }
    asr_conv_plan_view view() const { return {hdr, pool, groups, (unsigned)(blocks * 64)}; }
};
// One of the 13 neighbour lists of a grid hierarchy, with the plan of ALL its rows.  Grid i has a 55-slot list over itself
// (same), a 9-slot list that reads the next coarser grid (up) and that list inverted (down: its rows are grid i + 1).
constexpr int ASR_NUM_LISTS = 3 * ASR_NUM_GRIDS - 2;
struct NbList : asr_conv_plan {
    enum Kind { SAME, UP, DOWN };
    int id = 0;  // position in asr_hip_context::lists
    Kind kind = SAME;
    int lvl_out = 0, lvl_in = 0;  // grid of the rows, grid of the inputs
    i64 num_inp = 0, pairs = 0;
};

// Points of the last implicit_build in Morton order (asr_geom_presort): shared by the octree insertion (neighbouring
// lanes then carry the same key: one table probe per run) and by the aggregation search.
struct AsrPointIndex {
    bool valid = false;
    const float* pts = nullptr;
    const float* radii = nullptr;
    i64 n = 0;
    int lsort = 0;               // sorted on the code bits down to this level
    float4* sorted = nullptr;    // (x, y, z, original index bits)
    int32_t* ids = nullptr;      // original index per Morton position
    int32_t* rank = nullptr;     // Morton position per original index
    float* srad = nullptr;       // radii in Morton order
    u64* codes = nullptr;        // sorted level-21 codes
    // cell table of the levels [tab_lmin, tab_lmax] built ahead of the query (asr_geom_precells), or tab_keys == nullptr
    u64* tab_keys = nullptr;
    u64 tab_mask = 0;
    int32_t* tab_start = nullptr;
    int32_t* tab_end = nullptr;
    int tab_lmin = 0, tab_lmax = -1, tab_lhash = 0, tab_grow = 0;
};

// asr_hip_points_merge_count -> _fill: the caller's inputs and the sorted member lists in the scratch arena
struct AsrMergeState {
    const float *points = nullptr, *normals = nullptr, *radii = nullptr, *attributes = nullptr;
    int channels = 0;
    i64 n = 0, clusters = 0, num_long = 0;
    const u64* keys = nullptr;            // sorted keys, 0 for the dropped points in front
    const int32_t* ids = nullptr;         // input index per sorted position, each cluster's members in ascending order
    const i64* offsets = nullptr;         // exclusive scan of the cluster heads (n + 1)
    const i64* starts = nullptr;          // first sorted position of every cluster (clusters + 1)
    const int32_t* long_list = nullptr;   // clusters of more than ASR_MERGE_LONG_CLUSTER members, any order
};

struct asr_hip_context {
    hipStream_t stream = nullptr;
    hipEvent_t switch_ev = nullptr;  // asr_hip_context_set_stream: recorded on the old stream, awaited by the new one
    std::string err;
    AsrOptions opt;
    std::map<std::string, i64> sconv_launches;  // "NT,KC,IMP,WAVES,DUAL" -> launches (asr_hip_sparse_conv_variant_counts)
    ArenaMark build_mark;                         // persist arena right after implicit_build
    bool build_mark_ok = false;
    Arena persist;  // results that outlive a call (octree, grids, values)
    Arena scratch;  // temporaries
    Arena plan_arena;  // row-group plans created with option "plan_arena" (asr_hip_context_plan_arena_reset)
    uint64_t plan_arena_epoch = 0;  // generation of plan_arena: plans of an earlier generation are refused
    // last octree
    u64* nodes = nullptr;
    u64* leaves = nullptr;
    i64 num_nodes = 0, num_leaves = 0;
    // last implicit build
    asr_octree_frame frame;
    asr_implicit_sizes sizes;
    GridDev grids[ASR_NUM_GRIDS];
    NbList lists[ASR_NUM_LISTS];  // per grid i: same(i), up(i), down(i) -- the last grid has no coarser one
    NbList& same(int i) { return lists[3 * i]; }
    NbList& up(int i) { return lists[3 * i + 1]; }
    NbList& down(int i) { return lists[3 * i + 2]; }
    asr_hip_context() { reset_lists(); }
    void reset_lists() {  // what every build starts with: no arrays, no plans
        for (int j = 0; j < ASR_NUM_LISTS; ++j) {
            NbList& l = lists[j] = NbList();
            l.id = j;
            l.kind = NbList::Kind(j % 3);
            l.K = l.kind == NbList::SAME ? 55 : 9;
            l.lvl_out = j / 3 + (l.kind == NbList::DOWN);
            l.lvl_in = j / 3 + (l.kind == NbList::UP);
        }
    }
    int32_t* agg_idx = nullptr;
    float* agg_dist = nullptr;
    float* agg_compat = nullptr;
    i64* agg_rs = nullptr;
    int32_t* agg_spos = nullptr;         // neighbour of each aggregation pair as a position in Morton order
    const float4* agg_sorted = nullptr;  // points in Morton order (x, y, z, original index bits)
    bool has_search = false;             // the last implicit_build ran the aggregation search
    // the last implicit_build was ONE RANK's build of a sharded cloud (asr_hip_implicit_forward_sharded, option shard_geometry):
    // 55-slot lists, plans and the aggregation CSR hold the owned rows only -- the stand-alone network entry points refuse it
    bool build_sharded = false;
    // sharded geometry: the search covered agg_nq (> 0) rows of grid 0 only -- agg_rows lists them, the CSR above and
    // the query centres / sizes below are compact over that list
    const int32_t* agg_rows = nullptr;
    i64 agg_nq = 0;
    const float* agg_qcenters = nullptr;
    const float* agg_qsizes = nullptr;
    AsrPointIndex pindex;                // asr_geom_presort
    i64 shard_prefix_hint = 0;           // rows of the importance prefix the last sharded build needed
    int search_extras = 0;               // pairs the last aligned search took from the rounding margin (diagnostic)
    const u64* nb_grow_keys = nullptr;   // asr_geom_grid_neighbors_count: the keys of the last call, their number and the
    i64 nb_grow_v = 0;                   // enlargement (log2) its key map needed -- the next _fill call on these keys starts
                                         // there and clears the note (nb_grow_keys == nullptr: none)
    int nb_grow = 0;
    i64 table_regrows = 0;               // hash tables rebuilt larger after an overflow since the context exists (diagnostic)
    int leaf_lmin = -1, leaf_lmax = -1;  // levels of the first / last leaf of the last octree
    float* values = nullptr;
    float* feats1 = nullptr;
    int feats1_width = 0;
    float* importance = nullptr;
    float* code = nullptr;
    // asr_hip_implicit_query: `code` holds every grid-0 row of the last forward (false after a build alone, a failed or a
    // sharded forward), code_width its columns, code_scale_sdf that forward's scale_sdf
    bool code_ok = false;
    int code_width = 0;
    int code_scale_sdf = 0;
    float stage_ms[6] = {0, 0, 0, 0, 0, 0};
    hipEvent_t ev[8] = {};
    bool ev_ok = false;
    int* d_flags = nullptr;  // the CURRENT block of 64 device counters: a window into d_flags_base (asr_prim.h fresh_flags)
    int* d_flags_base = nullptr;  // pool of zeroed counter blocks, re-zeroed with ONE memset when it is used up
    int flags_next = 0;
    float* d_zeros = nullptr;  // 4 KB of zeros: target of masked-out loads
    float* split_part = nullptr;   // partial sums of the slot-range split of the 16-bit sparse conv (grown on demand)
    size_t split_part_bytes = 0;
    unsigned* d_status = nullptr;  // sharded forward: the status word of asr_shard_agree
    unsigned* d_absmax = nullptr;  // f16x2: running maxima of the network's activation buffers; [255]: one-off inputs
    Pending pending;               // which _count may be filled, under which generation of `scratch` (asr_pending.h)
    void* geom_state = nullptr;    // what that count parked: GeomState of asr_geom.hip (radius search, dual cells),
    void* mesh_state = nullptr;    // MeshState of asr_mesh.hip (contour, components, simplify, edge table, fill holes),
    AsrMergeState merge;           // asr_points.hip.  The auxiliary context has a slot and states of its own.
    std::map<std::string, std::pair<const void*, size_t>> named;  // asr_hip_implicit_get
    int device = 0;                 // HIP device of this context (helper threads must select it)
    asr_hip_context* aux = nullptr;  // second stream + arenas: the aggregation search runs there, overlapped
                                    // with the grid hierarchy build (asr_api.hip implicit_build)
    bool aux_stream_owned = false;
    hipEvent_t aux_ev = nullptr;
    hipEvent_t aux_t0 = nullptr, aux_t1 = nullptr;  // search start / end on the auxiliary stream
    bool search_overlapped = false;
    // packed 16-bit copies of the weight tensors of the whole-path driver, keyed by (pointers of the f32 tensors
    // of both banks, their shapes, mode).  A weight table is immutable while a context holds packed copies of it:
    // callers that update weights in place call asr_hip_context_weights_changed (the copies are made again).
    typedef std::tuple<const void*, const void*, i64, i64, i64, i64, int> PackedKey;
    std::map<PackedKey, void*> packed_weights;
    Arena shard_mem;  // ownership, halo lists and plans of the sharded forward (reset per forward, kept across)
    unsigned* shard_stage_send = nullptr;  // message staging of the halo exchanges (grow-only)
    unsigned* shard_stage_recv = nullptr;
    size_t shard_stage_cap = 0;  // dwords each
    struct asr_shard_state* shard = nullptr;  // set while asr_hip_implicit_forward_sharded runs its network half
    // preparation pass of the sharded network (asr_api.hip implicit_network, phase 1): every argument check, weight packing
    // and allocation of a convolution happens, the kernel launch and the halo exchange do not
    bool dry_launch = false;
};

#define ASR_FAIL(ctx, code, ...)                         \
    do {                                                 \
        char _b[512];                                    \
        snprintf(_b, sizeof(_b), __VA_ARGS__);           \
        (ctx)->err = _b;                                 \
        return (code);                                   \
    } while (0)

#define ASR_HIP_CHECK(ctx, expr)                                                            \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            ASR_FAIL(ctx, ASR_HIP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                     __FILE__, __LINE__);                                                   \
    } while (0)

#define ASR_CHECK_LAUNCH(ctx) ASR_HIP_CHECK(ctx, hipGetLastError())

#define ASR_TRY(expr)               \
    do {                            \
        int _r = (expr);            \
        if (_r != ASR_HIP_OK) return _r; \
    } while (0)

static inline int asr_ctx_zeros(asr_hip_context* ctx, const float** out) {
    if (!ctx->d_zeros) {
        ASR_HIP_CHECK(ctx, hipMalloc((void**)&ctx->d_zeros, 4096));
        ASR_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_zeros, 0, 4096, ctx->stream));
    }
    *out = ctx->d_zeros;
    return ASR_HIP_OK;
}

template <class T>
static inline T* arena_alloc(Arena& a, size_t count) {
    return (T*)a.alloc(count * sizeof(T));
}

static inline unsigned grid_for(i64 n, int block) {
    i64 g = (n + block - 1) / block;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// ---------------------------------------------------------------------------------------
// device helpers: Morton / location codes (cpp/lib/zindex.h, octreebase.h)
// ---------------------------------------------------------------------------------------
__host__ __device__ static inline u64 asr_dilate21(u64 x) {
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x00FF0000FF0000FFull;
    x = (x | (x << 8)) & 0xF00F00F00F00F00Full;
    x = (x | (x << 4)) & 0x30C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x9249249249249249ull;
    return x;
}
__host__ __device__ static inline u64 asr_compact21(u64 x) {
    x &= 0x1249249249249249ull;
    x = ((x >> 2) | x) & 0x30C30C30C30C30C3ull;
    x = ((x >> 4) | x) & 0xF00F00F00F00F00Full;
    x = ((x >> 8) | x) & 0x00FF0000FF0000FFull;
    x = ((x >> 16) | x) & 0x001F00000000FFFFull;
    x = ((x >> 32) | x) & 0x00000000001FFFFFull;
    return x;
}
__host__ __device__ static inline u64 asr_morton3d(u64 x, u64 y, u64 z) {
    return asr_dilate21(x) | (asr_dilate21(y) << 1) | (asr_dilate21(z) << 2);
}
__device__ static inline int asr_key_level(u64 key) { return (63 - __clzll((long long)key)) / 3; }
// key of (x,y,z,lev) or 0 if outside the level's cube (octreebase.h:59-65,120-128)
__device__ static inline u64 asr_coord_key(int x, int y, int z, int lev) {
    int lim = 1 << lev;
    if (lev > ASR_MAX_LEVEL || x < 0 || x >= lim || y < 0 || y >= lim || z < 0 || z >= lim)
        return 0;
    return asr_morton3d((u64)x, (u64)y, (u64)z) | (u64(1) << (3 * lev));
}
__device__ static inline void asr_key_coord(u64 key, int& x, int& y, int& z, int& lev) {
    lev = asr_key_level(key);
    u64 k = key & ~(u64(1) << (3 * lev));
    x = (int)asr_compact21(k);
    y = (int)asr_compact21(k >> 1);
    z = (int)asr_compact21(k >> 2);
}

// point -> integer cell of `level` in the frame (octree.h:49-66, Octree::ComputeCoord).  Translation units that use it
// are compiled with -ffp-contract=off (csrc/Makefile GEOM_FLAGS), so that every caller rounds like the reference.
__device__ static inline void frame_coord(const asr_octree_frame& f, float px, float py, float pz,
                                          int level, int& x, int& y, int& z) {
    float inv = f.inv_voxel_size[ASR_MAX_LEVEL];
    float tx = px * inv, ty = py * inv, tz = pz * inv;
    x = (int)floorf(tx) + f.offset[0];
    y = (int)floorf(ty) + f.offset[1];
    z = (int)floorf(tz) + f.offset[2];
    int s = ASR_MAX_LEVEL - level;
    x >>= s;
    y >>= s;
    z >>= s;
}
// frame_coord at level 21 for an arbitrary point: false (and no int conversion) unless all three cells lie in
// [0, 2^21) -- non-finite and huge inputs are rejected by the float comparisons.  Equal to frame_coord where true.
__device__ static inline bool frame_coord21_checked(const asr_octree_frame& f, float px, float py, float pz, int& x,
                                                    int& y, int& z) {
    float inv = f.inv_voxel_size[ASR_MAX_LEVEL];
    float tx = floorf(px * inv), ty = floorf(py * inv), tz = floorf(pz * inv);
    const float lim = (float)(1 << ASR_MAX_LEVEL);
    if (!(tx >= (float)-f.offset[0] && tx < lim - (float)f.offset[0] && ty >= (float)-f.offset[1] &&
          ty < lim - (float)f.offset[1] && tz >= (float)-f.offset[2] && tz < lim - (float)f.offset[2]))
        return false;
    x = (int)tx + f.offset[0];
    y = (int)ty + f.offset[1];
    z = (int)tz + f.offset[2];
    return true;
}

// 64-bit finaliser (murmur3 fmix64) used by all device hash tables
__device__ static inline u64 asr_hash64(u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

int asr_ctx_ensure_aux(asr_hip_context* ctx);  // the search's auxiliary context + stream (asr_api.hip)
// one scan over several GPUs (asr_shard.hip): ownership, owned row lists / plans, halo lists of the 13 neighbour lists
// of the last implicit_build; hooks of the network driver
struct asr_shard_state;
int asr_shard_build(asr_hip_context* ctx, const asr_shard_comm* comm, int want_plans, asr_shard_state** out);
// the same in two steps for a rank that builds the 55-slot lists of its own rows only (by_pairs 0: equal voxel counts)
int asr_shard_ownership(asr_hip_context* ctx, const asr_shard_comm* comm, int by_pairs, asr_shard_state** out);
int asr_shard_ownership_coarser(asr_hip_context* ctx, asr_shard_state* st);
const int32_t* asr_shard_owner(const asr_shard_state* st, int level);
int asr_shard_halos(asr_hip_context* ctx, asr_shard_state* st, int want_plans);
const int32_t* asr_shard_level_rows(const asr_shard_state* st, int level, i64* n);
int asr_shard_query_rows(asr_hip_context* ctx, const asr_shard_state* st, i64 prefix, Arena& keep, int32_t** rows_out,
                         i64* n_out);
int asr_shard_world(const asr_shard_state* st);
int asr_shard_rank(const asr_shard_state* st);
void asr_shard_free(asr_shard_state* st);
void asr_shard_release(asr_hip_context* ctx);  // the context's shard arena and staging buffers
const asr_shard_stats* asr_shard_get_stats(const asr_shard_state* st);
// all ranks learn whether ANY rank failed so far (one MAX all-reduce of a status word): rc_local when this rank failed,
// ASR_HIP_EPEER when only others did, ASR_HIP_OK when nobody did
int asr_shard_agree(asr_hip_context* ctx, const asr_shard_comm* comm, int rc_local, const char* phase);
// before a convolution over `list`: the halo exchange of its input; *rows = the rows this rank computes, with their plan
int asr_shard_before_conv(asr_hip_context* ctx, asr_shard_state* st, const NbList& list, void* feat, i64 ld_bytes,
                          i64 row_bytes, float* imp, unsigned* in_amax, const asr_conv_plan** rows);
int asr_shard_stitch(asr_hip_context* ctx, asr_shard_state* st, float* values);
const int32_t* asr_shard_owned_rows0(const asr_shard_state* st, i64* n);  // grid-0 rows of this rank, ascending (world > 1)

// internal entry points shared between translation units
int asr_geom_point_keys(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts,
                        const float* radii, i64 n, float radius_scale, int max_depth, u64* keys);
int asr_geom_octree_build(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts,
                          const float* radii, i64 n, float radius_scale, int max_depth, int grow_steps = 0,
                          const u64* extra_keys = nullptr, i64 num_extra = 0, bool balance = true);
// cell table of ctx->pindex (after asr_geom_presort) for every level a leaf can have; blocks on ctx->stream
int asr_geom_precells(asr_hip_context* ctx, Arena& keep);
// Morton order of the points (+ radii) into ctx->pindex, arrays in `keep`
int asr_geom_presort(asr_hip_context* ctx, Arena& keep, const asr_octree_frame* frame, const float* pts,
                     const float* radii, i64 n, float radius_scale = 0.f, int max_depth = 21);
// the stand-alone neighbour lists of one grid (asr_hip_grid_neighbors_*); rows (optional, nrows entries): the lists of
// those rows only, the other rows stay empty
int asr_geom_grid_neighbors_count(asr_hip_context* ctx, const u64* keys, i64 v, const int32_t* rows, i64 nrows, i64* rs,
                                  i64* num_pairs);
int asr_geom_grid_neighbors_fill(asr_hip_context* ctx, const u64* keys, i64 v, const int32_t* rows, i64 nrows,
                                 const i64* rs, int32_t* idx, uint8_t* kidx);
// the neighbour lists of all grids of a hierarchy in ONE pass: one launch each for the key maps, the counting pass and
// the filling pass, one scan, one read-back of the pair counts (round 4; was five times count / scan / read-back / fill)
struct asr_nb_job {
    const u64* keys;  // in: sorted voxel keys
    i64 v;
    i64* rs;          // out (arrays in out_arena)
    int32_t* idx;
    uint8_t* kidx;
    i64 p;
    const int32_t* owner = nullptr;  // optional: lists for the rows with owner[row] == me only (the others stay empty)
    int me = 0;
};
int asr_geom_neighbors_build_batch(asr_hip_context* ctx, Arena& out_arena, asr_nb_job* jobs, int n);
struct asr_row_group_job {
    const uint8_t* kidx;
    const i64* rs;
    i64 v;
    int kbits;  // the list's slots are below this (at most 56)
    int32_t* perm_out;
};
// MFMA tiling order of every list, rows regrouped inside segments of seg >= 16 rows by their slot mask >> mask_shift;
// ranked: sort on the masks' ranks where that is possible (option "row_ranked")
int asr_geom_row_groups_batch(asr_hip_context* ctx, const asr_row_group_job* jobs, int n, i64 seg, int mask_shift,
                              bool ranked);
int asr_geom_coarsen_count(asr_hip_context* ctx, const u64* keys, i64 v, i64* v_out);
// EINVAL when v_out is not what asr_geom_coarsen_count gives
int asr_geom_coarsen_fill(asr_hip_context* ctx, const u64* keys, i64 v, u64* out_keys, i64 v_out,
                          int32_t* up_idx, uint8_t* up_kidx, i64* up_rs);
// down_*: the inverted up lists (rows = coarse voxels; what open3d::invert_neighbors_list returns for the up lists)
int asr_geom_coarsen_build(asr_hip_context* ctx, Arena& keep, const u64* keys, i64 v, u64** out_keys, i64* v_out,
                           int32_t** up_idx, uint8_t** up_kidx, i64** up_rs, int32_t** down_idx, uint8_t** down_kidx,
                           i64** down_rs);
int asr_geom_voxel_info(asr_hip_context* ctx, const asr_octree_frame* frame, const u64* keys,
                        i64 v, float* centers, float* sizes);
// keep: arena for the Morton-ordered point arrays (scratch when null); fill: spos (optional) receives
// each pair's neighbour as a position in Morton order, sorted_out the Morton-ordered points (x, y, z,
// original index bits) they refer to
// radii: gathered into Morton order together with the points (the fill call then needs no pass of its own);
// voxel_keys: the queries are the centres of these grid voxels with radius = voxel size ("aligned": half-size search
// cells, see AlignedQ in asr_geom.hip); lmin / lmax: levels of the queries when the caller knows them (else -1)
int asr_geom_radius_count(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts,
                          i64 n, const float* centers, const float* sizes, i64 v, i64* rs,
                          i64* num_pairs, Arena* keep = nullptr, const float* radii = nullptr,
                          const u64* voxel_keys = nullptr, int lmin_hint = -1, int lmax_hint = -1,
                          const AsrPointIndex* pre = nullptr);

int asr_geom_radius_fill(asr_hip_context* ctx, const float* pts, const float* radii, i64 n,
                         const float* centers, const float* sizes, i64 v, const i64* rs,
                         int32_t* idx, float* dist, float* compat, int32_t* spos = nullptr,
                         const float4** sorted_out = nullptr);
int asr_geom_radius_neighbor_count(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts,
                                   const float* radii, i64 n, i64* counts_out);
// attributes [n,c] blended at positions [m,3] with the aggregation's weight, widening per row (asr_hip_point_attributes_at)
int asr_geom_attributes_at(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts, const float* radii, i64 n,
                           const float* attr, int c, const float* positions, const float* sizes, i64 m, int max_widen,
                           float min_weight, float fill, float* out, float* weight_out, int8_t* widen_out);
int asr_geom_knn(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts, i64 n, int k,
                 const float* radii_in, float radius_fraction, int outlier_threshold, float* radii_out,
                 uint8_t* inlier_out);
// nearest point of each query among pts (exact, ties to the smallest index); either output may be null
int asr_geom_nearest(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts, i64 n, const float* queries,
                     i64 m, int32_t* index_out, float* sqdist_out);
// one ICP step (pairs within max_distance, sums of the normal equations) and the ICP loop over one index of the target
int asr_geom_icp_step(asr_hip_context* ctx, const asr_octree_frame* frame, const float* target, i64 n, const float* normals,
                      const float* source, i64 m, const double transform[12], const double origin[3], float max_distance,
                      asr_icp_sums* sums, int32_t* index_out);
int asr_geom_register(asr_hip_context* ctx, const asr_octree_frame* frame, const float* target, i64 n, const float* normals,
                      const float* source, i64 m, const asr_icp_params* params, double transform[12],
                      asr_icp_report* report);
// the k nearest points of every point, itself included, ordered by (squared distance, index); either output may be null
int asr_geom_knn_index(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts, i64 n, int k,
                       int32_t* index_out, float* sqdist_out);
int asr_geom_dual_count(asr_hip_context* ctx, const u64* nodes, i64 num_nodes, const u64* leaves, i64 num_leaves,
                        i64* num_cells);
int asr_geom_dual_fill(asr_hip_context* ctx, i64* out);
int asr_geom_invert(asr_hip_context* ctx, i64 num_points, const int32_t* idx, const i64* rs,
                    i64 num_rows, const uint8_t* attr, int32_t* out_idx, i64* out_rs,
                    uint8_t* out_attr, i64 known_pairs = -1);
void asr_geom_release(asr_hip_context* ctx);

int asr_mesh_contour_count(asr_hip_context* ctx, const float* values, i64 num_values, const i64* duals,
                           i64 num_duals, const float* positions, float threshold, i64* num_vertices,
                           i64* num_triangles);
int asr_mesh_contour_fill(asr_hip_context* ctx, float* vertices, int32_t* triangles);
int asr_mesh_components_count(asr_hip_context* ctx, const float* vertices, i64 nv, const int32_t* triangles,
                              i64 nt, i64 keep_n, i64 min_size, i64* nv_out, i64* nt_out);
int asr_mesh_components_fill(asr_hip_context* ctx, float* vertices_out, int32_t* triangles_out);
// stratified area-weighted samples of a triangle mesh (asr_hip_mesh_sample); normals / tri may be null
int asr_mesh_sample(asr_hip_context* ctx, const float* vertices, i64 nv, const int32_t* triangles, i64 nt, i64 num_samples,
                    u64 seed, float* points, float* normals, int32_t* tri);
// octree vertex clustering with quadric placement (asr_hip_mesh_simplify_count / _fill); levels / vertex_map may be null
int asr_mesh_simplify_count(asr_hip_context* ctx, const asr_octree_frame* frame, const float* vertices, i64 nv,
                            const int32_t* triangles, i64 nt, const int8_t* levels, int level, i64* nv_out, i64* nt_out);
int asr_mesh_simplify_fill(asr_hip_context* ctx, float* vertices_out, int32_t* triangles_out, int32_t* vertex_map);
// mesh adjacency (asr_hip_mesh_edges_count / _fill, asr_hip_mesh_topology, asr_hip_mesh_smooth); arguments validated by the callers
int asr_mesh_edges_count(asr_hip_context* ctx, const int32_t* triangles, i64 nt, i64 nv, i64* num_edges);
int asr_mesh_edges_fill(asr_hip_context* ctx, int32_t* edges, int32_t* uses, int32_t* forward);
int asr_mesh_topology_report(asr_hip_context* ctx, const int32_t* triangles, i64 nt, i64 nv, asr_mesh_topology* out);
int asr_mesh_smooth(asr_hip_context* ctx, const float* vertices, i64 nv, const int32_t* triangles, i64 nt, int iterations,
                    double lambda, double mu, int boundary, float* vertices_out);
// centroid fans over the simple rims of at most max_edges edges (asr_hip_mesh_fill_holes_count / _fill)
int asr_mesh_fill_holes_count(asr_hip_context* ctx, const float* vertices, i64 nv, const int32_t* triangles, i64 nt,
                              int max_edges, i64* nv_out, i64* nt_out, asr_mesh_fill_report* report);
int asr_mesh_fill_holes_fill(asr_hip_context* ctx, float* vertices_out, int32_t* triangles_out);
void asr_mesh_release(asr_hip_context* ctx);
// asr_points.hip: one point per occupied octree cell (asr_hip_points_merge_count / _fill); arguments validated by the callers
int asr_points_merge_count(asr_hip_context* ctx, const asr_octree_frame* frame, const float* points, i64 n,
                           const float* normals, const float* radii, const float* attributes, int c, const int8_t* levels,
                           int level, int split_sides, i64* num_clusters, asr_points_merge_report* report);
int asr_points_merge_fill(asr_hip_context* ctx, float* points_out, float* normals_out, float* radii_out,
                          float* attributes_out, int32_t* counts_out, int32_t* cluster_out);
// PCA normals over given neighbour lists and their orientation (asr_hip_point_normals / asr_hip_normals_orient); arguments
// validated by the callers
int asr_points_normals(asr_hip_context* ctx, const float* points, i64 n, const int32_t* index, int k, float* normals_out,
                       float* eigenvalues_out, uint8_t* ok_out);
int asr_points_orient(asr_hip_context* ctx, const float* points, const float* normals, i64 n, const int32_t* index, int k,
                      const float* viewpoints, i64 num_viewpoints, float* normals_out, uint8_t* flips_out, i64 report[4]);

// Global registration (asr_hip_point_fpfh / _feature_match / _ransac_transform, asr_features.hip); arguments validated by
// the callers.  ASR_FEATURE_MATCH_TILE: rows of b per LDS tile of the match (asr_hip.ops.FEATURE_MATCH_TILE for the tests).
#define ASR_FEATURE_MATCH_TILE 128
int asr_features_fpfh(asr_hip_context* ctx, const float* points, const float* normals, i64 n, const int32_t* index, int k,
                      float* fpfh_out, float* spfh_out, uint8_t* ok_out);
int asr_features_match(asr_hip_context* ctx, const float* a, i64 m, const float* b, i64 n, int dim, int32_t* index_out,
                       float* sqdist_out);
int asr_features_ransac(asr_hip_context* ctx, const float* source, i64 m, const float* target, i64 n, const int32_t* corr,
                        i64 c, const asr_ransac_params* params, double transform_out[12], asr_ransac_report* report);

int asr_conv_agg_importance(asr_hip_context* ctx, const float* compat, const float* dist, i64 n,
                            float* out);
int asr_conv_cconv(asr_hip_context* ctx, const float* filters, const float* out_pos,
                   const float* extents, const float* inp_pos, const float* inp_feat,
                   const int32_t* nidx, const float* nimp, const i64* rs, i64 num_out, int cin,
                   int cout, int normalize, const float* bias, int relu, float* out, int sorted4 = 0,
                   unsigned* out_absmax = nullptr);  // != null: max(its value, f32 bits of the largest |out|), kept by the kernels
int asr_conv_cconv_basis(asr_hip_context* ctx, const float* out_pos, const float* extents, const float* inp_pos,
                         const float* inp_feat, const int32_t* nidx, const float* nimp, const i64* rs, i64 num_out,
                         float* basis_out, float* norm_out);
int asr_conv_sparse(asr_hip_context* ctx, const asr_sparse_conv_args* args);
// asr_conv16.hip: 16-bit matrix-core variants (f16 activations / exact bf16x3 split)
// two phases so that callers with several lists pay one host read-back: count enqueues the slot-set pass and
// the scan (the block total lands in plan->offs[groups_pad]); fill allocates the pool and writes it
int asr_geom_conv_plan_count(asr_hip_context* ctx, Arena& keep, const int32_t* nidx, const uint8_t* kidx, const i64* rs,
                             const int32_t* perm, i64 num_out, int K, asr_conv_plan* plan);
int asr_geom_conv_plan_fill(asr_hip_context* ctx, Arena& keep, asr_conv_plan* plan, i64 blocks);
// *plans[j] with nidx/kidx/rs/perm/num_out/K set: all built in one pass over the concatenated lists, one pool
int asr_geom_conv_plan_batch(asr_hip_context* ctx, Arena& keep, asr_conv_plan* const* plans, int n);
int asr_geom_conv_plan_build(asr_hip_context* ctx, Arena& keep, const int32_t* nidx, const uint8_t* kidx, const i64* rs,
                             const int32_t* perm, i64 num_out, int K, asr_conv_plan* plan);  // count + read-back + fill

size_t asr_conv16_packed_bytes(int mode, int K, int cin, int cout, int cout_b);
int asr_conv16_pack(asr_hip_context* ctx, int mode, const float* wa, const float* wb, int K, int cin, int ca, int cb,
                    void* out);
int asr_conv16_convert(asr_hip_context* ctx, const void* in, i64 n, void* out, int to_f16);
int asr_conv16_absmax(asr_hip_context* ctx, const float* x, i64 rows, int c, i64 ld, unsigned* out);
int asr_conv_sparse16(asr_hip_context* ctx, const asr_sparse_conv_args* args, const void* packed, int mode,
                      int out_f16, const asr_conv_plan* plan);
int asr_conv_reduce(asr_hip_context* ctx, const float* values, const int32_t* gidx, const i64* rs,
                    i64 rows, float* out);
int asr_conv_decode(asr_hip_context* ctx, const float* code, i64 v, int c, const float* w1,
                    const float* b1, int h1, const float* w2, const float* b2, int h2,
                    const float* w3, const float* sizes, float* out, const int32_t* rows = nullptr);  // rows: v listed rows
// asr_query.hip: leaf location, decoder at shifts (sizes: values[:, 0] *= sizes[row]; grad = d decode[:, 0] / d shift),
// and the fused whole-path query on a leaf set with its centres and sizes
int asr_query_leaf_locate(asr_hip_context* ctx, const asr_octree_frame* frame, const u64* keys, i64 n, const float* pos,
                          i64 m, int32_t* rows);
int asr_query_decode_at(asr_hip_context* ctx, const float* code, int c, const int32_t* rows, const float* shifts, i64 m,
                        const float* w1, const float* b1, int h1, const float* w2, const float* b2, int h2,
                        const float* w3, const float* sizes, float* values, float* grad);
int asr_query_implicit(asr_hip_context* ctx, const asr_octree_frame* frame, const u64* keys, const float* centers,
                       const float* sizes, i64 num_leaves, const float* code, int c, const float* w1, const float* b1,
                       int h1, const float* w2, const float* b2, int h2, const float* w3, int scale_sdf,
                       const float* pos, i64 m, float* values, float* grad, int32_t* rows_out);
