// asr_geom.hip -- integer / geometry half of the hot path on gfx950:
//   a3 point location codes, a4 octree closure + 2:1 face balance, a5 55-slot neighbour CSR,
//   a6 sibling coarsening, a7 voxel info, a8 multi-radius search + scale compatibility,
//   a11 CSR inversion.
// All kernels are HBM / latency bound integer work: open-addressing hash tables in HBM
// (64-bit CAS), rocPRIM radix sort / scan for ordering, one thread per voxel / point / pair.
// Compiled with -ffp-contract=off: the float expressions below must round exactly like the
// reference's.
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <rocprim/rocprim.hpp>

#include "asr_common.h"
#include "asr_prim.h"

namespace {
using namespace asr_prim;

constexpr int BLK = 256;

// ------------------------------------------------------------------------------------------
// hash set / map on u64 keys (0 = empty)
// ------------------------------------------------------------------------------------------
struct HashTab {
    u64* keys;
    int32_t* vals;  // may be null (set)
    u64 mask;
};

// Probe sequence of a key.  Locality preserving: the low 6 bits of a location code (two levels of child index = the
// position inside a 4 x 4 x 4 block of cells) are kept, only the block id is scrambled.  The keys of one block land in
// one 64-slot bucket (512 B) at distinct slots, and the probes a voxel makes for its face neighbours -- or a wave of
// Morton-ordered voxels makes together -- stay in a few cache lines instead of one random line per probe.  A
// collision (another block hashed to the same bucket) moves to the SAME position of another bucket (double
// hashing over buckets): stepping to the next slot instead would run through the neighbouring keys of both
// blocks (measured: 5x slower than plain hashing).  cap is a power of two >= 64, the bucket step is odd.
// Keys whose low 6 bits are concentrated on a few values (points on a lattice) fill "their" position of the buckets
// before the table is half full: the builders report the overflow and the hosts rebuild the table four times the size.
struct TabProbe {
    u64 bucket, step, low, bmask;
    __device__ inline u64 slot() const { return ((bucket & bmask) << 6) | low; }
    __device__ inline void next() { bucket += step; }
};
__device__ inline TabProbe tab_probe(const HashTab& t, u64 key) {
    const u64 h = asr_hash64(key >> 6);
    return TabProbe{h, (h >> 32) | 1, key & 63, t.mask >> 6};
}

__device__ inline u64 ld_agent(const u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// returns 1 = inserted, 0 = existed, -1 = table full; slot_out = slot of the key
__device__ inline int tab_insert(const HashTab& t, u64 key, u64* slot_out = nullptr) {
    TabProbe pr = tab_probe(t, key);
    for (u64 probe = 0; probe <= pr.bmask; ++probe, pr.next()) {
        const u64 slot = pr.slot();
        u64 cur = ld_agent(&t.keys[slot]);
        if (cur == 0) {
            cur = atomicCAS((unsigned long long*)&t.keys[slot], 0ull, (unsigned long long)key);
            if (cur == 0) {
                if (slot_out) *slot_out = slot;
                return 1;
            }
        }
        if (cur == key) {
            if (slot_out) *slot_out = slot;
            return 0;
        }
    }
    return -1;
}
// the same for key sets with FEW distinct values among many insertions (the slot masks of the neighbour lists: most rows
// of a grid share the interior mask, the rows of other ranks of a sharded cloud the empty one): an agent-scope load of one
// address by every wave of the launch serialises at that address's memory channel, so the probe reads through the caches
// first.  A key never changes once written: a cached non-zero value is the truth, a cached zero is checked again.
__device__ inline int tab_insert_shared(const HashTab& t, u64 key) {
    TabProbe pr = tab_probe(t, key);
    for (u64 probe = 0; probe <= pr.bmask; ++probe, pr.next()) {
        const u64 slot = pr.slot();
        u64 cur = t.keys[slot];
        if (cur == 0) cur = ld_agent(&t.keys[slot]);
        if (cur == 0) {
            cur = atomicCAS((unsigned long long*)&t.keys[slot], 0ull, (unsigned long long)key);
            if (cur == 0) return 1;
        }
        if (cur == key) return 0;
    }
    return -1;
}
// lookup after the building kernel finished (plain loads)
__device__ inline bool tab_contains(const HashTab& t, u64 key) {
    TabProbe pr = tab_probe(t, key);
    for (u64 probe = 0; probe <= pr.bmask; ++probe, pr.next()) {
        const u64 slot = pr.slot();
        const u64 cur = t.keys[slot];
        if (cur == key) return true;
        if (cur == 0) return false;
    }
    return false;
}
__device__ inline int tab_find(const HashTab& t, u64 key) {
    TabProbe pr = tab_probe(t, key);
    for (u64 probe = 0; probe <= pr.bmask; ++probe, pr.next()) {
        const u64 slot = pr.slot();
        const u64 cur = t.keys[slot];
        if (cur == key) return t.vals[slot];
        if (cur == 0) return -1;
    }
    return -1;
}
__device__ inline i64 tab_find_slot(const HashTab& t, u64 key) {
    TabProbe pr = tab_probe(t, key);
    for (u64 probe = 0; probe <= pr.bmask; ++probe, pr.next()) {
        const u64 slot = pr.slot();
        const u64 cur = t.keys[slot];
        if (cur == key) return (i64)slot;
        if (cur == 0) return -1;
    }
    return -1;
}

// append with ONE atomic per 256-thread block; must be reached by every thread of the block (4 waves).
// Same-address atomics retire at ~88 / us: one per wave is 0.5 ms for 2.6 M voxels.
__device__ inline int block_append(bool pred, int* counter) {
    __shared__ int s_cnt[4];
    __shared__ int s_base;
    const unsigned long long m = __ballot(pred);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        s_base = total ? atomicAdd(counter, total) : 0;
    }
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wave; ++w) off += s_cnt[w];
    return off + __popcll(m & ((1ull << lane) - 1));
}

u64 next_pow2(u64 x) {
    u64 p = 1;
    while (p < x) p <<= 1;
    return p;
}

// ------------------------------------------------------------------------------------------
// a3: point -> (level, key)   octree.h:42-68
// ------------------------------------------------------------------------------------------
__device__ inline int level_from_scale(const asr_octree_frame& f, float scale) {
    for (int level = 0; level <= ASR_MAX_LEVEL; ++level)
        if (f.voxel_size[level] < scale) return level - 1 > 0 ? level - 1 : 0;
    return ASR_MAX_LEVEL;
}
__device__ inline u64 point_key(const asr_octree_frame& f, const float* pts, const float* radii,
                                i64 i, float radius_scale, int max_depth) {
    float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    if (px < f.bb_min[0] || py < f.bb_min[1] || pz < f.bb_min[2] || px > f.bb_max[0] ||
        py > f.bb_max[1] || pz > f.bb_max[2])
        return 0;
    int level = level_from_scale(f, radius_scale * radii[i]);
    level = level < max_depth ? level : max_depth;
    int x, y, z;
    frame_coord(f, px, py, pz, level, x, y, z);
    return asr_coord_key(x, y, z, level);
}

__global__ void k_point_keys(asr_octree_frame f, const float* pts, const float* radii, i64 n,
                             float radius_scale, int max_depth, u64* keys) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i < n) keys[i] = point_key(f, pts, radii, i, radius_scale, max_depth);
}

// ------------------------------------------------------------------------------------------
// a4: octree node set.  Nodes live in an open-addressing hash set (membership) AND in an append
// only list of sibling groups (8 consecutive keys, first sibling first): the list gives the
// BalanceFaces frontiers and the final node array without ever scanning the (mostly empty) table.
// cnt[F_ENTRIES] = list entries (multiple of 8), cnt[F_OVERFLOW] = overflow flag, cnt[F_ROOT] = root inserted (asr_prim.h).
// ------------------------------------------------------------------------------------------
// insert the sibling group of `a` and all missing ancestor groups (+ root).
// The thread that wins the CAS on a group's first sibling creates the other seven and
// continues upwards; losers stop (CreateAncestorsAndSiblings, octree.cpp:110-150).
__device__ inline void insert_with_ancestors(const HashTab& t, u64 a, int* cnt, u64* list,
                                             int list_cap) {
    const int lane = threadIdx.x & 63;
    while (true) {
        if (a == 1) {
            int r = tab_insert(t, 1);
            if (r == 1) cnt[F_ROOT] = 1;
            if (r < 0) cnt[F_OVERFLOW] = 1;
            return;
        }
        u64 first = a & ~u64(7);
        int r = tab_insert(t, first);
        if (r < 0) {
            cnt[F_OVERFLOW] = 1;
            return;
        }
        // One list append per WAVE iteration: the lanes of the wave that are in this iteration of the loop and created
        // a group share one atomic on the list counter (same-address atomics are the bottleneck of this kernel: one
        // per new group was 0.37 M of them at 10 M points).  __ballot / __shfl act on the lanes that execute them.
        const bool created = r == 1;
        const unsigned long long m = __ballot(created);
        if (!created) return;
        for (int j = 1; j < 8; ++j)
            if (tab_insert(t, first + j) < 0) cnt[F_OVERFLOW] = 1;
        const int leader = __builtin_ctzll(m);
        int base = 0;
        if (lane == leader) base = atomicAdd(&cnt[F_ENTRIES], 8 * __popcll(m));
        base = __shfl(base, leader, 64);
        const int pos = base + 8 * __popcll(m & ((1ull << lane) - 1));
        if (pos + 8 <= list_cap) {
            for (int j = 0; j < 8; ++j) list[pos + j] = first + j;
        } else {
            cnt[F_OVERFLOW] = 1;
        }
        a >>= 3;
    }
}

// cnt[F_KEY_BITS] = number of significant bits of the longest key in the node list (cnt[F_ENTRIES] entries; the list is radix-sorted on
// those bits only).  A pass of its own over the list: the same test inside the insertion kernels, next to their atomics
// on cnt[F_ENTRIES], made them 2.6x slower.
__global__ void k_list_key_bits(const u64* list, int list_cap, int* cnt) {
    const int n = min(cnt[F_ENTRIES], list_cap);
    int bits = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const u64 k = list[i];
        bits = max(bits, k ? 64 - __clzll((long long)k) : 0);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits = max(bits, __shfl_xor(bits, o, 64));
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(&cnt[F_KEY_BITS], bits);
}

__global__ void k_octree_insert_points(asr_octree_frame f, const float* pts, const float* radii,
                                       i64 n, float radius_scale, int max_depth, HashTab t,
                                       int* cnt, u64* list, int list_cap) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    u64 key = 0;
    if (i < n) {
        if (!(isfinite(pts[3 * i]) && isfinite(pts[3 * i + 1]) && isfinite(pts[3 * i + 2]) && isfinite(radii[i])))
            cnt[F_NONFINITE] = 1;  // rejected by the host: the reference has undefined behaviour on such input
        else
            key = point_key(f, pts, radii, i, radius_scale, max_depth);
    }
    // consecutive points of a scan mostly fall into the same cell: a lane whose left neighbour carries the same key
    // leaves the insertion (a probe of the table at least) to it
    const u64 left = __shfl_up(key, 1, 64);
    if ((threadIdx.x & 63) != 0 && left == key) return;
    if (key == 0) return;  // the reference inserts key 0 here and then hits UB
    insert_with_ancestors(t, key, cnt, list, list_cap);
}

// ------------------------------------------------------------------------------------------
// Octree::Grow (octree.cpp:44-108), on the raw point keys: a second hash set + key list.  One iteration = two
// kernels: the candidates of condition :87 ("not a node, has no child") are evaluated against the set as it is at
// the START of the iteration, then candidates and siblings are inserted (what is new forms the next frontier).
// ------------------------------------------------------------------------------------------
__global__ void k_grow_init(asr_octree_frame f, const float* pts, const float* radii, i64 n, float radius_scale,
                            int max_depth, HashTab t, int* cnt, u64* list, int list_cap) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!(isfinite(pts[3 * i]) && isfinite(pts[3 * i + 1]) && isfinite(pts[3 * i + 2]) && isfinite(radii[i]))) {
        cnt[F_NONFINITE] = 1;
        return;
    }
    const u64 key = point_key(f, pts, radii, i, radius_scale, max_depth);
    if (key == 0) return;
    const int r = tab_insert(t, key);
    if (r < 0) cnt[F_OVERFLOW] = 1;
    if (r == 1) {
        const int pos = atomicAdd(&cnt[F_ENTRIES], 1);
        if (pos < list_cap)
            list[pos] = key;
        else
            cnt[F_OVERFLOW] = 1;
    }
}
__device__ inline bool tab_has_child(const HashTab& t, u64 key) {
    if (__clzll((long long)key) <= 1) return false;
    for (int k = 0; k < 8; ++k)
        if (tab_contains(t, (key << 3) + k)) return true;
    return false;
}
// one thread per (frontier key, j): cand[7 i + jj] = the parent-level cell to add, or 0
__global__ void k_grow_candidates(HashTab t, const u64* list, int lo, int count, u64* cand) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count * 7) return;
    const u64 cur = list[lo + e / 7];
    u64 out = 0;
    if (cur != 1) {
        const int cfg = 7 - (int)(cur & 7);
        int j = e % 7;
        if (j >= cfg) ++j;  // the eight cells of the block without the parent itself
        int x, y, z, lev;
        asr_key_coord(cur >> 3, x, y, z, lev);
        const u64 key = asr_coord_key(x + (j & 1) - (cfg & 1), y + ((j >> 1) & 1) - ((cfg >> 1) & 1),
                                      z + ((j >> 2) & 1) - ((cfg >> 2) & 1), lev);
        if (key != 0 && !tab_contains(t, key) && !tab_has_child(t, key)) out = key;
    }
    cand[e] = out;
}
__global__ void k_grow_insert(HashTab t, u64* list, int lo, int count, const u64* cand, int* cnt, int list_cap) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count * 14) return;
    const u64 cur = list[lo + e / 14];
    if (cur == 1) return;
    const int j = e % 14;
    u64 key;
    if (j < 7) {
        key = cand[(e / 14) * 7 + j];
        if (key == 0) return;
    } else {  // siblings (:94-101)
        const u64 first = cur & ~u64(7);
        int sj = j - 7;
        if (first + sj >= cur) ++sj;
        key = first + sj;
    }
    const int r = tab_insert(t, key);
    if (r < 0) cnt[F_OVERFLOW] = 1;
    if (r == 1) {
        const int pos = atomicAdd(&cnt[F_ENTRIES], 1);
        if (pos < list_cap)
            list[pos] = key;
        else
            cnt[F_OVERFLOW] = 1;
    }
}
// closure over an explicit key list (the grown set) instead of the points
__global__ void k_octree_insert_keys(const u64* keys, i64 n, HashTab t, int* cnt, u64* list, int list_cap) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    insert_with_ancestors(t, keys[i], cnt, list, list_cap);
}

// BalanceFaces (octree.cpp:152-206), one round: the frontier is the list range [lo, hi) of sibling
// groups.  Leaf test against the node set at round start (octree.cpp:175) ...
__global__ void k_balance_classify(HashTab t, const u64* list, int lo, int ngroups, uint8_t* flag) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ngroups) return;
    u64 k = list[lo + 8 * i];
    bool has_child = (__clzll((long long)k) > 1) && tab_contains(t, k << 3);
    flag[i] = has_child ? 0 : 1;
}
// ... then octree.cpp:177-203 for all leaf groups: the 6 face neighbours of the parent must exist
__global__ void k_balance_insert(HashTab t, u64* list, int lo, int ngroups, const uint8_t* flag,
                                 int* cnt, int list_cap) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ngroups * 6) return;
    if (!flag[i / 6]) return;
    u64 k = list[lo + 8 * (i / 6)];
    int j = i % 6;
    const int ox = (j == 0) ? -1 : (j == 3) ? 1 : 0;
    const int oy = (j == 1) ? -1 : (j == 4) ? 1 : 0;
    const int oz = (j == 2) ? -1 : (j == 5) ? 1 : 0;
    int x, y, z, lev;
    asr_key_coord(k >> 3, x, y, z, lev);
    u64 key = asr_coord_key(x + ox, y + oy, z + oz, lev);
    if (key == 0) return;
    insert_with_ancestors(t, key, cnt, list, list_cap);
}
// leaves = nodes without first child (InitAttributesAndLeaves, octree.cpp:208-228): flags over the SORTED node
// array, compacted in order (the leaves come out sorted: no second radix sort)
__global__ void k_leaf_flags(HashTab t, const u64* nodes, i64 n, uint8_t* flags) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 k = nodes[i];
    flags[i] = (k != 0 && !((__clzll((long long)k) > 1) && tab_contains(t, k << 3))) ? 1 : 0;
}

// number of leaves + first / last leaf key in one read-back (the levels of the leaves are the query levels of the
// aggregation search)
__global__ void k_leaf_tail(const u64* leaves, const i64* num, i64* out3) {
    const i64 n = *num;
    out3[0] = n;
    out3[1] = n > 0 ? (i64)leaves[0] : 0;
    out3[2] = n > 0 ? (i64)leaves[n - 1] : 0;
}

// ------------------------------------------------------------------------------------------
// a5: neighbour CSR.  grid.cpp:43-175
// ------------------------------------------------------------------------------------------
__global__ void k_map_build(const u64* keys, i64 v, HashTab t, int* cnt) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= v) return;
    u64 slot;
    int r = tab_insert(t, keys[i], &slot);
    if (r < 0)
        cnt[F_OVERFLOW] = 1;
    else
        t.vals[slot] = (int32_t)i;
}

__constant__ int8_t c_child_off[24][3] = {
        {-1, 0, 0}, {-1, 1, 0}, {-1, 0, 1}, {-1, 1, 1}, {2, 0, 0},  {2, 1, 0},  {2, 0, 1},  {2, 1, 1},
        {0, -1, 0}, {1, -1, 0}, {0, -1, 1}, {1, -1, 1}, {0, 2, 0},  {1, 2, 0},  {0, 2, 1},  {1, 2, 1},
        {0, 0, -1}, {1, 0, -1}, {0, 1, -1}, {1, 1, -1}, {0, 0, 2},  {1, 0, 2},  {0, 1, 2},  {1, 1, 2}};
__constant__ int8_t c_nb_off[6][3] = {{-1, 0, 0}, {1, 0, 0}, {0, -1, 0},
                                      {0, 1, 0},  {0, 0, -1}, {0, 0, 1}};
__constant__ int8_t c_parent_koff[6][8] = {
        {-1, 0, -1, 1, -1, 2, -1, 3}, {0, -1, 1, -1, 2, -1, 3, -1}, {-1, -1, 0, 1, -1, -1, 2, 3},
        {0, 1, -1, -1, 2, 3, -1, -1}, {-1, -1, -1, -1, 0, 1, 2, 3}, {0, 1, 2, 3, -1, -1, -1, -1}};

// candidate c in [0,36): 0..5 same level, 6..29 child level, 30..35 parent level.
// returns neighbour index or -1; slot = kernel index of the hit.
__device__ inline int neighbor_candidate(const HashTab& t, u64 key, int x, int y, int z, int lev,
                                         int c, int& slot) {
    if (c < 6) {
        u64 nk = asr_coord_key(x + c_nb_off[c][0], y + c_nb_off[c][1], z + c_nb_off[c][2], lev);
        slot = 1 + c;
        return nk ? tab_find(t, nk) : -1;
    } else if (c < 30) {
        if (lev >= ASR_MAX_LEVEL) return -1;
        int j = c - 6;
        u64 nk = asr_coord_key(2 * x + c_child_off[j][0], 2 * y + c_child_off[j][1],
                               2 * z + c_child_off[j][2], lev + 1);
        slot = 7 + j;
        return nk ? tab_find(t, nk) : -1;
    } else {
        if (lev <= 0) return -1;
        int j = c - 30;
        u64 nk = asr_coord_key(x + c_nb_off[j][0], y + c_nb_off[j][1], z + c_nb_off[j][2], lev);
        if (!nk) return -1;
        int koff = c_parent_koff[j][nk & 7];
        if (koff < 0) return -1;  // sibling: its parent is this voxel's parent, never in the grid
        slot = 31 + 4 * j + koff;
        return tab_find(t, nk >> 3);
    }
}

// public row lists / key lists are caller data: a bad entry must become an error, not an out-of-bounds write.
// mark (optional, zeroed int32[v]): 1 at the listed rows, the row filter of a neighbour batch
__global__ void k_check_rows(const int32_t* rows, i64 nrows, i64 v, int* cnt, int32_t* mark) {
    const i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const i64 q = rows[r];
    if (q < 0 || q >= v || (r > 0 && rows[r - 1] >= q)) cnt[F_BAD_KEY] = 1;  // in range, strictly ascending
    else if (mark) mark[q] = 1;
}
__global__ void k_check_keys(const u64* keys, i64 n, int* cnt) {
    const i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys[i];
    // a location code: leading bit at position 3 * level, level <= ASR_MAX_LEVEL (0 is the tables' empty sentinel)
    if (k == 0 || (63 - __clzll((long long)k)) % 3 != 0) cnt[F_BAD_KEY] = 1;
}

// The lists of ALL grids of a hierarchy in one launch each (asr_geom_neighbors_build_batch; the stand-alone operators
// are a batch of one grid): the coarse grids hold a few thousand voxels, whose 13-odd dependent probes cost a level-0
// kernel's latency each when launched one by one.  Rows of all jobs share one index space, every job followed by one
// terminator entry, so that ONE exclusive scan gives every job's row splits (shifted by the job's first value) and the
// pair counts at the job boundaries.
// The hits of the counting pass are parked (neighbour index + slot, NB_STAGE per row) so that the fill pass is a copy for
// all but the few rows with more neighbours: the 8..13 hash probes per voxel are not repeated.
constexpr int NB_STAGE = 16;
constexpr int NB_MAX_JOBS = 8;
struct NbBatch {
    int n;
    i64 base[NB_MAX_JOBS + 1];  // first entry of each job in the shared index space; base[n] = total
    i64 v[NB_MAX_JOBS];
    const u64* keys[NB_MAX_JOBS];
    HashTab tab[NB_MAX_JOBS];
    i64* rs[NB_MAX_JOBS];  // optional: the fill writes each job's row splits here
    int32_t* idx[NB_MAX_JOBS];
    uint8_t* kidx[NB_MAX_JOBS];
    const int32_t* owner[NB_MAX_JOBS];  // optional row filter (one rank of a sharded cloud builds its own rows)
    int me[NB_MAX_JOBS];
};
// job of entry e of a batch's shared index space (NbBatch, RowGroupBatch, PlanBatch: n jobs, job j from base[j] on)
template <class Batch>
__device__ inline int job_of(const Batch& b, i64 e) {
    int j = 0;
    while (j + 1 < b.n && e >= b.base[j + 1]) ++j;
    return j;
}
__global__ void k_map_build_batch(NbBatch b, int* cnt) {
    const i64 e = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (e >= b.base[b.n]) return;
    const int j = job_of(b, e);
    const i64 i = e - b.base[j];
    if (i >= b.v[j]) return;
    u64 slot;
    if (tab_insert(b.tab[j], b.keys[j][i], &slot) < 0)
        cnt[F_OVERFLOW] = 1;
    else
        b.tab[j].vals[slot] = (int32_t)i;
}
// masks, stage_idx / stage_slot: optional, for the fill pass
__global__ void k_neighbors_count_batch(NbBatch b, i64* counts, u64* masks, int32_t* stage_idx, uint8_t* stage_slot) {
    const i64 e = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (e >= b.base[b.n]) return;
    const int j = job_of(b, e);
    const i64 i = e - b.base[j];
    if (i >= b.v[j]) {  // the job's terminator
        counts[e] = 0;
        return;
    }
    if (b.owner[j] && b.owner[j][i] != b.me[j]) {
        counts[e] = 0;
        if (masks) masks[e] = 0;
        return;
    }
    const HashTab t = b.tab[j];
    const u64 key = b.keys[j][i];
    int x, y, z, lev;
    asr_key_coord(key, x, y, z, lev);
    u64 m = 0;
    int n = 1;
    // The voxels of a grid are disjoint cells: where the same-level neighbour across a face exists, neither its four
    // children nor its parent can, so those five probes are skipped (36 -> ~13 probes per voxel on a scan; the resulting
    // mask is the same).
#pragma unroll 6
    for (int c = 0; c < 36; ++c) {
        if (c >= 6) {
            const int face = c < 30 ? (c - 6) >> 2 : c - 30;
            if ((m >> face) & 1) continue;
        }
        int slot = 0;
        const int idx = neighbor_candidate(t, key, x, y, z, lev, c, slot);
        if (idx < 0) continue;
        m |= u64(1) << c;
        if (stage_idx && n - 1 < NB_STAGE) {
            stage_idx[e * NB_STAGE + (n - 1)] = idx;
            stage_slot[e * NB_STAGE + (n - 1)] = (uint8_t)slot;
        }
        ++n;
    }
    counts[e] = n;
    if (masks) masks[e] = m;
}
// totals[j] = pairs of job j (scan value at the next job's first entry minus the job's own)
__global__ void k_nb_totals(NbBatch b, const i64* scan, i64* totals) {
    const int j = threadIdx.x;
    if (j < b.n) totals[j] = scan[b.base[j] + b.v[j]] - scan[b.base[j]];
}
// without masks and staging every row probes all 36 candidates
__global__ void k_neighbors_fill_batch(NbBatch b, const i64* scan, const u64* masks, const int32_t* stage_idx,
                                       const uint8_t* stage_slot) {
    const i64 e = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (e >= b.base[b.n]) return;
    const int j = job_of(b, e);
    const i64 i = e - b.base[j];
    const i64 first = scan[b.base[j]];
    i64 o = scan[e] - first;
    if (b.rs[j]) b.rs[j][i] = o;  // (the terminator writes rs[v] = pairs of the job)
    if (i >= b.v[j]) return;
    const int n = (int)(scan[e + 1] - first - o);
    if (n == 0) return;  // a row of another rank
    int32_t* nidx = b.idx[j];
    uint8_t* nkidx = b.kidx[j];
    nidx[o] = (int32_t)i;
    nkidx[o] = 0;
    ++o;
    if (stage_idx && n - 1 <= NB_STAGE) {  // the candidate order of the counting pass is ascending slot order
        for (int q = 0; q < n - 1; ++q) {
            nidx[o + q] = stage_idx[e * NB_STAGE + q];
            nkidx[o + q] = stage_slot[e * NB_STAGE + q];
        }
        return;
    }
    const HashTab t = b.tab[j];
    const u64 key = b.keys[j][i];
    int x, y, z, lev;
    asr_key_coord(key, x, y, z, lev);
    const u64 m = masks ? masks[e] : ~u64(0);
    for (int c = 0; c < 36; ++c) {
        if (!((m >> c) & 1)) continue;
        int slot;
        const int idx = neighbor_candidate(t, key, x, y, z, lev, c, slot);
        if (idx >= 0) {
            nidx[o] = idx;
            nkidx[o] = (uint8_t)slot;
            ++o;
        }
    }
}

// ------------------------------------------------------------------------------------------
// a6: CombineSiblings.  grid.cpp:177-243
// ------------------------------------------------------------------------------------------
__device__ inline bool merged_head(const u64* keys, i64 v, i64 i) {
    u64 k = keys[i];
    return (k & 7) == 0 && i + 7 < v && keys[i + 7] == (k | 7);
}
// state: 0 = carried, 1 = merged head, 2 = merged member (dropped)
__device__ inline int coarsen_state(const u64* keys, i64 v, i64 i) {
    u64 k = keys[i];
    if ((k & 7) == 0) return merged_head(keys, v, i) ? 1 : 0;
    i64 h = i - (i64)(k & 7);
    if (h >= 0 && keys[h] == (k & ~u64(7)) && merged_head(keys, v, h)) return 2;
    return 0;
}
// CombineSiblings without a sort (round 4).  The coarse key set is the kept keys plus one parent per merged group; both
// sub-sequences are already sorted in input order, and location codes sort level-major, so an emitted key's position in
// the sorted output is  (#kept keys smaller) + (#parents smaller):
//   kept key e at input index i:        kept_before[i] + heads_before[lower_bound(keys, e << 3)]
//   parent e = keys[i] >> 3 of a head:  heads_before[i] + kept_before[lower_bound(keys, e)]
// (every key of a lower level is smaller; a head with key < 8 e has a parent < e).  One flag pass, one exclusive scan of
// the packed (kept | heads << 32) counts, one placement pass with a binary search -- instead of a multi-pass radix sort
// whose dozen launches per level dominate the four small coarsening steps.
__global__ void k_coarsen_flags(const u64* keys, i64 v, u64* packed) {
    const i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i > v) return;
    u64 f = 0;
    if (i < v) {
        const int st = coarsen_state(keys, v, i);
        f = st == 0 ? u64(1) : (st == 1 ? (u64(1) << 32) : 0);
    }
    packed[i] = f;
}
__global__ void k_coarsen_place(const u64* keys, i64 v, const u64* pre, u64* out_keys, int32_t* out_src) {
    const i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= v) return;
    const u64 mine = pre[i + 1] - pre[i];  // 1: kept, 1 << 32: head, 0: merged member
    if (!mine) return;
    const bool head = (mine >> 32) != 0;
    const u64 key = keys[i];
    const u64 e = head ? key >> 3 : key;
    const u64 probe = head ? e : key << 3;
    i64 lo = 0, hi = v;  // first input key >= probe (a level-21 key has no children: its probe overflows to "beyond the end")
    if (!head && asr_key_level(key) >= ASR_MAX_LEVEL) {
        lo = v;
    } else {
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (keys[mid] < probe)
                lo = mid + 1;
            else
                hi = mid;
        }
    }
    const u64 at = pre[lo];
    const i64 pos = head ? (i64)(pre[i] >> 32) + (i64)(at & 0xffffffffu) : (i64)(pre[i] & 0xffffffffu) + (i64)(at >> 32);
    out_keys[pos] = e;
    out_src[pos] = (int32_t)i;
}
__global__ void k_coarsen_up(const u64* keys, i64 v, const int32_t* sorted_src, i64 v_out,
                             int32_t* up_idx, uint8_t* up_kidx) {
    i64 p = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (p >= v_out) return;
    i64 i = sorted_src[p];
    if (merged_head(keys, v, i)) {
        for (int j = 0; j < 8; ++j) {
            up_idx[i + j] = (int32_t)p;
            up_kidx[i + j] = (uint8_t)j;
        }
    } else {
        up_idx[i] = (int32_t)p;
        up_kidx[i] = 8;
    }
}
// The inverted up lists ("down" lists, net_definitions_torch.py:548-559) follow from the same facts without the
// generic inversion (histogram + scan + stable sort): coarse voxel p owns either its eight consecutive children
// (slots 0..7) or the one carried voxel (slot 8), in ascending fine index -- the order of
// open3d::invert_neighbors_list.  cnt[p] feeds the exclusive scan that gives the row splits.
__global__ void k_coarsen_down_count(const u64* keys, i64 v, const int32_t* sorted_src, i64 v_out, i64* cnt) {
    i64 p = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (p > v_out) return;
    cnt[p] = p < v_out ? (merged_head(keys, v, sorted_src[p]) ? 8 : 1) : 0;
}
__global__ void k_coarsen_down_fill(const u64* keys, i64 v, const int32_t* sorted_src, i64 v_out, const i64* rs,
                                    int32_t* down_idx, uint8_t* down_kidx) {
    i64 p = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (p >= v_out) return;
    const i64 i = sorted_src[p], o = rs[p];
    if (merged_head(keys, v, i)) {
        for (int j = 0; j < 8; ++j) {
            down_idx[o + j] = (int32_t)(i + j);
            down_kidx[o + j] = (uint8_t)j;
        }
    } else {
        down_idx[o] = (int32_t)i;
        down_kidx[o] = 8;
    }
}
__global__ void k_iota64(i64* out, i64 n) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}

// ------------------------------------------------------------------------------------------
// a7: voxel centres / sizes.  grid.cpp:251-268, octree.h:78-93 (double arithmetic)
// ------------------------------------------------------------------------------------------
__global__ void k_voxel_info(asr_octree_frame f, const u64* keys, i64 v, float* centers,
                             float* sizes) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= v) return;
    int x, y, z, lev;
    asr_key_coord(keys[i], x, y, z, lev);
    int s = ASR_MAX_LEVEL - lev;
    double half = 0.5 * (double)(u64(1) << s);
    double vs = (double)f.voxel_size[ASR_MAX_LEVEL];
    if (centers) {
        centers[3 * i + 0] = (float)((((x << s) - f.offset[0]) + half) * vs);
        centers[3 * i + 1] = (float)((((y << s) - f.offset[1]) + half) * vs);
        centers[3 * i + 2] = (float)((((z << s) - f.offset[2]) + half) * vs);
    }
    if (sizes) sizes[i] = f.voxel_size[lev];
}

// ------------------------------------------------------------------------------------------
// a8: multi radius search.  Points are sorted by their level-21 Morton code inside the octree
// frame; for every level used by a query a hash table maps cell -> [start,end) in that order;
// a query of radius r looks at the 3^3 cells of the deepest level whose cell size is >= r.
// ------------------------------------------------------------------------------------------
__global__ void k_point_codes(asr_octree_frame f, const float* pts, i64 n, u64* codes,
                              int32_t* ids, int* cnt) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!(isfinite(pts[3 * i]) && isfinite(pts[3 * i + 1]) && isfinite(pts[3 * i + 2]))) cnt[F_NONFINITE] = 1;
    int x, y, z;
    frame_coord(f, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], ASR_MAX_LEVEL, x, y, z);
    const int lim = (1 << ASR_MAX_LEVEL) - 1;
    x = min(max(x, 0), lim);
    y = min(max(y, 0), lim);
    z = min(max(z, 0), lim);
    codes[i] = asr_morton3d((u64)x, (u64)y, (u64)z);
    ids[i] = (int32_t)i;
}
__global__ void k_gather_points(const float* pts, const int32_t* ids, i64 n, float4* sorted, int32_t* rank,
                                const float* radii = nullptr, float* srad = nullptr) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t id = ids[i];
    sorted[i] = make_float4(pts[3 * (i64)id], pts[3 * (i64)id + 1], pts[3 * (i64)id + 2],
                            __int_as_float(id));
    if (rank) rank[id] = (int32_t)i;  // original index -> position in Morton order
    if (srad) srad[i] = radii[id];    // per-point radii in Morton order (k_gather_radii in the same pass)
}
// per-point radii in Morton order (the compat factor of a pair then reads next to its neighbours)
__global__ void k_gather_radii(const float* radii, const int32_t* ids, i64 n, float* out) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i < n) out[i] = radii[ids[i]];
}
__device__ inline int query_level(const asr_octree_frame& f, float r) {
    int lev = 0;
    while (lev < ASR_MAX_LEVEL && f.voxel_size[lev + 1] >= r) ++lev;
    return lev;
}
// block reduction of the level range of a 256-thread block: one atomic pair per BLOCK (same-address atomics retire at
// ~88 / us, one per wave was 0.9 ms for 2.6 M voxels)
__device__ __forceinline__ void block_level_range(int lo, int hi, int* cnt) {
    __shared__ int s_lo[4], s_hi[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(&cnt[F_LEVEL_MIN], min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3])));
        atomicMax(&cnt[F_LEVEL_MAX], max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3])));
    }
}
// grid-stride loop over the query sizes
__global__ __launch_bounds__(256) void k_query_levels(asr_octree_frame f, const float* sizes, i64 v, int* cnt) {
    int lo = ASR_MAX_LEVEL, hi = 0;
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < v; i += (i64)gridDim.x * blockDim.x) {
        const int l = query_level(f, sizes[i]);
        lo = min(lo, l);
        hi = max(hi, l);
    }
    block_level_range(lo, hi, cnt);
}
// boundaries of the sorted code array: cell (prefix,level) starts / ends at i
template <bool COUNT_ONLY>
__global__ __launch_bounds__(256) void k_cell_bounds(const u64* codes, i64 n, int lmin, int lmax, HashTab t,
                                                     int32_t* start, int32_t* end, int* cnt, int* level_cnt) {
    __shared__ int s_sum[4];
    __shared__ int s_lvl[ASR_MAX_LEVEL + 1];  // COUNT_ONLY: cells per level (the host picks the hashed levels)
    if (COUNT_ONLY) {
        if (threadIdx.x <= ASR_MAX_LEVEL) s_lvl[threadIdx.x] = 0;
        __syncthreads();
    }
    int local = 0;
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i <= n; i += (i64)gridDim.x * blockDim.x) {
        u64 a = i > 0 ? codes[i - 1] : 0, b = i < n ? codes[i] : 0;
        for (int l = lmin; l <= lmax; ++l) {
            int s = 3 * (ASR_MAX_LEVEL - l);
            u64 pa = (s >= 63) ? 0 : (a >> s), pb = (s >= 63) ? 0 : (b >> s);
            bool has_a = i > 0, has_b = i < n;
            if (has_a && has_b && pa == pb) continue;
            u64 marker = u64(1) << (3 * l);
            if (COUNT_ONLY) {
                if (has_b) {
                    ++local;
                    atomicAdd(&s_lvl[l], 1);
                }
            } else {
                u64 slot;
                if (has_a) {
                    if (tab_insert(t, pa | marker, &slot) < 0)
                        cnt[F_OVERFLOW] = 1;
                    else
                        end[slot] = (int32_t)i;
                }
                if (has_b) {
                    if (tab_insert(t, pb | marker, &slot) < 0)
                        cnt[F_OVERFLOW] = 1;
                    else
                        start[slot] = (int32_t)i;
                }
            }
        }
    }
    if (COUNT_ONLY) {  // one atomic per block: 10^7 same-address atomics cost 2 ms
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o, 64);
        if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = local;
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(&cnt[F_CELLS], s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);
        if (level_cnt && threadIdx.x <= ASR_MAX_LEVEL && s_lvl[threadIdx.x]) atomicAdd(&level_cnt[threadIdx.x], s_lvl[threadIdx.x]);
    }
}

__device__ inline float sqdist3(float ax, float ay, float az, float bx, float by, float bz) {
    float dx = ax - bx, dy = ay - by, dz = az - bz;
    float s = dx * dx;
    s = s + dy * dy;
    s = s + dz * dz;
    return s;
}

// One WAVE per query: lanes 0..26 look up the 3^3 cells, the candidate points of all cells are
// then walked 64 at a time (flattened through a prefix of the cell counts).  Row lengths range
// from 0 to tens of thousands (a coarse voxel near the surface sees every point within one voxel
// size), so a thread-per-query loop is dominated by its longest row.
// MODE 0: count only (KDTree::ComputeRadiusNeighbors).
// MODE 2: single pass of the aggregation search.  Hits are collected in LDS; a row of at most
// RADIUS_LIGHT hits is ranked inside the wave (rank = number of smaller keys, keys are unique) and
// written, sorted, to the row's fixed slot tmp[q * RADIUS_LIGHT ..].  Rows with more hits, and rows
// whose 27 cells hold more than RADIUS_GIANT candidates (a coarse voxel next to a dense region: up
// to 10^5 candidates, which one wave would walk for milliseconds), go to the heavy list and are
// processed by k_radius_heavy with RADIUS_SPLIT blocks per row.
constexpr int RADIUS_LIGHT = 128;
constexpr int RADIUS_GIANT = 4096;
constexpr int RADIUS_SPLIT = 64;

// lanes 0..26 look up the 3^3 cells around the query; returns the candidate total, fills the
// per-wave prefix / begin tables
// Point ranges of cells.  Levels up to `lhash` are in the hash table; finer levels -- where a cloud with very dense
// spots would put nearly every point into a cell of its own, ten million entries per level -- are looked up by two
// binary searches in the Morton-sorted level-21 codes (the points of a cell are contiguous in that order).
struct CellIndex {
    HashTab tab;
    const int32_t* start;
    const int32_t* end;
    const u64* codes;  // sorted (on the bits of the finest indexed level)
    int n;
    int lhash;
};
__device__ inline void cell_range(const CellIndex& ci, u64 cell, int lev, int& b, int& cnt) {
    b = 0;
    cnt = 0;
    if (lev <= ci.lhash) {
        const i64 slot = tab_find_slot(ci.tab, cell | (u64(1) << (3 * lev)));
        if (slot >= 0) {
            b = ci.start[slot];
            cnt = ci.end[slot] - b;
        }
        return;
    }
    const int s = 3 * (ASR_MAX_LEVEL - lev);
    int lo = 0, hi = ci.n;  // first point whose level-`lev` cell is >= cell
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((ci.codes[mid] >> s) < cell)
            lo = mid + 1;
        else
            hi = mid;
    }
    int lo2 = lo, hi2 = ci.n;  // first point whose cell is > cell
    while (lo2 < hi2) {
        const int mid = (lo2 + hi2) >> 1;
        if ((ci.codes[mid] >> s) <= cell)
            lo2 = mid + 1;
        else
            hi2 = mid;
    }
    b = lo;
    cnt = lo2 - lo;
}

// Prefix / begin tables of the point ranges [b, b + n) that lanes 0..NCELL-1 hold; returns the candidate total.
// WALK: the form for a caller that goes through several blocks in a loop (the level walk below).  A total below `need`
// is returned with the tables untouched -- the caller skips such a block -- and a wave barrier comes BEFORE the writes
// too: the previous block's reads of the tables are finished.
template <int NCELL>
__device__ inline int cells_inclusive(int n, int lane) {  // inclusive prefix of n over lanes 0..NCELL-1
    int pre = n;
#pragma unroll
    for (int o = 1; o < (NCELL > 32 ? 64 : 32); o <<= 1) {
        int up = __shfl_up(pre, o, 64);
        if (lane >= o) pre += up;
    }
    return pre;
}
template <int NCELL, bool WALK = false>
__device__ inline int cells_prefix(int b, int n, int lane, int* s_pref, int* s_beg, int need = 0) {
    const int pre = cells_inclusive<NCELL>(n, lane);
    int total = 0;
    if (WALK) {
        total = __shfl(pre, NCELL - 1, 64);
        if (total < need) return total;
        __builtin_amdgcn_wave_barrier();
    }
    if (lane < NCELL) {
        s_pref[lane + 1] = pre;
        s_beg[lane] = b;
    }
    if (lane == 0) s_pref[0] = 0;
    if (!WALK) total = __shfl(pre, NCELL - 1, 64);
    __builtin_amdgcn_wave_barrier();
    return total;
}
// THE 3^3 look-up: lane c < 27 gets the point range [b, b + n) of cell (x, y, z) + (c % 3, c / 3 % 3, c / 9) - 1 of level
// `lev`; cells outside the root cube and the lanes from 27 up get n = 0.
__device__ inline void block27_ranges(const CellIndex& ci, int x, int y, int z, int lev, int lane, int& b, int& n) {
    const int lim = (1 << lev) - 1;
    b = 0;
    n = 0;
    if (lane < 27) {
        const int xx = x + lane % 3 - 1, yy = y + (lane / 3) % 3 - 1, zz = z + lane / 9 - 1;
        if (xx >= 0 && yy >= 0 && zz >= 0 && xx <= lim && yy <= lim && zz <= lim)
            cell_range(ci, asr_morton3d((u64)xx, (u64)yy, (u64)zz), lev, b, n);
    }
}
// ... and its tables.  The barrier a level loop needs before the writes is in the helper (cells_prefix, WALK), not at the
// call sites.
template <bool WALK = false>
__device__ inline int block27_cells(const CellIndex& ci, int x, int y, int z, int lev, int lane, int* s_pref, int* s_beg,
                                    int need = 0) {
    int b, n;
    block27_ranges(ci, x, y, z, lev, lane, b, n);
    return cells_prefix<27, WALK>(b, n, lane, s_pref, s_beg, need);
}
__device__ inline int radius_cells(const asr_octree_frame& f, const CellIndex& ci, float cx, float cy, float cz,
                                   float r, int lane, int* s_pref, int* s_beg) {
    const int lev = query_level(f, r);
    int x, y, z;
    frame_coord(f, cx, cy, cz, lev, x, y, z);
    return block27_cells(ci, x, y, z, lev, lane, s_pref, s_beg);
}

// ------------------------------------------------------------------------------------------
// ALIGNED queries (the aggregation search proper): query q is the centre of the grid voxel `keys[q]` = cell
// (x, y, z) of level L with radius = that level's cell size s.  The ball is then covered EXACTLY by the 4 x 4 x 4
// half-size cells (level L + 1) [2x-1, 2x+2]^3 -- a cube of side 2 s holding 1.9x the hits instead of the 6.4x of
// the 3 x 3 x 3 full-size cells.  "Exactly" has no margin, and the cell of a point (floor of a float product) and
// the centre of a voxel (a double rounded to float) carry rounding errors of up to 3 M 2^-24 level-21 units
// (M = largest coordinate magnitude in those units): a hit may sit in one of the first T = 2 + floor(3 M 2^-24)
// level-21 layers beyond a face of the cube -- then within sqrt(2 S T) + 2 T units of the axis through the voxel
// centre (S = voxel size in units), i.e. the "pole" of the ball.  k_radius_extras finds exactly those (point,
// voxel) pairs -- integer tests on the point codes, a handful of candidates per million points -- and the query
// kernels take them as additional candidates.  Levels whose half cell is narrower than 16 T units (and level 21)
// keep the 3 x 3 x 3 block of full-size cells, whose margin is half a cell.
// ------------------------------------------------------------------------------------------
constexpr int EXTRA_CAP = 1 << 16;
struct AlignedQ {
    const u64* keys;     // sorted voxel keys, one per query
    const int2* extras;  // (query, position in Morton order) pairs beyond the cube
    const int* extras_cnt;
    int lhalf_max;       // finest voxel level that uses half cells
};
__device__ inline int aligned_cells(const CellIndex& ci, const AlignedQ& aq, u64 key, int lane, int* s_pref, int* s_beg) {
    int x, y, z, lev;
    asr_key_coord(key, x, y, z, lev);
    int b = 0, n = 0;
    if (lev <= aq.lhalf_max) {
        const int lim = (2 << lev) - 1;
        const int xx = 2 * x - 1 + (lane & 3), yy = 2 * y - 1 + ((lane >> 2) & 3), zz = 2 * z - 1 + (lane >> 4);
        if (xx >= 0 && yy >= 0 && zz >= 0 && xx <= lim && yy <= lim && zz <= lim)
            cell_range(ci, asr_morton3d((u64)xx, (u64)yy, (u64)zz), lev + 1, b, n);
    } else {
        block27_ranges(ci, x, y, z, lev, lane, b, n);
    }
    return cells_prefix<64>(b, n, lane, s_pref, s_beg);
}
// candidate i of the concatenated cell ranges
template <int NCELL = 27>
__device__ inline float4 radius_candidate(const float4* sorted, const int* s_pref, const int* s_beg, int i,
                                          int* pos_out = nullptr) {
    int lo = 0, hi = NCELL;  // cell c with pref[c] <= i < pref[c+1]
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (s_pref[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    const int pos = s_beg[lo] + (i - s_pref[lo]);  // position in Morton order
    if (pos_out) *pos_out = pos;
    return sorted[pos];
}

// the (voxel, point) pairs of the rounding margin, see above.  One thread per point (position s in Morton order).
struct ExtraParams {
    int lmin, lmax;  // voxel levels to test (<= lhalf_max)
    int T;
    int rho[ASR_MAX_LEVEL + 1];  // pole radius in level-21 units per voxel level
};
__global__ void k_radius_extras(const u64* codes, const float4* sorted, i64 n, const u64* keys, i64 v, const float* centers,
                                const float* sizes, ExtraParams ep, int2* out, int* out_cnt) {
    const i64 s = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (s >= n) return;
    const u64 code = codes[s];
    const int c[3] = {(int)asr_compact21(code), (int)asr_compact21(code >> 1), (int)asr_compact21(code >> 2)};
    for (int lev = ep.lmin; lev <= ep.lmax; ++lev) {
        const int sh = ASR_MAX_LEVEL - lev, H = 1 << (sh - 1), S = 1 << sh;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int A = c[a] + H, m = A & (S - 1);
            int xa;
            if (m < ep.T)
                xa = (A >> sh) - 2;  // beyond the + face of voxel xa
            else if (m >= S - ep.T)
                xa = (A >> sh) + 1;  // beyond the - face
            else
                continue;
            const int b0 = (a + 1) % 3, b1 = (a + 2) % 3;
            const int y0 = c[b0] >> sh, y1 = c[b1] >> sh;
            if (abs(c[b0] - (y0 * S + H)) > ep.rho[lev] || abs(c[b1] - (y1 * S + H)) > ep.rho[lev]) continue;
            int xyz[3];
            xyz[a] = xa;
            xyz[b0] = y0;
            xyz[b1] = y1;
            const u64 key = asr_coord_key(xyz[0], xyz[1], xyz[2], lev);
            if (!key) continue;
            i64 lo = 0, hi = v;  // first voxel key >= key
            while (lo < hi) {
                const i64 mid = (lo + hi) >> 1;
                if (keys[mid] < key)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo >= v || keys[lo] != key) continue;
            const float4 pt = sorted[s];
            const float r = sizes[lo];
            if (sqdist3(pt.x, pt.y, pt.z, centers[3 * lo], centers[3 * lo + 1], centers[3 * lo + 2]) < r * r) {
                const int o = atomicAdd(out_cnt, 1);
                if (o < EXTRA_CAP) out[o] = make_int2((int)lo, (int)s);
            }
        }
    }
}

// end of a row of the aggregation search (MODE 2): the wave holds `found` hits, the first RADIUS_LIGHT of them as
// (distance bits | index) keys + Morton positions in LDS.  Heavy rows go to the list of k_radius_heavy; the others
// are ranked inside the wave (rank = number of smaller keys, keys are unique) and written, sorted, to the row's fixed
// slot tmp[q * RADIUS_LIGHT ..] as (distance, position in Morton order): k_radius_place turns the position back into
// the index with a clustered read.
__device__ __forceinline__ void radius_row_out(i64 q, i64 found, bool heavy, int lane, const u64* s_keys, const int* s_pos,
                                      i64* counts, u64* tmp, int32_t* heavy_out, int* heavy_cnt, uint8_t* is_heavy) {
    if (heavy) {  // counted and written by k_radius_heavy
        if (lane == 0) {
            counts[q] = 0;
            is_heavy[q] = 1;
            heavy_out[atomicAdd(heavy_cnt, 1)] = (int32_t)q;
        }
        return;
    }
    if (lane == 0) {
        counts[q] = found;
        is_heavy[q] = 0;
    }
    __builtin_amdgcn_wave_barrier();
    const int h = (int)found;
    u64 mine[RADIUS_LIGHT / 64];
    int mypos[RADIUS_LIGHT / 64];
    int rank[RADIUS_LIGHT / 64];
#pragma unroll
    for (int u = 0; u < RADIUS_LIGHT / 64; ++u) {
        mine[u] = lane + 64 * u < h ? s_keys[lane + 64 * u] : 0;
        mypos[u] = lane + 64 * u < h ? s_pos[lane + 64 * u] : 0;
        rank[u] = 0;
    }
    if (h <= 64) {  // (wave uniform; 19 of 20 rows)
        for (int j = 0; j < h; ++j) rank[0] += s_keys[j] < mine[0];  // LDS broadcast reads
    } else {
        for (int j = 0; j < h; ++j) {
            const u64 kj = s_keys[j];
#pragma unroll
            for (int u = 0; u < RADIUS_LIGHT / 64; ++u) rank[u] += kj < mine[u];
        }
    }
#pragma unroll
    for (int u = 0; u < RADIUS_LIGHT / 64; ++u)
        if (lane + 64 * u < h) tmp[q * RADIUS_LIGHT + rank[u]] = (mine[u] & 0xffffffff00000000ull) | (u32)mypos[u];
}

// one query of k_radius_query by one wave; s_*: the wave's LDS rows
template <int MODE, bool ALIGNED>
__device__ __forceinline__ void radius_query_one(const asr_octree_frame& f, const float4* sorted, const float* centers,
                                                 const float* sizes, i64 q, const CellIndex& ci, const AlignedQ& aq,
                                                 i64* counts, u64* tmp, int32_t* heavy_out, int* heavy_cnt, uint8_t* is_heavy,
                                                 int lane, int* s_pref, int* s_beg, u64* s_keys, int* s_pos) {
    constexpr int NCELL = ALIGNED ? 64 : 27;
    const float cx = centers[3 * q], cy = centers[3 * q + 1], cz = centers[3 * q + 2];
    const float r = sizes[q];
    const float r2 = r * r;
    const int total = ALIGNED ? aligned_cells(ci, aq, aq.keys[q], lane, s_pref, s_beg)
                              : radius_cells(f, ci, cx, cy, cz, r, lane, s_pref, s_beg);
    i64 found = 0;
    bool heavy = MODE == 2 && total > RADIUS_GIANT;
    for (int i0 = 0; i0 < total && !heavy; i0 += 64) {
        const int i = i0 + lane;
        bool hit = false;
        float d = 0.f;
        int id = 0, pos = 0;
        if (i < total) {
            const float4 pt = radius_candidate<NCELL>(sorted, s_pref, s_beg, i, &pos);
            d = sqdist3(pt.x, pt.y, pt.z, cx, cy, cz);
            hit = d < r2;
            id = __float_as_int(pt.w);
        }
        const unsigned long long m = __ballot(hit);
        if (MODE == 2 && hit) {
            const i64 o = found + __popcll(m & ((1ull << lane) - 1));
            if (o < RADIUS_LIGHT) {
                s_keys[o] = ((u64)__float_as_uint(d) << 32) | (u32)id;
                s_pos[o] = pos;
            }
        }
        found += __popcll(m);
        if (MODE == 2 && found > RADIUS_LIGHT) heavy = true;
    }
    if (ALIGNED) {  // the pairs of the rounding margin (k_radius_extras): normally none at all
        const int nex = min(*aq.extras_cnt, EXTRA_CAP);
        for (int e0 = 0; e0 < nex && !heavy; e0 += 64) {
            const int e = e0 + lane;
            bool hit = false;
            float d = 0.f;
            int id = 0, pos = 0;
            if (e < nex) {
                const int2 it = aq.extras[e];
                if (it.x == (int)q) {
                    pos = it.y;
                    const float4 pt = sorted[pos];
                    d = sqdist3(pt.x, pt.y, pt.z, cx, cy, cz);
                    hit = d < r2;
                    id = __float_as_int(pt.w);
                }
            }
            const unsigned long long m = __ballot(hit);
            if (MODE == 2 && hit) {
                const i64 o = found + __popcll(m & ((1ull << lane) - 1));
                if (o < RADIUS_LIGHT) {
                    s_keys[o] = ((u64)__float_as_uint(d) << 32) | (u32)id;
                    s_pos[o] = pos;
                }
            }
            found += __popcll(m);
            if (MODE == 2 && found > RADIUS_LIGHT) heavy = true;
        }
    }
    if (MODE == 0) {
        if (lane == 0) counts[q] = found;
        return;
    }
    radius_row_out(q, found, heavy, lane, s_keys, s_pos, counts, tmp, heavy_out, heavy_cnt, is_heavy);
}

// all queries 0..v (launch of ceil((v + 1) / 4) blocks), one query per wave
template <int MODE, bool ALIGNED>
__global__ __launch_bounds__(256) void k_radius_query(asr_octree_frame f, const float4* sorted,
                                                      const float* centers, const float* sizes,
                                                      i64 v, CellIndex ci, AlignedQ aq, i64* counts, u64* tmp,
                                                      int32_t* heavy_out, int* heavy_cnt,
                                                      uint8_t* is_heavy) {
    constexpr int NCELL = ALIGNED ? 64 : 27;
    __shared__ int s_pref[4][NCELL + 1];
    __shared__ int s_beg[4][NCELL];
    __shared__ u64 s_keys[MODE == 2 ? 4 : 1][RADIUS_LIGHT];
    __shared__ int s_pos[MODE == 2 ? 4 : 1][RADIUS_LIGHT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kw = MODE == 2 ? wave : 0;
    const i64 q = blockIdx.x * (i64)4 + wave;
    if (q == v && lane == 0) counts[v] = 0;
    if (q >= v) return;
    radius_query_one<MODE, ALIGNED>(f, sorted, centers, sizes, q, ci, aq, counts, tmp, heavy_out, heavy_cnt, is_heavy, lane,
                                    s_pref[wave], s_beg[wave], s_keys[kw], s_pos[kw]);
}

// ------------------------------------------------------------------------------------------
// Per-point attributes blended at arbitrary positions (asr_hip_point_attributes_at).  The search above with
// nothing written per pair: one wave per query walks the 3^3 cells of radius_cells, every lane tests its candidates with the
// search's predicate and keeps  sum w  and  sum w a[c]  in registers,
//     w = (min(R, 2 r) / max(R, 2 r))^2 * clamp((1 - d / R^2)^3, 0, 1)       (k_radius_place's compat x k_agg_importance),
// the wave adds the 64 partial sums with a fixed butterfly (same inputs, same bits) and, while the weight stays below
// min_weight, goes on to R = 2 R, 4 R, ... itself -- a wave-uniform loop, no relaunch.  A long row is a longer loop.
// sattr: the attributes in Morton order, CP (= C rounded up to 1, 2, 4, 8, 16) floats per point, so that the members of a
// query -- neighbours in that order -- are read from adjacent, 4 CP byte aligned records.
// ------------------------------------------------------------------------------------------
template <int CP>
__global__ void k_attr_permute(const float* attr, const int32_t* ids, i64 n, int c, float* sattr) {
    const i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= n * CP) return;
    const i64 s = i / CP;
    const int ch = (int)(i % CP);
    sattr[i] = ch < c ? attr[(i64)ids[s] * c + ch] : 0.f;
}
// levels of the cell table: the finest any query starts on (k = 0) and the coarsest any can widen to (k = max_widen)
__global__ __launch_bounds__(256) void k_attr_levels(asr_octree_frame f, const float* sizes, i64 m, float widen, int* cnt) {
    int lo = ASR_MAX_LEVEL, hi = 0;
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < m; i += (i64)gridDim.x * blockDim.x) {
        const float s = sizes[i];
        if (!(s > 0.f && s < INFINITY)) continue;  // such a row searches nothing
        hi = max(hi, query_level(f, s));
        lo = min(lo, query_level(f, s * widen));
    }
    block_level_range(lo, hi, cnt);
}
template <int CP>
__global__ __launch_bounds__(256) void k_attr_blend(asr_octree_frame f, const float4* __restrict__ sorted,
                                                    const float* __restrict__ srad, const float* __restrict__ sattr,
                                                    CellIndex ci, const float* __restrict__ positions,
                                                    const float* __restrict__ sizes, i64 m, int c, int max_widen,
                                                    float min_weight, float fill, float* __restrict__ out,
                                                    float* __restrict__ weight_out, int8_t* __restrict__ widen_out) {
    __shared__ int s_pref[4][28];
    __shared__ int s_beg[4][27];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 q = blockIdx.x * (i64)4 + wave;
    if (q >= m) return;  // (no block-wide barrier below)
    const float cx = positions[3 * q], cy = positions[3 * q + 1], cz = positions[3 * q + 2];
    const float s = sizes[q];
    int x21, y21, z21;
    const bool ok = frame_coord21_checked(f, cx, cy, cz, x21, y21, z21) && s > 0.f && s < INFINITY;
    float wsum = 0.f;
    float acc[CP], lo[CP], hi[CP];  // sums, and the members' range per channel: the blend is clamped to it, so that rounding
    int chosen = -1;                // never takes a convex combination out of its hull (a constant comes back exactly)
    float r = s;
    for (int k = 0; ok && k <= max_widen; ++k, r = r * 2.f) {
        const float r2 = r * r;
        const int total = radius_cells(f, ci, cx, cy, cz, r, lane, s_pref[wave], s_beg[wave]);
        wsum = 0.f;
#pragma unroll
        for (int ch = 0; ch < CP; ++ch) {
            acc[ch] = 0.f;
            lo[ch] = INFINITY;
            hi[ch] = -INFINITY;
        }
        for (int i0 = 0; i0 < total; i0 += 64) {
            const int i = i0 + lane;
            if (i >= total) continue;
            int pos;
            const float4 pt = radius_candidate<27>(sorted, s_pref[wave], s_beg[wave], i, &pos);
            const float d = sqdist3(pt.x, pt.y, pt.z, cx, cy, cz);
            if (!(d < r2)) continue;
            const float bb = 2 * srad[pos];
            const float ratio = fminf(r, bb) / fmaxf(r, bb);
            const float t = 1.f - d / r2;
            const float w = (ratio * ratio) * fminf(fmaxf(t * t * t, 0.f), 1.f);
            if (!(w > 0.f)) continue;  // (a point on the rim)
            wsum += w;
            float av[CP];
            if (CP >= 4) {
#pragma unroll
                for (int v = 0; v < CP / 4; ++v)
                    reinterpret_cast<float4*>(av)[v] = reinterpret_cast<const float4*>(sattr + (size_t)pos * CP)[v];
            } else {
#pragma unroll
                for (int ch = 0; ch < CP; ++ch) av[ch] = sattr[(size_t)pos * CP + ch];
            }
#pragma unroll
            for (int ch = 0; ch < CP; ++ch) {
                acc[ch] += w * av[ch];
                lo[ch] = fminf(lo[ch], av[ch]);
                hi[ch] = fmaxf(hi[ch], av[ch]);
            }
        }
        // fixed-order butterfly: every lane ends with the same sums
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            wsum += __shfl_xor(wsum, o, 64);
#pragma unroll
            for (int ch = 0; ch < CP; ++ch) acc[ch] += __shfl_xor(acc[ch], o, 64);
        }
        __builtin_amdgcn_wave_barrier();  // the cell tables in LDS are rewritten for the next radius
        if (wsum >= min_weight) {  // wave uniform
            chosen = k;
            break;
        }
    }
    float mine = fill;
    if (chosen >= 0) {
        float mlo = 0.f, mhi = 0.f;
#pragma unroll
        for (int ch = 0; ch < CP; ++ch)
            if (lane == ch) mine = acc[ch] / wsum;
        // the range of this lane's channel over the wave (min and max are exact in any order)
#pragma unroll
        for (int ch = 0; ch < CP; ++ch) {
            float l = lo[ch], h = hi[ch];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                l = fminf(l, __shfl_xor(l, o, 64));
                h = fmaxf(h, __shfl_xor(h, o, 64));
            }
            if (lane == ch) {
                mlo = l;
                mhi = h;
            }
        }
        mine = mine < mlo ? mlo : (mine > mhi ? mhi : mine);  // (a NaN stays a NaN)
    }
    if (lane < c) out[q * c + lane] = mine;
    if (lane == 0) {
        if (weight_out) weight_out[q] = chosen >= 0 ? wsum : 0.f;
        if (widen_out) widen_out[q] = (int8_t)chosen;
    }
}

// Cell ranges of the heavy rows, looked up ONCE per row (one wave each) and kept for the RADIUS_SPLIT x 4 waves of the
// counting pass and of the filling pass, which used to repeat the 27 / 64 table look-ups each (2 x 2 x 10^8 probes at
// 10 M points, three times the light rows' own)
constexpr int HC_LD = 65;  // ints per row in hc_pref (prefix, NCELL + 1 used) and hc_beg (NCELL used)
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_radius_heavy_cells(asr_octree_frame f, const float* centers, const float* sizes,
                                                            const int32_t* heavy, int nh, CellIndex ci, AlignedQ aq,
                                                            int* hc_pref, int* hc_beg) {
    constexpr int NCELL = ALIGNED ? 64 : 27;
    __shared__ int s_pref[4][NCELL + 1];
    __shared__ int s_beg[4][NCELL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 4 + wave;
    if (j >= nh) return;
    const i64 q = heavy[j];
    if (ALIGNED)
        aligned_cells(ci, aq, aq.keys[q], lane, s_pref[wave], s_beg[wave]);
    else
        radius_cells(f, ci, centers[3 * q], centers[3 * q + 1], centers[3 * q + 2], sizes[q], lane, s_pref[wave], s_beg[wave]);
    __builtin_amdgcn_wave_barrier();
    if (lane <= NCELL) hc_pref[(i64)j * HC_LD + lane] = s_pref[wave][lane];
    if (NCELL == 64 && lane == 0) hc_pref[(i64)j * HC_LD + 64] = s_pref[wave][64];
    if (lane < NCELL) hc_beg[(i64)j * HC_LD + lane] = s_beg[wave][lane];
}

// Heavy rows: RADIUS_SPLIT blocks per row, each block walks 1/RADIUS_SPLIT of the candidates.
// FILL = false: accumulates the hit count into counts[q]; FILL = true: writes the (distance, index)
// keys at hoff[j] + cursor (any order: the rows are sorted by a segmented sort afterwards).
template <bool FILL, bool ALIGNED>
__global__ __launch_bounds__(256) void k_radius_heavy(asr_octree_frame f, const float4* sorted, const float* centers,
                                                      const float* sizes, const int32_t* heavy, CellIndex ci, AlignedQ aq,
                                                      i64* counts, const i64* hoff, int* cursor, u64* keys_out,
                                                      int32_t* row_out, const int* hc_pref, const int* hc_beg,
                                                      int idx_bits) {
    // idx_bits > 0 (FILL): ONE sortable key per hit, (row j, squared distance bits, index) = row_bits + 31 + idx_bits
    // <= 64 bits (distances are >= 0: the sign bit is dropped) -- the rows are then ordered by a single keys-only
    // radix sort; idx_bits == 0: (distance bits << 32 | index) + the row in row_out, two stable sorts
    constexpr int NCELL = ALIGNED ? 64 : 27;
    __shared__ int s_pref[4][NCELL + 1];
    __shared__ int s_beg[4][NCELL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x;
    const int total = hc_pref[(i64)j * HC_LD + NCELL];  // (k_radius_heavy_cells)
    int per = (total + RADIUS_SPLIT - 1) / RADIUS_SPLIT;
    per = (per + 255) & ~255;  // whole 4-wave rounds
    const int lo = blockIdx.y * per;
    const int hi = min(total, lo + per);
    if (lo >= total && !(ALIGNED && blockIdx.y == 0)) return;  // (block 0 also walks the pairs of the rounding margin)
    const i64 q = heavy[j];
    const float cx = centers[3 * q], cy = centers[3 * q + 1], cz = centers[3 * q + 2];
    const float r = sizes[q];
    const float r2 = r * r;
    if (lane <= NCELL) s_pref[wave][lane] = hc_pref[(i64)j * HC_LD + lane];
    if (NCELL == 64 && lane == 0) s_pref[wave][64] = total;
    if (lane < NCELL) s_beg[wave][lane] = hc_beg[(i64)j * HC_LD + lane];
    __builtin_amdgcn_wave_barrier();
    unsigned long long found = 0;
    auto consume = [&](bool hit, float d, int id) {
        const unsigned long long m = __ballot(hit);
        if (FILL && m) {
            int o0 = 0;
            if (lane == 0) o0 = atomicAdd(&cursor[j], __popcll(m));
            o0 = __shfl(o0, 0, 64);
            if (hit) {
                const i64 o = hoff[j] + o0 + __popcll(m & ((1ull << lane) - 1));
                if (idx_bits > 0) {
                    keys_out[o] = ((u64)j << (31 + idx_bits)) | ((u64)__float_as_uint(d) << idx_bits) | (u32)id;
                } else {
                    keys_out[o] = ((u64)__float_as_uint(d) << 32) | (u32)id;
                    row_out[o] = j;
                }
            }
        }
        found += __popcll(m);
    };
    for (int i0 = lo + wave * 64; i0 < hi; i0 += 256) {
        const int i = i0 + lane;
        bool hit = false;
        float d = 0.f;
        int id = 0;
        if (i < hi) {
            const float4 pt = radius_candidate<NCELL>(sorted, s_pref[wave], s_beg[wave], i);
            d = sqdist3(pt.x, pt.y, pt.z, cx, cy, cz);
            hit = d < r2;
            id = __float_as_int(pt.w);
        }
        consume(hit, d, id);
    }
    if (ALIGNED && blockIdx.y == 0 && wave == 0) {  // pairs of the rounding margin, once per row
        const int nex = min(*aq.extras_cnt, EXTRA_CAP);
        for (int e0 = 0; e0 < nex; e0 += 64) {
            const int e = e0 + lane;
            bool hit = false;
            float d = 0.f;
            int id = 0;
            if (e < nex) {
                const int2 it = aq.extras[e];
                if (it.x == (int)q) {
                    const float4 pt = sorted[it.y];
                    d = sqdist3(pt.x, pt.y, pt.z, cx, cy, cz);
                    hit = d < r2;
                    id = __float_as_int(pt.w);
                }
            }
            if (__ballot(hit)) consume(hit, d, id);
        }
    }
    if (!FILL && lane == 0 && found) atomicAdd((unsigned long long*)&counts[q], found);
}
// copies the light rows from their fixed slots to the CSR positions: 16 lanes per row.  The slots hold
// (squared distance, position in Morton order); index and radius come from the Morton-ordered arrays
// (neighbours of one voxel are close in that order: clustered reads instead of one line per pair)
__global__ void k_radius_place(const u64* tmp, const i64* rs, const uint8_t* is_heavy, i64 v, const float* sizes,
                               const int32_t* ids, const float* srad, int32_t* idx, int32_t* spos, float* dist,
                               float* compat) {
    const i64 q = (blockIdx.x * (i64)blockDim.x + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    if (q >= v) return;
    const i64 b = rs[q];
    const int cnt = (int)(rs[q + 1] - b);
    if (is_heavy[q]) return;  // written by k_radius_unpack_heavy
    const float a = sizes[q];
    for (int i = l; i < cnt; i += 16) {
        const u64 k = tmp[q * RADIUS_LIGHT + i];
        const int32_t pos = (int32_t)(k & 0xffffffffu);
        idx[b + i] = ids[pos];
        if (spos) spos[b + i] = pos;
        dist[b + i] = __uint_as_float((unsigned)(k >> 32));
        if (compat) {
            float bb = 2 * srad[pos];
            float ratio = fminf(a, bb) / fmaxf(a, bb);
            compat[b + i] = ratio * ratio;
        }
    }
}
__global__ void k_heavy_counts(const int32_t* heavy, i64 nh, const i64* rs, i64* cnt) {
    i64 j = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (j > nh) return;
    cnt[j] = j < nh ? rs[heavy[j] + 1] - rs[heavy[j]] : 0;
}
__global__ void k_radius_unpack_heavy(const u64* keys, const int32_t* hrow, i64 num_pairs, const int32_t* heavy,
                                      const i64* hoff, const i64* rs, const float* sizes, const float* radii,
                                      const int32_t* rank, int32_t* idx, int32_t* spos, float* dist, float* compat,
                                      int idx_bits) {
    i64 p = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (p >= num_pairs) return;
    u64 k = keys[p];
    int j;
    if (idx_bits > 0) {  // (row, distance bits, index) in one key: see k_radius_heavy
        j = (int)(k >> (31 + idx_bits));
        k = (((k >> idx_bits) & 0x7fffffffull) << 32) | (k & ((u64(1) << idx_bits) - 1));
    } else {
        j = hrow[p];
    }
    const i64 q = heavy[j];
    const i64 o = rs[q] + (p - hoff[j]);
    const int32_t id = (int32_t)(k & 0xffffffffu);
    idx[o] = id;
    if (spos) spos[o] = rank[id];
    dist[o] = __uint_as_float((unsigned)(k >> 32));
    if (compat) {
        float a = sizes[q];
        float bb = 2 * radii[id];
        float ratio = fminf(a, bb) / fmaxf(a, bb);
        compat[o] = ratio * ratio;
    }
}
// ------------------------------------------------------------------------------------------
// THE LEVEL WALK of the nearest-neighbour searches (k_knn, k_nearest, k_icp_pairs, k_knn_index): one wave per query,
// level by level from a start level towards the root, until a level's result is provably that of the whole cloud.
// Written once: nearest_walk<CAPPED> below is k_nearest's and k_icp_pairs' search.  k_knn and k_knn_index share the
//   look-up (block27_ranges) and this description; their start level, prefix and face test stay written out in the
//   kernels, in the order they had: with the helpers (crowded_start_level, cells_prefix, block_face_gap, candidate_key)
//   the two compiled to other schedules, measured 0.4 % (knn_index) and 1.5 % (knn_radius) slower, and written out
//   they compile to the instructions they had before the look-up was shared.
// Block: on level `lev` lanes 0..26 look up the 3^3 cells around the query's cell (block27_ranges; a block with too few
//   points for the caller is skipped before its tables are written) and the wave walks the block's points 64 at a
//   time (radius_candidate).  Results are (squared distance bits << 32 | point index) keys, so ties go to the smallest
//   index.  A query outside the root cube is clamped into a boundary cell; the block of level 0 is the whole cloud.
// Crowding start (crowded_start_level): the walk starts on the finest table level lfine, or -- in a cloud with dense
//   spots, whose codes are sorted down to ldeep > lfine -- on the level at which the query's own cell holds at most
//   KNN_CROWD points; cells below lfine are found by binary search in the sorted codes (cell_range).
// Face gap (block_face_gap): a point that is NOT in the block lies beyond one of the block's six faces, so it is at least
//   as far away as that face; faces on the root cube's boundary do not count (points beyond them were clamped into the
//   boundary cells, which the block holds).  g is the distance to the nearest counting face, shrunk by the rounding
//   margin, and the statement every exit rests on is: every point outside the block has a COMPUTED squared distance of at
//   least g * g.  Margin: a point is binned by floor(fl(p * inv)) and the face position is computed as
//   fl(fl(c) * voxel_size), where inv * voxel_size = 1 +- 2^-23.  A point beyond the face at integer coordinate c has
//   p < F + |F| 2^-23 with F = c / inv, the computed face f is within |F| 2^-22 of F, and sqdist3 loses at most 2^-22
//   relative: the gap q - f is shrunk to (q - f)(1 - 2^-20) - |f| 2^-20, which covers all of it several times over.  The
//   margin bounds what sqdist3 can lose against the true gap, whatever value g * g is then compared with.
// Exits: nearest_walk leaves when its best key has d2 < g * g.  On an empty block (best = ~0, whose distance bits are a
//   NaN: the comparison would be false) it moves on at once.  CAPPED (only points with d2 <= cap2 count) adds the exit
//   cap2 < g * g: all points outside the block are then beyond the cap, so the best of the block, if it is within the cap,
//   is the best of the cloud within the cap -- and a query with no counterpart leaves at the first level whose cells are
//   wider than the cap instead of climbing to the whole cloud.  k_knn_index puts its k-th key in place of the best; the
//   test d2_k < g * g is strict, so a point outside the block cannot even tie with the k-th key and no smaller index is
//   lost at the block's boundary.  k_knn (distances only, queries are points of the cloud, hence inside their centre
//   cell) keeps its own exit d_k <= (cell size)^2.
// ------------------------------------------------------------------------------------------
constexpr int KNN_CROWD = 1024;  // points of a finest-level cell above which a point starts its search on a finer level
__device__ inline int crowded_start_level(const CellIndex& ci, u64 code, int lfine, int ldeep) {
    int lev0 = lfine;
    if (ldeep > lfine) {
        int b0, pop;
        cell_range(ci, code >> (3 * (ASR_MAX_LEVEL - lfine)), lfine, b0, pop);
        while (pop > KNN_CROWD && lev0 < ldeep) {
            ++lev0;
            cell_range(ci, code >> (3 * (ASR_MAX_LEVEL - lev0)), lev0, b0, pop);
        }
    }
    return lev0;
}
// floor(t) + off clamped into [0, 2^21): k_point_codes' cell for points of the cube, the nearest boundary cell outside
__device__ inline int clamped_cell21(float t, int off) {
    const float ft = fminf(fmaxf(floorf(t), -4.0e9f), 4.0e9f);
    const i64 c = (i64)ft + off, lim = (1 << ASR_MAX_LEVEL) - 1;
    return (int)(c < 0 ? 0 : c > lim ? lim : c);
}
// the level-21 cell of a finite query
__device__ inline void query_cell21(const asr_octree_frame& f, float qx, float qy, float qz, int& cx, int& cy, int& cz) {
    const float inv = f.inv_voxel_size[ASR_MAX_LEVEL];
    cx = clamped_cell21(qx * inv, f.offset[0]);
    cy = clamped_cell21(qy * inv, f.offset[1]);
    cz = clamped_cell21(qz * inv, f.offset[2]);
}
__device__ inline bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }
// Morton code of a query's level-21 cell, the sort key of the query order; non-finite rows last
__device__ inline u64 query_code21(const asr_octree_frame& f, float qx, float qy, float qz) {
    if (!finite3(qx, qy, qz)) return (u64(1) << 63) - 1;
    int cx, cy, cz;
    query_cell21(f, qx, qy, qz, cx, cy, cz);
    return asr_morton3d((u64)cx, (u64)cy, (u64)cz);
}
// distance from q to the nearer of the block's two faces on one axis, shrunk by the rounding margin; +inf for a face
// on the root cube's boundary, negative when q lies outside the block.  c = centre cell of the block on `lev`.
__device__ inline float nearest_face_gap(const asr_octree_frame& f, float q, int c, int lev, int off) {
    const int s = ASR_MAX_LEVEL - lev;
    const float vs = f.voxel_size[ASR_MAX_LEVEL];
    const float keep = 0.99999904632568359375f, slack = 9.5367431640625e-7f;  // 1 - 2^-20, 2^-20
    float g = __uint_as_float(0x7f800000u);
    if (c - 1 > 0) {
        const float face = (float)(((i64)(c - 1) << s) - off) * vs;
        g = fminf(g, (q - face) * keep - fabsf(face) * slack);
    }
    if (c + 2 < (1 << lev)) {
        const float face = (float)(((i64)(c + 2) << s) - off) * vs;
        g = fminf(g, (face - q) * keep - fabsf(face) * slack);
    }
    return g;
}
// g of the block around cell (x, y, z) of level `lev`
__device__ inline float block_face_gap(const asr_octree_frame& f, float qx, float qy, float qz, int x, int y, int z, int lev) {
    return fminf(fminf(nearest_face_gap(f, qx, x, lev, f.offset[0]), nearest_face_gap(f, qy, y, lev, f.offset[1])),
                 nearest_face_gap(f, qz, z, lev, f.offset[2]));
}
__device__ inline u64 shfl_xor_u64(u64 v, int o) {
    const u32 hi = __shfl_xor((u32)(v >> 32), o, 64), lo = __shfl_xor((u32)v, o, 64);
    return ((u64)hi << 32) | lo;
}
__device__ inline u64 shfl_u64(u64 v, int src) {
    const u32 hi = __shfl((u32)(v >> 32), src, 64), lo = __shfl((u32)v, src, 64);
    return ((u64)hi << 32) | lo;
}
// (squared distance bits << 32) | original point index of candidate pt for the query (qx, qy, qz)
__device__ inline u64 candidate_key(const float4& pt, float qx, float qy, float qz) {
    return ((u64)__float_as_uint(sqdist3(pt.x, pt.y, pt.z, qx, qy, qz)) << 32) | (u64)(u32)__float_as_int(pt.w);
}
// The walk for ONE nearest point of one finite query by one wave: the smallest key of the final level's block, the same
// value in every lane; ~0 when that block is empty (CAPPED only: level 0 holds all n >= 1 points).
template <bool CAPPED>
__device__ __forceinline__ u64 nearest_walk(const asr_octree_frame& f, const float4* __restrict__ sorted,
                                            const CellIndex& ci, int lfine, int ldeep, float qx, float qy, float qz,
                                            float cap2, int lane, int* s_pref, int* s_beg) {
    int cx, cy, cz;
    query_cell21(f, qx, qy, qz, cx, cy, cz);
    const int lev0 = crowded_start_level(ci, asr_morton3d((u64)cx, (u64)cy, (u64)cz), lfine, ldeep);
    u64 best = ~u64(0);
    for (int lev = lev0; lev >= 0; --lev) {
        const int s = ASR_MAX_LEVEL - lev;
        const int x = cx >> s, y = cy >> s, z = cz >> s;
        const int total = block27_cells<true>(ci, x, y, z, lev, lane, s_pref, s_beg, 1);
        if (!CAPPED && total == 0) continue;  // only the cap can end the walk on an empty block
        if (total > 0) {
            for (int i0 = 0; i0 < total; i0 += 64) {
                const int i = i0 + lane;
                if (i < total) {
                    const u64 key = candidate_key(radius_candidate(sorted, s_pref, s_beg, i), qx, qy, qz);
                    best = key < best ? key : best;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const u64 other = shfl_xor_u64(best, o);
                best = other < best ? other : best;
            }
        }
        if (lev == 0) break;
        const float g = block_face_gap(f, qx, qy, qz, x, y, z, lev);
        if (g > 0.f && (__uint_as_float((u32)(best >> 32)) < g * g || (CAPPED && cap2 < g * g))) break;
    }
    return best;
}

// Exact k-th nearest neighbour distance, one wave per point (in Morton order): the level walk above with the query's cell
// taken from frame_coord (from the sorted codes below lfine).  If a block holds >= k points the k-th smallest squared
// distance d_k among them is selected; it is exact as soon as d_k <= (cell size)^2, because every point closer than one
// cell size lies inside the 3^3 block.
// Selection: binary search on the bit pattern of the (non-negative) squared distances with wave
// ballots; up to 512 candidates are held in registers, larger sets are streamed from memory.
__global__ __launch_bounds__(256) void k_knn(asr_octree_frame f, const float4* sorted, i64 n, CellIndex ci, int lfine,
                                             int ldeep, int k, const float* radii_in, float radius_fraction,
                                             int outlier_threshold, float* radii_out,
                                             uint8_t* inlier_out, const int32_t* list, i64 nlist) {
    constexpr int CMAX = 8;
    __shared__ int s_pref[4][28];
    __shared__ int s_beg[4][28];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    i64 s = blockIdx.x * (i64)4 + wave;
    if (list) {  // only the points (positions in Morton order) that k_knn_cells could not settle
        if (s >= nlist) return;
        s = list[s];
    }
    if (s >= n) return;
    const float4 me = sorted[s];
    const int kk = (int)(n < k ? n : k);
    u32 kth_bits = 0;
    u32 bound_bits = 0x7f800000u;  // upper bound of the answer (+inf until a level has been evaluated)
    int total = 0;
    // Start level: the finest table level, or -- for a point in a crowded cell of a cloud with dense spots (ldeep >
    // lfine: the codes are sorted that deep) -- the level at which its own cell holds at most KNN_CROWD points; cells
    // below the table's finest level are found by binary search in the sorted codes (cell_range).
    int lev0 = lfine;
    if (ldeep > lfine) {
        const u64 code = ci.codes[s];
        int b0, pop;
        cell_range(ci, code >> (3 * (ASR_MAX_LEVEL - lfine)), lfine, b0, pop);
        while (pop > KNN_CROWD && lev0 < ldeep) {
            ++lev0;
            cell_range(ci, code >> (3 * (ASR_MAX_LEVEL - lev0)), lev0, b0, pop);
        }
    }
    for (int lev = lev0; lev >= 0; --lev) {
        int x, y, z;
        if (lev > lfine) {  // the point's cell as the sorted codes have it
            const u64 cell = ci.codes[s] >> (3 * (ASR_MAX_LEVEL - lev));
            x = (int)asr_compact21(cell);
            y = (int)asr_compact21(cell >> 1);
            z = (int)asr_compact21(cell >> 2);
        } else {
            frame_coord(f, me.x, me.y, me.z, lev, x, y, z);
        }
        const int lim = (1 << lev) - 1;
        x = min(max(x, 0), lim);  // points outside the root cube were clamped into it
        y = min(max(y, 0), lim);
        z = min(max(z, 0), lim);
        int b, cnt;
        block27_ranges(ci, x, y, z, lev, lane, b, cnt);
        int pre = cnt;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            int up = __shfl_up(pre, o, 64);
            if (lane >= o) pre += up;
        }
        total = __shfl(pre, 26, 64);
        if (total < kk && lev > 0) continue;
        __builtin_amdgcn_wave_barrier();
        if (lane < 27) {
            s_pref[wave][lane + 1] = pre;
            s_beg[wave][lane] = b;
        }
        if (lane == 0) s_pref[wave][0] = 0;
        __builtin_amdgcn_wave_barrier();
        auto cand = [&](int i) -> float {
            int lo = 0, hi = 27;
            while (hi - lo > 1) {
                int mid = (lo + hi) >> 1;
                if (s_pref[wave][mid] <= i)
                    lo = mid;
                else
                    hi = mid;
            }
            const float4 pt = sorted[s_beg[wave][lo] + (i - s_pref[wave][lo])];
            return sqdist3(pt.x, pt.y, pt.z, me.x, me.y, me.z);
        };
        const int need = total < kk ? total : kk;  // lev == 0 with fewer than k points overall
        // Selection of the need-th smallest squared distance: one pass over the candidates that keeps a
        // pool of 8 values per lane.  Only values <= bound enter, where bound is an upper bound of the
        // answer: the result of the finer level (k-th among a subset of these candidates) and, once a
        // lane's slots are full, the need-th smallest of the pool itself.  (The previous version ran a
        // 31-pass bit search over ALL candidates of every level it tried: an isolated point whose
        // 3^3 block is a coarse cell next to a dense region walked 10^6 candidates 31 times.)
        u32 pool[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) pool[c] = 0x7f800000u;
        int nl = 0;  // used slots of this lane
        bool overflow = false;
        // need-th smallest of the pool = largest bit pattern t with #{pool < t} < need
        auto select = [&]() {
            u32 lo_bits = 0;
            for (int bit = 30; bit >= 0; --bit) {
                const u32 trial = lo_bits | (1u << bit);
                int c_lt = 0;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) c_lt += __popcll(__ballot(pool[c] < trial));
                if (c_lt < need) lo_bits = trial;
            }
            return lo_bits;
        };
        for (int i0 = 0; i0 < total && !overflow; i0 += 64) {
            const int i = i0 + lane;
            const u32 db = i < total ? __float_as_uint(cand(i)) : 0x7f800001u;
            if (__ballot(db <= bound_bits && nl == CMAX)) {
                // a lane is full: tighten the bound to the pool's need-th smallest and drop the rest
                int have = 0;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) have += __popcll(__ballot(pool[c] != 0x7f800000u));
                if (have >= need) {
                    const u32 nb = select();
                    if (nb < bound_bits) bound_bits = nb;
                }
                u32 keep[CMAX];
                int m = 0;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) keep[c] = 0x7f800000u;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    const bool k2 = pool[c] <= bound_bits && pool[c] != 0x7f800000u;
#pragma unroll
                    for (int e = 0; e < CMAX; ++e)
                        if (k2 && e == m) keep[e] = pool[c];
                    m += k2;
                }
#pragma unroll
                for (int c = 0; c < CMAX; ++c) pool[c] = keep[c];
                nl = m;
                if (__ballot(db <= bound_bits && nl == CMAX)) overflow = true;  // > 8 ties on one lane
            }
            if (!overflow && db <= bound_bits) {
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (c == nl) pool[c] = db;
                ++nl;
            }
        }
        u32 lo_bits = 0;
        if (!overflow) {
            lo_bits = select();
        } else {  // pathological (hundreds of equal distances): bit search over the stream
            for (int bit = 30; bit >= 0; --bit) {
                const u32 trial = lo_bits | (1u << bit);
                int c_lt = 0;
                for (int i0 = 0; i0 < total; i0 += 64) {
                    const int i = i0 + lane;
                    const bool lt = i < total && __float_as_uint(cand(i)) < trial;
                    c_lt += __popcll(__ballot(lt));
                }
                if (c_lt < need) lo_bits = trial;
            }
        }
        bound_bits = lo_bits;  // k-th among a subset of the next (coarser) level's candidates
        kth_bits = lo_bits;
        const float cs = f.voxel_size[lev];
        if (lev == 0 || __uint_as_float(kth_bits) <= cs * cs) {
            // exact.  Optional inlier vote (KDTree::ComputeInlier): neighbours among the k nearest
            // whose radius is below radius_fraction * radius_i
            if (inlier_out) {
                // The vote is over exactly `need` neighbours, like the k results of a kNN query
                // (nsearch.cpp:62-80): all candidates strictly closer than the k-th distance, plus as
                // many of the candidates AT that distance as are needed to reach k, taken in ascending
                // point index (which tie a k-d tree returns is traversal dependent; this is the
                // deterministic rule, and the one the brute-force check in the tests uses).
                const float thr = radii_in[__float_as_int(me.w)] * radius_fraction;
                auto cand_pt = [&](int i) -> float4 {
                    int lo = 0, hi = 27;
                    while (hi - lo > 1) {
                        int mid = (lo + hi) >> 1;
                        if (s_pref[wave][mid] <= i)
                            lo = mid;
                        else
                            hi = mid;
                    }
                    return sorted[s_beg[wave][lo] + (i - s_pref[wave][lo])];
                };
                int c_lt = 0, n_eq = 0, votes_lt = 0, votes_eq = 0;
                for (int i0 = 0; i0 < total; i0 += 64) {
                    const int i = i0 + lane;
                    bool lt = false, eq = false, voter = false;
                    if (i < total) {
                        const float4 pt = cand_pt(i);
                        const u32 db = __float_as_uint(sqdist3(pt.x, pt.y, pt.z, me.x, me.y, me.z));
                        lt = db < kth_bits;
                        eq = db == kth_bits;
                        voter = (lt || eq) && radii_in[__float_as_int(pt.w)] < thr;
                    }
                    c_lt += __popcll(__ballot(lt));
                    n_eq += __popcll(__ballot(eq));
                    votes_lt += __popcll(__ballot(lt && voter));
                    votes_eq += __popcll(__ballot(eq && voter));
                }
                const int admit = need - c_lt;  // >= 1: the k-th neighbour itself sits at kth_bits
                if (n_eq > admit) {
                    // more ties than places: the `admit` smallest indices among them (bit search)
                    u32 idx_hi = 0;  // largest t with #{ties with index < t} < admit == the admit-th smallest index
                    for (int bit = 30; bit >= 0; --bit) {
                        const u32 trial = idx_hi | (1u << bit);
                        int below = 0;
                        for (int i0 = 0; i0 < total; i0 += 64) {
                            const int i = i0 + lane;
                            bool b2 = false;
                            if (i < total) {
                                const float4 pt = cand_pt(i);
                                b2 = __float_as_uint(sqdist3(pt.x, pt.y, pt.z, me.x, me.y, me.z)) == kth_bits &&
                                     (u32)__float_as_int(pt.w) < trial;
                            }
                            below += __popcll(__ballot(b2));
                        }
                        if (below < admit) idx_hi = trial;
                    }
                    votes_eq = 0;
                    for (int i0 = 0; i0 < total; i0 += 64) {
                        const int i = i0 + lane;
                        bool v = false;
                        if (i < total) {
                            const float4 pt = cand_pt(i);
                            v = __float_as_uint(sqdist3(pt.x, pt.y, pt.z, me.x, me.y, me.z)) == kth_bits &&
                                (u32)__float_as_int(pt.w) <= idx_hi && radii_in[__float_as_int(pt.w)] < thr;
                        }
                        votes_eq += __popcll(__ballot(v));
                    }
                }
                const int votes = votes_lt + votes_eq;
                if (lane == 0) inlier_out[__float_as_int(me.w)] = votes < outlier_threshold ? 1 : 0;
            }
            break;
        }
    }
    if (lane == 0 && radii_out) radii_out[__float_as_int(me.w)] = sqrtf(__uint_as_float(kth_bits));
}

// ------------------------------------------------------------------------------------------
// kNN radius, fast path: ONE WAVE PER OCCUPIED CELL of the finest level.  All points of a cell share the 3^3
// block of candidate cells, so the wave stages the candidates in LDS 64 at a time and every lane keeps the K
// smallest squared distances of ITS query point in registers (ascending; inserting d and dropping the largest is
// a[c] = med3(a[c-1], d, a[c]) from the top down: one v_med3_f32 per slot, no divergence; a chunk no lane can use
// is skipped with one ballot).  The wave-per-point kernel above spends 27 table probes, a candidate walk and two
// 31-step bit searches on every point.  A result is exact when the k-th distance does not exceed the cell size
// (the k nearest lie inside the block); the other points -- sparse regions, cells with fewer than k candidates
// -- go to a list that k_knn settles level by level as before.  Same numbers as k_knn (tested).  Measured and not
// kept: cells one level coarser (43 vs 26 ms), one wave per parent cell with the 4^3 block of finest cells as
// candidates (fuller waves, but 2.3x the candidates per query: 20.5 vs 16.7 ms).
// ------------------------------------------------------------------------------------------
// largest population of a level-`level` cell (table slots hold [start, end) per (cell, level))
__global__ void k_max_cell_pop(HashTab t, const int32_t* start, const int32_t* end, int level, int* out) {
    const u64 slot = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (slot > t.mask) return;
    const u64 key = t.keys[slot];
    if (key == 0 || asr_key_level(key) != level) return;
    const int pop = end[slot] - start[slot];
    if (pop > KNN_CROWD) atomicMax(out, pop);
}

// first point of every run of equal level-`level` cells in the sorted codes.  4096 points per block, ONE atomic per
// block for the block's share of the list (same-address atomics retire at ~88 / us).
__global__ __launch_bounds__(256) void k_cell_list(const u64* codes, i64 n, int level, int32_t* list, int* cnt) {
    __shared__ int s_cnt[256];
    __shared__ int s_base;
    const int s = 3 * (ASR_MAX_LEVEL - level);
    const i64 base = blockIdx.x * (i64)4096;
    int mine = 0;
    unsigned flags = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const i64 i = base + j * 256 + threadIdx.x;
        if (i < n && (i == 0 || (codes[i - 1] >> s) != (codes[i] >> s))) {
            flags |= 1u << j;
            ++mine;
        }
    }
    s_cnt[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int t = 0; t < 256; ++t) {
            const int c = s_cnt[t];
            s_cnt[t] = tot;
            tot += c;
        }
        s_base = tot ? atomicAdd(cnt, tot) : 0;
    }
    __syncthreads();
    int o = s_base + s_cnt[threadIdx.x];
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (flags & (1u << j)) list[o++] = (int32_t)(base + j * 256 + threadIdx.x);
}

constexpr int KNN_CELL_MAX_WORK = 12288;  // passes of 64 queries x candidates of the 3^3 block a wave may take on (~0.5 ms)
template <int K>
__global__ __launch_bounds__(256) void k_knn_cells(asr_octree_frame f, const float4* sorted, i64 n, HashTab t,
                                                   const int32_t* start, const int32_t* end, int lfine, int k,
                                                   const int32_t* cells, i64 ncells, float* radii_out,
                                                   int32_t* fallback, int* fallback_cnt) {
    __shared__ int s_pref[4][28];
    __shared__ int s_beg[4][28];
    __shared__ __attribute__((aligned(16))) float4 s_cand[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 ci = blockIdx.x * (i64)4 + wave;
    if (ci >= ncells) return;
    const int first = cells[ci];
    const float4 p0 = sorted[first];
    int x, y, z;
    frame_coord(f, p0.x, p0.y, p0.z, lfine, x, y, z);
    const int lim = (1 << lfine) - 1;
    x = min(max(x, 0), lim);
    y = min(max(y, 0), lim);
    z = min(max(z, 0), lim);
    int b = 0, cnt = 0;
    if (lane < 27) {
        // Not block27_cells: the candidate cells come nearest first (the cell itself, 6 face, 12 edge, 8 corner
        // neighbours) -- the k-th distance is tight after the first few, and chunks of the far cells are skipped by the
        // ballot test below -- and lfine is a table level, so the table is probed directly.
        constexpr unsigned char order[27] = {13, 4, 10, 12, 14, 16, 22, 1, 3, 5, 7, 9, 11, 15, 17, 19, 21, 23, 25,
                                             0, 2, 6, 8, 18, 20, 24, 26};
        const int c = order[lane];
        int xx = x + c % 3 - 1, yy = y + (c / 3) % 3 - 1, zz = z + c / 9 - 1;
        if (xx >= 0 && yy >= 0 && zz >= 0 && xx <= lim && yy <= lim && zz <= lim) {
            i64 slot = tab_find_slot(t, asr_morton3d((u64)xx, (u64)yy, (u64)zz) | (u64(1) << (3 * lfine)));
            if (slot >= 0) {
                b = start[slot];
                cnt = end[slot] - b;
            }
        }
    }
    // The prefix is cells_prefix's; the total and the tables are written out in this order: through cells_prefix the
    // tables cost two LDS writes under a branch instead of one paired write, and knn_radius was 1.5 % slower.
    const int pre = cells_inclusive<27>(cnt, lane);
    const int total = __shfl(pre, 26, 64);
    const int qb = __shfl(b, 0, 64), qn = __shfl(cnt, 0, 64);  // the cell itself: its points are the queries
    if (lane < 27) {
        s_pref[wave][lane + 1] = pre;
        s_beg[wave][lane] = b;
    }
    if (lane == 0) s_pref[wave][0] = 0;
    __builtin_amdgcn_wave_barrier();
    const float cs = f.voxel_size[lfine];
    const float cs2 = cs * cs;
    // Crowded cells go to the wave-per-point kernel: this wave would walk points x candidates alone (a dense spot of
    // 10^5 points in one cell: 10^10 distance evaluations on one SIMD; such a cloud took 312 s before this line).
    if (total < k || (i64)((qn + 63) / 64) * total > KNN_CELL_MAX_WORK) {
        for (int q0 = lane; q0 < qn; q0 += 64) fallback[atomicAdd(fallback_cnt, 1)] = qb + q0;
        return;
    }
    for (int q0 = 0; q0 < qn; q0 += 64) {
        const bool active = q0 + lane < qn;
        const float4 me = sorted[qb + (active ? q0 + lane : 0)];
        float a[K];  // squared distances are >= 0 and finite: float order, +inf = empty
#pragma unroll
        for (int c = 0; c < K; ++c) a[c] = __uint_as_float(0x7f800000u);
        if (total >= k) {
            for (int c0 = 0; c0 < total; c0 += 64) {
                const int m = min(64, total - c0);
                __builtin_amdgcn_wave_barrier();  // the previous chunk has been read
                if (lane < m) s_cand[wave][lane] = radius_candidate(sorted, s_pref[wave], s_beg[wave], c0 + lane);
                __builtin_amdgcn_wave_barrier();
                for (int j = 0; j < m; ++j) {
                    const float4 pt = s_cand[wave][j];
                    const float d = sqdist3(pt.x, pt.y, pt.z, me.x, me.y, me.z);
                    if (__ballot(d < a[K - 1]) == 0) continue;
#pragma unroll
                    for (int c = K - 1; c > 0; --c) a[c] = __builtin_amdgcn_fmed3f(a[c - 1], d, a[c]);
                    a[0] = fminf(a[0], d);
                }
            }
        }
        float kth = a[K - 1];
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (c == k - 1) kth = a[c];
        if (active) {
            if (total >= k && kth <= cs2)
                radii_out[__float_as_int(me.w)] = sqrtf(kth);
            else
                fallback[atomicAdd(fallback_cnt, 1)] = qb + q0 + lane;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Nearest point of ANOTHER set (asr_hip_nearest_point): one wave per query, queries taken in Morton order so that
// neighbouring waves probe the same cells; nearest_walk without a cap.
// ------------------------------------------------------------------------------------------
__global__ void k_query_codes(asr_octree_frame f, const float* q, i64 m, u64* codes, int32_t* ids) {
    const i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= m) return;
    codes[i] = query_code21(f, q[3 * i], q[3 * i + 1], q[3 * i + 2]);
    ids[i] = (int32_t)i;
}
__global__ __launch_bounds__(256) void k_nearest(asr_octree_frame f, const float4* __restrict__ sorted, CellIndex ci,
                                                 int lfine, int ldeep, const float* __restrict__ queries,
                                                 const int32_t* __restrict__ order, i64 m, int32_t* index_out,
                                                 float* sqdist_out) {
    __shared__ int s_pref[4][28];
    __shared__ int s_beg[4][28];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 w = blockIdx.x * (i64)4 + wave;
    if (w >= m) return;
    const i64 j = order[w];
    const float qx = queries[3 * j], qy = queries[3 * j + 1], qz = queries[3 * j + 2];
    if (!finite3(qx, qy, qz)) {
        if (lane == 0) {
            if (index_out) index_out[j] = -1;
            if (sqdist_out) sqdist_out[j] = __uint_as_float(0x7f800000u);
        }
        return;
    }
    const u64 best = nearest_walk<false>(f, sorted, ci, lfine, ldeep, qx, qy, qz, 0.f, lane, s_pref[wave], s_beg[wave]);
    if (lane == 0) {
        if (index_out) index_out[j] = (int32_t)(u32)best;
        if (sqdist_out) sqdist_out[j] = __uint_as_float((u32)(best >> 32));
    }
}

// ------------------------------------------------------------------------------------------
// One ICP step (asr_hip_icp_step): the transformed source points are the queries of nearest_walk, capped at a distance
// (only points with d2 <= cap2 count), and the terms of the normal equations are accumulated behind it.
// Sums: no float atomics.  The queries are taken in the Morton order of q; wave w owns the ICP_RUN consecutive queries
// from w * ICP_RUN, lane t < 28 keeps entry t of (ata[21], atb[6], sq_residual) in a register across the run, lane 28
// sq_distance, lane 29 the pair count.  The four waves of a block are added in wave order, k_icp_fold adds the blocks'
// partials in a fixed order: the bits depend on the inputs alone.
// ------------------------------------------------------------------------------------------
struct IcpTransform {
    double t[12];  // rows of (R | t)
    double o[3];
};
constexpr int ICP_RUN = 32;     // queries per wave
constexpr int ICP_TERMS = 30;   // 21 + 6 + 2 sums, the pair count
constexpr int ICP_STRIDE = 32;  // doubles per partial
constexpr int ICP_FOLD = 32;    // strided chains of k_icp_fold
__global__ void k_icp_codes(asr_octree_frame f, IcpTransform x, const float* __restrict__ src, i64 m, float* __restrict__ q,
                            u64* codes, int32_t* ids) {
    const i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= m) return;
    const float px = src[3 * i], py = src[3 * i + 1], pz = src[3 * i + 2];
    float qx = __uint_as_float(0x7fc00000u), qy = qx, qz = qx;
    if (finite3(px, py, pz)) {
        qx = (float)(((x.t[0] * (double)px + x.t[1] * (double)py) + x.t[2] * (double)pz) + x.t[3]);
        qy = (float)(((x.t[4] * (double)px + x.t[5] * (double)py) + x.t[6] * (double)pz) + x.t[7]);
        qz = (float)(((x.t[8] * (double)px + x.t[9] * (double)py) + x.t[10] * (double)pz) + x.t[11]);
    }
    q[3 * i] = qx;
    q[3 * i + 1] = qy;
    q[3 * i + 2] = qz;
    codes[i] = query_code21(f, qx, qy, qz);  // rows without a finite q last
    ids[i] = (int32_t)i;
}
// the row (a, r) of one pair and one direction n: (e0..e5) = (u x n, n), e6 = r; d = u - v.  Named members and a chain of
// selects: an array indexed by the lane's entry would be placed in LDS.
struct IcpRow {
    double e0, e1, e2, e3, e4, e5, e6;
};
__device__ inline IcpRow icp_row(double ux, double uy, double uz, double dx, double dy, double dz, double nx, double ny,
                                 double nz) {
    IcpRow e;
    e.e0 = uy * nz - uz * ny;
    e.e1 = uz * nx - ux * nz;
    e.e2 = ux * ny - uy * nx;
    e.e3 = nx;
    e.e4 = ny;
    e.e5 = nz;
    e.e6 = (nx * dx + ny * dy) + nz * dz;
    return e;
}
__device__ inline double icp_pick(const IcpRow& e, int k) {
    return k == 0 ? e.e0 : k == 1 ? e.e1 : k == 2 ? e.e2 : k == 3 ? e.e3 : k == 4 ? e.e4 : k == 5 ? e.e5 : e.e6;
}
__device__ inline double icp_term(const IcpRow& e, int ti, int tj) { return icp_pick(e, ti) * icp_pick(e, tj); }
template <bool PLANE>
__global__ __launch_bounds__(256) void k_icp_pairs(asr_octree_frame f, const float4* __restrict__ sorted, CellIndex ci,
                                                   int lfine, int ldeep, const float* __restrict__ q,
                                                   const int32_t* __restrict__ order, i64 m,
                                                   const float* __restrict__ target, const float* __restrict__ normals,
                                                   double ox, double oy, double oz, float cap2, int32_t* index_out,
                                                   double* __restrict__ partial) {
    __shared__ int s_pref[4][28];
    __shared__ int s_beg[4][28];
    __shared__ double s_part[4][ICP_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // entry `lane` of the sums is e[ti] * e[tj]: the upper triangle of a a^T row by row, then a r, then r r
    int ti = 6, tj = 6;
    if (lane < 21) {
        ti = 0;
        int rem = lane;
        while (rem >= 6 - ti) {
            rem -= 6 - ti;
            ++ti;
        }
        tj = ti + rem;
    } else if (lane < 27) {
        ti = lane - 21;
    }
    double acc = 0.0;
    i64 pairs = 0;
    const i64 first = (blockIdx.x * (i64)4 + wave) * ICP_RUN;
    const i64 last = first + ICP_RUN < m ? first + ICP_RUN : m;
    for (i64 w = first; w < last; ++w) {
        const i64 j = order[w];
        const float qx = q[3 * j], qy = q[3 * j + 1], qz = q[3 * j + 2];
        int32_t hit = -1;
        float yx = 0.f, yy = 0.f, yz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
        if (finite3(qx, qy, qz)) {
            const u64 best = nearest_walk<true>(f, sorted, ci, lfine, ldeep, qx, qy, qz, cap2, lane, s_pref[wave], s_beg[wave]);
            if (best != ~u64(0) && __uint_as_float((u32)(best >> 32)) <= cap2) {
                hit = (int32_t)(u32)best;
                yx = target[3 * (i64)hit];
                yy = target[3 * (i64)hit + 1];
                yz = target[3 * (i64)hit + 2];
                if (PLANE) {
                    nx = normals[3 * (i64)hit];
                    ny = normals[3 * (i64)hit + 1];
                    nz = normals[3 * (i64)hit + 2];
                    if (!finite3(nx, ny, nz) || (nx == 0.f && ny == 0.f && nz == 0.f)) hit = -1;
                }
            }
        }
        if (lane == 0 && index_out) index_out[j] = hit;
        if (hit < 0) continue;  // (the same decision in every lane)
        ++pairs;
        const double ux = (double)qx - ox, uy = (double)qy - oy, uz = (double)qz - oz;
        const double vx = (double)yx - ox, vy = (double)yy - oy, vz = (double)yz - oz;
        const double dx = ux - vx, dy = uy - vy, dz = uz - vz;
        double term;
        if (lane == 28) {
            term = (dx * dx + dy * dy) + dz * dz;
        } else if (PLANE) {
            term = icp_term(icp_row(ux, uy, uz, dx, dy, dz, (double)nx, (double)ny, (double)nz), ti, tj);
        } else {
            const double t0 = icp_term(icp_row(ux, uy, uz, dx, dy, dz, 1.0, 0.0, 0.0), ti, tj);
            const double t1 = icp_term(icp_row(ux, uy, uz, dx, dy, dz, 0.0, 1.0, 0.0), ti, tj);
            const double t2 = icp_term(icp_row(ux, uy, uz, dx, dy, dz, 0.0, 0.0, 1.0), ti, tj);
            term = (t0 + t1) + t2;
        }
        acc += term;
    }
    if (lane < ICP_TERMS) s_part[wave][lane] = lane == 29 ? __longlong_as_double(pairs) : acc;
    __syncthreads();
    if (wave == 0 && lane < ICP_TERMS) {
        double out;
        if (lane == 29)
            out = __longlong_as_double(((__double_as_longlong(s_part[0][29]) + __double_as_longlong(s_part[1][29])) +
                                        __double_as_longlong(s_part[2][29])) +
                                       __double_as_longlong(s_part[3][29]));
        else
            out = ((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane];
        partial[blockIdx.x * (i64)ICP_STRIDE + lane] = out;
    }
}
// sums[t] = the partials of entry t: chain g of ICP_FOLD adds the blocks g, g + ICP_FOLD, ... in that order, then the chains
// are added in order.  One block of 32 * ICP_FOLD threads; entry 29 (the pair count) is an integer.
__global__ __launch_bounds__(32 * ICP_FOLD) void k_icp_fold(const double* __restrict__ partial, i64 nb, double* __restrict__ sums) {
    __shared__ double s_chain[ICP_FOLD][32];
    const int t = threadIdx.x & 31, g = threadIdx.x >> 5;
    double acc = 0.0;
    i64 cnt = 0;
    if (t < ICP_TERMS)
        for (i64 b = g; b < nb; b += ICP_FOLD) {
            const double v = partial[b * ICP_STRIDE + t];
            if (t == 29)
                cnt += __double_as_longlong(v);
            else
                acc += v;
        }
    s_chain[g][t] = t == 29 ? __longlong_as_double(cnt) : acc;
    __syncthreads();
    if (g == 0 && t < ICP_TERMS) {
        acc = 0.0;
        cnt = 0;
        for (int c = 0; c < ICP_FOLD; ++c) {
            if (t == 29)
                cnt += __double_as_longlong(s_chain[c][t]);
            else
                acc += s_chain[c][t];
        }
        sums[t] = t == 29 ? __longlong_as_double(cnt) : acc;
    }
}

// ------------------------------------------------------------------------------------------
// Exact k-nearest-neighbour LISTS (asr_hip_knn_index): one wave per point in Morton order, the level walk with the k-th
// key in place of the best.  The best 64 (squared distance bits << 32 | point index) keys seen on a level are one key per
// lane, ascending over the lanes; row i of the output is the first k of them.  Candidates come 64 at a time: a batch in
// which no key lies below the current k-th one (a ballot) is skipped, one with at most KNN_INSERT such keys has them
// inserted one by one, any other is sorted by a bitonic network of lane shuffles, reversed and merged: min(best[l],
// batch[63 - l]) is a bitonic sequence that holds the 64 smallest of the 128, six more compare-exchange steps sort it.
// Keys are distinct (the index is part of them), so the order (d2, index) is total.  A level that is not accepted hands
// its k-th key down as a bound (its block is a subset of the next one's), and the list starts again, because the next
// block holds the same points once more.
// ------------------------------------------------------------------------------------------
constexpr int KNN_INSERT = 12;  // survivors of a batch up to which they are inserted one by one instead of sorted and merged
__global__ __launch_bounds__(256) void k_knn_index(asr_octree_frame f, const float4* __restrict__ sorted, i64 n, CellIndex ci,
                                                   int lfine, int ldeep, int k, int32_t* __restrict__ index_out,
                                                   float* __restrict__ sqdist_out) {
    __shared__ int s_pref[4][28];
    __shared__ int s_beg[4][28];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 s = blockIdx.x * (i64)4 + wave;
    if (s >= n) return;
    const float4 me = sorted[s];
    const u64 code = ci.codes[s];  // the point's level-21 cell as the index has it
    const int cx = (int)asr_compact21(code), cy = (int)asr_compact21(code >> 1), cz = (int)asr_compact21(code >> 2);
    const int kk = (int)(n < k ? n : k);
    int lev0 = lfine;
    if (ldeep > lfine) {  // crowded cells start deeper, as in k_knn
        int b0, pop;
        cell_range(ci, code >> (3 * (ASR_MAX_LEVEL - lfine)), lfine, b0, pop);
        while (pop > KNN_CROWD && lev0 < ldeep) {
            ++lev0;
            cell_range(ci, code >> (3 * (ASR_MAX_LEVEL - lev0)), lev0, b0, pop);
        }
    }
    u64 best = ~u64(0);   // lane l: the l-th smallest key of this level so far
    u64 bound = ~u64(0);  // the k-th key of a finer level: no key of the answer is larger
    for (int lev = lev0; lev >= 0; --lev) {
        const int sh = ASR_MAX_LEVEL - lev;
        const int x = cx >> sh, y = cy >> sh, z = cz >> sh;
        int b, cnt;
        block27_ranges(ci, x, y, z, lev, lane, b, cnt);
        int pre = cnt;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const int up = __shfl_up(pre, o, 64);
            if (lane >= o) pre += up;
        }
        const int total = __shfl(pre, 26, 64);
        if (total < kk && lev > 0) continue;  // (level 0 holds all n >= kk points)
        __builtin_amdgcn_wave_barrier();
        if (lane < 27) {
            s_pref[wave][lane + 1] = pre;
            s_beg[wave][lane] = b;
        }
        if (lane == 0) s_pref[wave][0] = 0;
        __builtin_amdgcn_wave_barrier();
        best = ~u64(0);
        u64 worst = bound;  // min(bound, current k-th key): a candidate above it cannot enter the first k
        for (int i0 = 0; i0 < total; i0 += 64) {
            const int i = i0 + lane;
            u64 key = ~u64(0);
            if (i < total) {
                const float4 pt = radius_candidate(sorted, s_pref[wave], s_beg[wave], i);
                key = ((u64)__float_as_uint(sqdist3(pt.x, pt.y, pt.z, me.x, me.y, me.z)) << 32) |
                      (u64)(u32)__float_as_int(pt.w);
            }
            if (key > worst) key = ~u64(0);
            unsigned long long live = __ballot(key != ~u64(0));
            if (!live) continue;
            if (__popcll(live) <= KNN_INSERT) {
                // few survivors (every batch but the first ones of a level): each is inserted where it belongs -- the keys
                // below it are a prefix of the lanes, the rest moves up by one lane and the last key falls off
                while (live) {
                    const int src = __ffsll((long long)live) - 1;
                    live &= live - 1;
                    const u64 c = shfl_u64(key, src);
                    if (c > worst) continue;  // (the k-th key has come down meanwhile)
                    const int pos = __popcll(__ballot(best < c));
                    const u32 uhi = __shfl_up((u32)(best >> 32), 1, 64), ulo = __shfl_up((u32)best, 1, 64);
                    best = lane < pos ? best : (lane == pos ? c : (((u64)uhi << 32) | ulo));
                    const u64 kth = shfl_u64(best, kk - 1);
                    worst = kth < bound ? kth : bound;
                }
                continue;
            }
            // bitonic sort of the batch, ascending over the lanes
#pragma unroll
            for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
                for (int o = size >> 1; o > 0; o >>= 1) {
                    const u64 other = shfl_xor_u64(key, o);
                    const bool take_min = ((lane & o) == 0) == ((lane & size) == 0);
                    key = take_min ? (other < key ? other : key) : (other > key ? other : key);
                }
            }
            const u64 rev = shfl_u64(key, 63 - lane);
            best = rev < best ? rev : best;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const u64 other = shfl_xor_u64(best, o);
                best = (lane & o) == 0 ? (other < best ? other : best) : (other > best ? other : best);
            }
            const u64 kth = shfl_u64(best, kk - 1);
            worst = kth < bound ? kth : bound;
        }
        if (lev == 0) break;
        const u64 kth = shfl_u64(best, kk - 1);
        const float g = fminf(fminf(nearest_face_gap(f, me.x, x, lev, f.offset[0]), nearest_face_gap(f, me.y, y, lev, f.offset[1])),
                              nearest_face_gap(f, me.z, z, lev, f.offset[2]));
        if (g > 0.f && kth != ~u64(0) && __uint_as_float((u32)(kth >> 32)) < g * g) break;
        bound = kth < bound ? kth : bound;
    }
    if (lane < k) {
        const i64 row = (i64)__float_as_int(me.w) * k + lane;
        const bool have = lane < kk && best != ~u64(0);
        if (index_out) index_out[row] = have ? (int32_t)(u32)best : -1;
        if (sqdist_out) sqdist_out[row] = have ? __uint_as_float((u32)(best >> 32)) : __uint_as_float(0x7f800000u);
    }
}

// rows are sorted by a segmented radix sort on (distance bits, index) keys; unpack + compat
// ------------------------------------------------------------------------------------------
// a11: CSR inversion
// ------------------------------------------------------------------------------------------
__global__ void k_invert_hist(const int32_t* idx, i64 p, i64* counts, i64 num_points) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i < p) atomicAdd((unsigned long long*)&counts[idx[i]], 1ull);
    (void)num_points;
}
__global__ void k_iota32(int32_t* out, i64 n) {
    i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int32_t)i;
}
__global__ void k_invert_fill(const int32_t* sorted_src, i64 p, const i64* rs, i64 num_rows,
                              const uint8_t* attr, int32_t* out_idx, uint8_t* out_attr) {
    i64 d = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (d >= p) return;
    i64 src = sorted_src[d];
    // row of pair src: largest q with rs[q] <= src
    i64 lo = 0, hi = num_rows;
    while (hi - lo > 1) {
        i64 mid = (lo + hi) >> 1;
        if (rs[mid] <= src)
            lo = mid;
        else
            hi = mid;
    }
    out_idx[d] = (int32_t)lo;
    if (attr) out_attr[d] = attr[src];
}

// ------------------------------------------------------------------------------------------
// row regrouping for the MFMA sparse conv: rows of one CSR are reordered inside segments of
// `seg` consecutive rows so that rows with the same set of kernel slots sit in the same 16-row
// MFMA tile (ascending 55-bit slot mask).  Purely a tiling order: results do not depend on it.
//
// One routine for one list and for the 13 CSRs of a grid hierarchy (5 neighbour lists, 4 up lists, 4 inverted up
// lists): ONE radix sort + one chunk sort instead of 13 x (2..3 sorts) -- on the small levels each rocPRIM sort is
// a dozen launches of a few microseconds.  Rows of all jobs live in one index space, every job padded to a
// multiple of 128 rows; key = job | segment | slot mask (or its rank among the distinct masks), each field as wide
// as the jobs at hand need: the stable sort leaves each job's rows contiguous, ordered by (segment, mask, row).
// Padding rows take the all-ones segment, which no real segment uses, and so sort last inside their job.
// ------------------------------------------------------------------------------------------
constexpr int RG_MAX_JOBS = 16;  // what the argument struct holds; more lists run in groups
struct RowGroupBatch {
    int n;
    i64 base[RG_MAX_JOBS + 1];  // first padded row of each job (multiples of 128); base[n] = total
    i64 v[RG_MAX_JOBS];
    const uint8_t* kidx[RG_MAX_JOBS];
    const i64* rs[RG_MAX_JOBS];
    int32_t* out[RG_MAX_JOBS];
};
// the (job, segment) field of a key; segment < 0: a padding row
__device__ inline u64 rg_job_segment(int j, i64 segment, int seg_bits) {
    return ((u64)j << seg_bits) | (segment < 0 ? (u64(1) << seg_bits) - 1 : (u64)segment);
}
// Slot mask of every row (0 for padding rows).  For ranked keys (t.keys set) the distinct masks >> shift are gathered in a
// small hash set: all but the first insertion of a mask are read-only probes.
__global__ void k_rg_masks(RowGroupBatch b, u64* masks, int32_t* ids, int shift, HashTab t, int* cnt) {
    const i64 e = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (e >= b.base[b.n]) return;
    const int j = job_of(b, e);
    const i64 r = e - b.base[j];
    u64 m = 0;
    if (r < b.v[j]) {
        const i64* rs = b.rs[j];
        const uint8_t* kidx = b.kidx[j];
        for (i64 p = rs[r]; p < rs[r + 1]; ++p) m |= u64(1) << (kidx[p] & 63);
        if (t.keys && tab_insert_shared(t, (m >> shift) + 1) < 0) cnt[F_OVERFLOW] = 1;
    }
    masks[e] = m;
    if (ids) ids[e] = (int32_t)e;  // (ranked keys: k_rg_keys_ranked writes them; beside the probes the store costs 17 us at 10 M points)
}
// key = (job, segment, slot mask >> shift) in job_bits + seg_bits + mask_bits <= 64 bits
__global__ void k_rg_keys(RowGroupBatch b, i64 seg, const u64* masks, u64* keys, int seg_bits, int mask_bits, int shift) {
    const i64 e = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (e >= b.base[b.n]) return;
    const int j = job_of(b, e);
    const i64 r = e - b.base[j];
    const u64 ones = (u64(1) << mask_bits) - 1;
    keys[e] = r < b.v[j] ? (rg_job_segment(j, r / seg, seg_bits) << mask_bits) | ((masks[e] >> shift) & ones)
                         : (rg_job_segment(j, -1, seg_bits) << mask_bits) | ones;
}
// Longest-processing-time order of the 128-row chunks inside each segment: a chunk's cost is the number of slots in the
// union of its rows' masks, per 64-row tile (one weight panel walk + barrier per slot), so heavy tiles start first and the
// tail of a launch is made of light ones.  key = (job, segment of the chunk's position, 127 - cost); one wave per chunk.
__global__ void k_rg_chunk_keys(RowGroupBatch b, i64 seg, const int32_t* sorted_ids, const u64* masks, int32_t* ckey,
                                int32_t* cid, int seg_bits) {
    const i64 c = (blockIdx.x * (i64)blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (c * 128 >= b.base[b.n]) return;
    const int j = job_of(b, c * 128);
    const i64 r0 = c * 128 - b.base[j];
    u64 m0 = masks[sorted_ids[c * 128 + lane]], m1 = masks[sorted_ids[c * 128 + 64 + lane]];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m0 |= __shfl_xor(m0, o, 64);
        m1 |= __shfl_xor(m1, o, 64);
    }
    if (lane == 0) {
        int cost = __popcll(m0) + __popcll(m1);  // the two 64-row tiles of the chunk
        if (r0 + 128 > b.v[j]) cost = 0;         // the partial chunk stays last
        ckey[c] = (int32_t)((rg_job_segment(j, r0 / seg, seg_bits) << 7) | (u64)(127 - cost));
        cid[c] = (int32_t)c;
    }
}
__global__ void k_rg_apply(RowGroupBatch b, const int32_t* sorted_ids, const int32_t* order, int lpt) {
    const i64 e = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (e >= b.base[b.n]) return;
    const int j = job_of(b, e);
    const i64 r = e - b.base[j];
    if (r >= b.v[j]) return;
    const i64 src = lpt ? (i64)order[e >> 7] * 128 + (e & 127) : e;
    b.out[j][r] = (int32_t)(sorted_ids[src] - b.base[j]);
}

// Ranked keys (round 4): a hierarchy has a few thousand DISTINCT slot masks, so the 54 mask bits of the sort key are replaced
// by the mask's rank among the distinct masks (same order, same permutation): (job, segment, rank) is at most 22 bits -- three
// digit passes over all 13 lists in one sort instead of three passes over the 9-slot lists plus eight over the 55-slot ones.
// Distinct masks: the hash set k_rg_masks filled, collected into a dense list (k_rg_mask_collect) and ranked by counting
// (k_rg_mask_ranks), rank written back as the set's value.  More than RG_MAX_MASKS distinct masks, or a key of more than
// 32 bits: the caller falls back to the full-mask keys.
constexpr int RG_MAX_MASKS = 16384;  // (C3: ~1 500 distinct masks, mixed-density C5: more than 4 096)
constexpr int RG_MASK_TAB = 65536;
// the set's keys as a dense list (any order) with their slots; cnt[F_MASKS] = how many
__global__ void k_rg_mask_collect(HashTab t, u64* list, int32_t* slot_of, int* cnt) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    const u64 k = i <= t.mask ? t.keys[i] : 0;
    const int o = block_append(k != 0, cnt + F_MASKS);
    if (k && o < RG_MAX_MASKS) {
        list[o] = k;
        slot_of[o] = (int32_t)i;
    }
}
// rank of every distinct mask = number of smaller ones (the masks are distinct): one thread per mask, the list read through
// LDS tiles.  (Round 4: this was a bitonic sort by ONE workgroup, 0.5 ms alone and 1.3 ms beside the search's query kernel,
// whose waves share that CU's issue slots -- on the critical chain of the build.)
__global__ __launch_bounds__(256) void k_rg_mask_ranks(HashTab t, const u64* list, const int32_t* slot_of, const int* cnt) {
    __shared__ u64 s_key[2048];
    const int n = cnt[F_MASKS];
    if (n > RG_MAX_MASKS) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x * blockDim.x >= n) return;
    const u64 mine = i < n ? list[i] : 0;
    int rank = 0;
    for (int base = 0; base < n; base += 2048) {
        __syncthreads();
        for (int e = threadIdx.x; e < 2048; e += blockDim.x) s_key[e] = base + e < n ? list[base + e] : ~u64(0);
        __syncthreads();
        const int m = min(2048, n - base);
        for (int e = 0; e < m; ++e) rank += s_key[e] < mine;  // (LDS broadcast reads)
    }
    if (i < n) t.vals[slot_of[i]] = rank;
}
// key = (job, segment, rank of the slot mask >> shift) in job_bits + seg_bits + rank_bits <= 32 bits, of row order[i] (of row
// i without an order).  rank_bits = 0 leaves (job, segment): the second of two stable sorts, over rows already in mask order.
__global__ void k_rg_keys_ranked(RowGroupBatch b, i64 seg, const u64* masks, const int32_t* order, HashTab t, unsigned* keys,
                                 int32_t* ids, int seg_bits, int rank_bits, int shift) {
    const i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (i >= b.base[b.n]) return;
    const i64 e = order ? order[i] : i;
    if (!order) ids[i] = (int32_t)i;
    const int j = job_of(b, e);
    const i64 r = e - b.base[j];
    const u64 low = r >= b.v[j] ? (u64(1) << rank_bits) - 1 : rank_bits ? (u64)tab_find(t, (masks[e] >> shift) + 1) : 0;
    keys[i] = (unsigned)((rg_job_segment(j, r < b.v[j] ? r / seg : -1, seg_bits) << rank_bits) | low);
}

// ------------------------------------------------------------------------------------------
// dual cells ("next" row D.1): CreateDualVertexIndices, cpp/lib/grid.cpp:316-459 with the vertex /
// adjacent-node key algebra of cpp/lib/octreebase.h:86-118.  One thread per leaf, 8 corners each.
// ------------------------------------------------------------------------------------------
__device__ inline u64 dev_morton_add(u64 a, u64 b) {
    const u64 M = 0x9249249249249249ull;
    u64 c = ((a | ~M) + (b & M)) & M;
    c |= ((a | ~(M << 1)) + (b & (M << 1))) & (M << 1);
    c |= ((a | ~(M << 2)) + (b & (M << 2))) & (M << 2);
    return c;
}
__device__ inline u64 dev_morton_sub(u64 a, u64 b) {
    const u64 M = 0x9249249249249249ull;
    u64 c = ((a & M) - (b & M)) & M;
    c |= ((a & (M << 1)) - (b & (M << 1))) & (M << 1);
    c |= ((a & (M << 2)) - (b & (M << 2))) & (M << 2);
    return c;
}
// map: node key -> leaf index, or -1 for inner nodes; returns -2 when the key is no node
__device__ inline int node_lookup(const HashTab& t, u64 key) {
    TabProbe pr = tab_probe(t, key);
    for (u64 probe = 0; probe <= pr.bmask; ++probe, pr.next()) {
        const u64 slot = pr.slot();
        const u64 cur = t.keys[slot];
        if (cur == key) return t.vals[slot];
        if (cur == 0) return -2;
    }
    return -2;
}
// does leaf `key` own the dual cell of its corner i? (grid.cpp:334-360)
__device__ inline bool dual_owned(const HashTab& t, u64 key, int i, u64& vertex_key) {
    const u64 IM = 0x9249249249249249ull;
    const int lev = asr_key_level(key);
    const u64 min_lev_key = u64(1) << (3 * lev);
    const u64 vk = dev_morton_add(key, (u64)i);
    const u64 vk_ = vk - min_lev_key;
    if (vk >= (min_lev_key << 1) || !(vk_ & IM) || !(vk_ & (IM << 1)) || !(vk_ & (IM << 2))) return false;
    vertex_key = vk;
    for (int j = 0; j < 8; ++j) {
        if (j == i) continue;
        const u64 ak = dev_morton_sub(vk, (u64)j);
        const int r = node_lookup(t, ak);
        if (r == -2) continue;        // no node there: this leaf is the deeper one
        if (r == -1) return false;    // inner node: one of its children owns the vertex
        if (ak < key) return false;   // same-level leaf with the smaller key owns it
    }
    return true;
}
__global__ void k_dual_count(const u64* leaves, i64 v, HashTab t, i64* counts) {
    i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (q > v) return;
    if (q == v) {
        counts[v] = 0;
        return;
    }
    const u64 key = leaves[q];
    int n = 0;
    u64 vk;
    for (int i = 0; i < 8; ++i) n += dual_owned(t, key, i, vk) ? 1 : 0;
    counts[q] = n;
}
__global__ void k_dual_fill(const u64* leaves, i64 v, HashTab t, const i64* offsets, i64* out, int* cnt) {
    i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (q >= v) return;
    const u64 key = leaves[q];
    i64 o = offsets[q];
    for (int i = 0; i < 8; ++i) {
        u64 vk;
        if (!dual_owned(t, key, i, vk)) continue;
        for (int j = 0; j < 8; ++j) {
            u64 k = dev_morton_sub(vk, (u64)j);
            int r = -2;
            while (k != 0 && (r = node_lookup(t, k)) == -2) k >>= 3;  // grid.cpp:429-441
            if (k == 0 || r < 0) {
                cnt[F_DUAL_KEY] = 1;  // "invalid key after searching for node" / "found node is not a leaf"
                r = -1;
            }
            out[o * 8 + j] = r;
        }
        ++o;
    }
}

// ------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------
int make_table(asr_hip_context* ctx, Arena& arena, u64 cap, bool with_vals, HashTab& t) {
    t.keys = arena_alloc<u64>(arena, cap);
    t.vals = with_vals ? arena_alloc<int32_t>(arena, cap) : nullptr;
    t.mask = cap - 1;
    if (!t.keys || (with_vals && !t.vals)) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, hipMemsetAsync(t.keys, 0, cap * sizeof(u64), ctx->stream));
    return ASR_HIP_OK;
}

}  // namespace

// ==========================================================================================
// entry points used by asr_api.hip
// ==========================================================================================
int asr_geom_point_keys(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts,
                        const float* radii, i64 n, float radius_scale, int max_depth, u64* keys) {
    if (n <= 0) return ASR_HIP_OK;
    k_point_keys<<<grid_for(n, BLK), BLK, 0, ctx->stream>>>(*frame, pts, radii, n, radius_scale,
                                                            max_depth, keys);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

// Result: ctx->nodes / ctx->leaves (sorted) in the persist arena.
// Octree::Grow: the grown key set of `grow_steps` iterations as a device list in `arena` (see k_grow_*)
static int grow_keys(asr_hip_context* ctx, Arena& arena, const asr_octree_frame* frame, const float* pts, const float* radii,
                     i64 n, float radius_scale, int max_depth, int grow_steps, u64** keys_out, i64* count_out) {
    HostFlags host;
    u64 cap = next_pow2((u64)std::max<i64>(i64(1) << 16, 8 * n));
    for (int attempt = 0; attempt < 6; ++attempt, cap <<= 2) {
        if (attempt) ++ctx->table_regrows;
        HashTab t;
        ASR_TRY(make_table(ctx, arena, cap, false, t));
        const int lcap = (int)std::min<u64>(cap / 2, u64(1) << 30);
        u64* list = arena_alloc<u64>(arena, (size_t)lcap + 8);
        if (!list) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        ASR_TRY(fresh_flags(ctx));
        k_grow_init<<<grid_for(n, BLK), BLK, 0, ctx->stream>>>(*frame, pts, radii, n, radius_scale, max_depth, t,
                                                             ctx->d_flags, list, lcap);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(read_flags(ctx, host));
        if (host[F_BAD_KEY]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "octree: extra_keys holds a value that is no location code (0 or a leading "
                                                   "bit that is not at 3 * level)");
        if (host[F_NONFINITE]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "octree: points / radii contain non-finite values");
        bool overflow = host[F_OVERFLOW] != 0;
        int lo = 0, hi = host[F_ENTRIES];
        for (int it = 0; it < grow_steps && !overflow && hi > lo; ++it) {
            const int count = hi - lo;
            if ((i64)count * 14 >= (i64(1) << 31) || (u64)(hi + (i64)count * 14) > (u64)lcap) {
                overflow = true;  // worst case of this iteration does not fit: larger table
                break;
            }
            u64* cand = arena_alloc<u64>(arena, (size_t)count * 7);
            if (!cand) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
            k_grow_candidates<<<grid_for((i64)count * 7, BLK), BLK, 0, ctx->stream>>>(t, list, lo, count, cand);
            ASR_CHECK_LAUNCH(ctx);
            k_grow_insert<<<grid_for((i64)count * 14, BLK), BLK, 0, ctx->stream>>>(t, list, lo, count, cand, ctx->d_flags,
                                                                                  lcap);
            ASR_CHECK_LAUNCH(ctx);
            ASR_TRY(read_flags(ctx, host));
            overflow = host[F_OVERFLOW] != 0;
            lo = hi;
            hi = host[F_ENTRIES];
        }
        if (overflow) continue;
        *keys_out = list;
        *count_out = host[F_ENTRIES];
        return ASR_HIP_OK;
    }
    ASR_FAIL(ctx, ASR_HIP_ELOGIC, "octree grow: hash table overflow");
}

int asr_geom_octree_build(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts,
                          const float* radii, i64 n, float radius_scale, int max_depth, int grow_steps,
                          const u64* extra_keys, i64 num_extra, bool balance) {
    ASR_TRY(ensure_flags(ctx));
    if (max_depth > ASR_MAX_LEVEL) max_depth = ASR_MAX_LEVEL;
    if (max_depth < 0) ASR_FAIL(ctx, ASR_HIP_EINVAL, "max_depth must be >= 0");
    if (grow_steps < 0) ASR_FAIL(ctx, ASR_HIP_EINVAL, "grow_steps must be >= 0");
    // Octree::Grow (octree.cpp:266) works on the raw point keys, before ancestors and siblings exist: its result
    // replaces the points as the input of the closure below
    u64* grown = nullptr;
    i64 num_grown = 0;
    Arena grow_arena;
    grow_arena.min_slab = size_t(16) << 20;
    struct ArenaGuard {
        Arena& a;
        ~ArenaGuard() { a.release(); }
    } grow_guard{grow_arena};
    if (grow_steps > 0 && n > 0)
        ASR_TRY(grow_keys(ctx, grow_arena, frame, pts, radii, n, radius_scale, max_depth, grow_steps, &grown, &num_grown));
    // nodes of a scan are ~0.3 n; the table must stay at most half full (cap / 2 list entries), else retry 4x larger
    u64 cap = next_pow2((u64)std::max<i64>(i64(1) << 16, 2 * std::max(std::max(n, 4 * num_grown), num_extra)));
    HostFlags host;
    for (int attempt = 0; attempt < 7; ++attempt, cap <<= 2) {
        if (attempt) ++ctx->table_regrows;
        ctx->scratch.reset();
        HashTab t;
        ASR_TRY(make_table(ctx, ctx->scratch, cap, false, t));
        // the table is kept at most half full, so the node list never exceeds cap / 2 entries
        int lcap = (int)std::min<u64>(cap / 2, u64(1) << 30);
        u64* list = arena_alloc<u64>(ctx->scratch, (size_t)lcap + 8);
        uint8_t* flag = arena_alloc<uint8_t>(ctx->scratch, (size_t)lcap / 8 + 8);
        if (!list || !flag) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        ASR_TRY(fresh_flags(ctx));
        if (grown) {
            if (num_grown > 0)
                k_octree_insert_keys<<<grid_for(num_grown, BLK), BLK, 0, ctx->stream>>>(grown, num_grown, t, ctx->d_flags,
                                                                                       list, lcap);
            ASR_CHECK_LAUNCH(ctx);
        } else if (n > 0) {
            k_octree_insert_points<<<grid_for(n, BLK), BLK, 0, ctx->stream>>>(*frame, pts, radii, n, radius_scale, max_depth,
                                                                              t, ctx->d_flags, list, lcap);
            ASR_CHECK_LAUNCH(ctx);
        }
        if (num_extra > 0) {  // node keys of other builds (the local octrees of the other ranks): same closure
            k_check_keys<<<grid_for(num_extra, BLK), BLK, 0, ctx->stream>>>(extra_keys, num_extra, ctx->d_flags);
            ASR_CHECK_LAUNCH(ctx);
            k_octree_insert_keys<<<grid_for(num_extra, BLK), BLK, 0, ctx->stream>>>(extra_keys, num_extra, t, ctx->d_flags,
                                                                                   list, lcap);
            ASR_CHECK_LAUNCH(ctx);
        }
        k_list_key_bits<<<256, BLK, 0, ctx->stream>>>(list, lcap, ctx->d_flags);  // (balancing adds no longer keys)
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(read_flags(ctx, host));
        if (host[F_NONFINITE]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "octree: points / radii contain non-finite values");
        bool overflow = host[F_OVERFLOW] != 0 || (u64)host[F_ENTRIES] * 2 > cap;
        int lo = 0, hi = host[F_ENTRIES];
        while (balance && !overflow && hi > lo) {
            int ngroups = (hi - lo) / 8;
            k_balance_classify<<<grid_for(ngroups, BLK), BLK, 0, ctx->stream>>>(t, list, lo, ngroups, flag);
            ASR_CHECK_LAUNCH(ctx);
            k_balance_insert<<<grid_for((i64)ngroups * 6, BLK), BLK, 0, ctx->stream>>>(
                    t, list, lo, ngroups, flag, ctx->d_flags, lcap);
            ASR_CHECK_LAUNCH(ctx);
            ASR_TRY(read_flags(ctx, host));
            overflow = host[F_OVERFLOW] != 0 || (u64)host[F_ENTRIES] * 2 > cap;
            lo = hi;
            hi = host[F_ENTRIES];
        }
        if (overflow) continue;
        i64 num_nodes = (i64)host[F_ENTRIES] + (host[F_ROOT] ? 1 : 0);
        ctx->leaf_lmin = ctx->leaf_lmax = -1;
        if (num_nodes == 0) {
            ctx->num_nodes = ctx->num_leaves = 0;
            ctx->nodes = ctx->leaves = nullptr;
            return ASR_HIP_OK;
        }
        if (host[F_ROOT]) {  // the root closes the list
            const u64 one = 1;
            ASR_HIP_CHECK(ctx, hipMemcpyAsync(list + host[F_ENTRIES], &one, sizeof(u64), hipMemcpyHostToDevice,
                                              ctx->stream));
        }
        ctx->nodes = arena_alloc<u64>(ctx->persist, num_nodes);
        u64* leaves_tmp = arena_alloc<u64>(ctx->scratch, num_nodes);
        uint8_t* lflag = arena_alloc<uint8_t>(ctx->scratch, num_nodes);
        i64* d_num = arena_alloc<i64>(ctx->scratch, 1);
        if (!ctx->nodes || !leaves_tmp || !lflag || !d_num) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        // (every node key is a prefix of an inserted key or a sibling / face neighbour of one: never longer)
        ASR_TRY(sort_keys(ctx, ctx->scratch, list, ctx->nodes, num_nodes, host[F_KEY_BITS] > 0 && host[F_KEY_BITS] <= 64 ? host[F_KEY_BITS] : 64));
        k_leaf_flags<<<grid_for(num_nodes, BLK), BLK, 0, ctx->stream>>>(t, ctx->nodes, num_nodes, lflag);
        ASR_CHECK_LAUNCH(ctx);
        {
            size_t tb = 0;
            ASR_HIP_CHECK(ctx, rocprim::select(nullptr, tb, ctx->nodes, lflag, leaves_tmp, d_num, (size_t)num_nodes,
                                               ctx->stream));
            void* tmp = ctx->scratch.alloc(tb ? tb : 256);
            if (!tmp) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
            ASR_HIP_CHECK(ctx, rocprim::select(tmp, tb, ctx->nodes, lflag, leaves_tmp, d_num, (size_t)num_nodes,
                                               ctx->stream));
        }
        i64* d_tail = arena_alloc<i64>(ctx->scratch, 3);
        if (!d_tail) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        k_leaf_tail<<<1, 1, 0, ctx->stream>>>(leaves_tmp, d_num, d_tail);
        ASR_CHECK_LAUNCH(ctx);
        i64 tail[3] = {0, 0, 0};
        ASR_HIP_CHECK(ctx, hipMemcpyAsync(tail, d_tail, sizeof(tail), hipMemcpyDeviceToHost, ctx->stream));
        ASR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        const i64 num_leaves = tail[0];
        auto level_of = [](u64 k) { return k ? (63 - __builtin_clzll(k)) / 3 : 0; };
        ctx->leaf_lmin = level_of((u64)tail[1]);
        ctx->leaf_lmax = level_of((u64)tail[2]);
        ctx->leaves = arena_alloc<u64>(ctx->persist, num_leaves);
        if (!ctx->leaves) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        ASR_HIP_CHECK(ctx, hipMemcpyAsync(ctx->leaves, leaves_tmp, 8 * num_leaves, hipMemcpyDeviceToDevice, ctx->stream));
        ctx->num_nodes = num_nodes;
        ctx->num_leaves = num_leaves;
        return ASR_HIP_OK;
    }
    ASR_FAIL(ctx, ASR_HIP_ELOGIC, "octree hash table overflow after 6 growth attempts");
}

// Key maps of all jobs of `b` (one allocation and one memset for all tables, one launch), then `pass` -- the work that
// uses them, enqueued on ctx->stream -- and ONE read-back of the overflow flag.  A map that lost keys (see TabProbe:
// lattice-like key sets fill "their" positions of the 64-slot buckets early) is rebuilt four times the size and `pass`
// run again, so that every caller either sees all keys or fails; none drops neighbours silently.
// grow0 / grow_out: the enlargement to start with and the one that sufficed (the _fill call of a stand-alone operator starts
// where its _count call ended instead of overflowing its way up again).
template <class Pass>
static int nb_key_maps(asr_hip_context* ctx, NbBatch& b, Pass&& pass, int grow0 = 0, int* grow_out = nullptr) {
    ASR_TRY(ensure_flags(ctx));
    for (int grow = grow0;; grow += 2) {
        u64 caps[NB_MAX_JOBS], cap_sum = 0;
        for (int j = 0; j < b.n; ++j) {
            caps[j] = next_pow2((u64)std::max<i64>(1024, 2 * b.v[j])) << grow;
            cap_sum += caps[j];
        }
        u64* tkeys = arena_alloc<u64>(ctx->scratch, cap_sum);
        int32_t* tvals = arena_alloc<int32_t>(ctx->scratch, cap_sum);
        if (!tkeys || !tvals) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        u64 off = 0;
        for (int j = 0; j < b.n; ++j) {
            b.tab[j] = HashTab{tkeys + off, tvals + off, caps[j] - 1};
            off += caps[j];
        }
        ASR_HIP_CHECK(ctx, hipMemsetAsync(tkeys, 0, cap_sum * sizeof(u64), ctx->stream));
        ASR_TRY(fresh_flags(ctx));
        k_map_build_batch<<<grid_for(b.base[b.n], BLK), BLK, 0, ctx->stream>>>(b, ctx->d_flags);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(pass());
        HostFlags host;
        ASR_TRY(read_flags(ctx, host));
        if (!host[F_OVERFLOW]) {
            if (grow_out) *grow_out = grow;
            return ASR_HIP_OK;
        }
        if (grow >= 6) ASR_FAIL(ctx, ASR_HIP_ELOGIC, "voxel key map overflow");
        ++ctx->table_regrows;
    }
}

// the stand-alone operators: one grid, a batch of one job whose row splits and lists are the caller's
static NbBatch nb_one_grid(const u64* keys, i64 v) {
    NbBatch b;
    b.n = 1;
    b.base[0] = 0;
    b.base[1] = v + 1;
    b.v[0] = v;
    b.keys[0] = keys;
    b.rs[0] = nullptr;
    b.idx[0] = nullptr;
    b.kidx[0] = nullptr;
    b.owner[0] = nullptr;
    b.me[0] = 1;
    return b;
}

static int check_row_list(asr_hip_context* ctx, const int32_t* rows, i64 nrows, i64 v, int32_t* mark = nullptr) {
    ASR_TRY(ensure_flags(ctx));
    ASR_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_flags + F_BAD_KEY, 0, sizeof(int), ctx->stream));
    k_check_rows<<<grid_for(nrows, BLK), BLK, 0, ctx->stream>>>(rows, nrows, v, ctx->d_flags, mark);
    ASR_CHECK_LAUNCH(ctx);
    HostFlags host;
    ASR_TRY(read_flags(ctx, host));
    if (host[F_BAD_KEY]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "neighbour rows: the row list must be strictly ascending indices in [0, %lld)", (long long)v);
    return ASR_HIP_OK;
}

int asr_geom_grid_neighbors_count(asr_hip_context* ctx, const u64* keys, i64 v, const int32_t* rows, i64 nrows, i64* rs,
                                  i64* num_pairs) {
    *num_pairs = 0;
    if (v <= 0) {
        ASR_HIP_CHECK(ctx, hipMemsetAsync(rs, 0, sizeof(i64), ctx->stream));
        return ASR_HIP_OK;
    }
    ctx->nb_grow_keys = nullptr;  // (set again below only when this call succeeds)
    NbBatch b = nb_one_grid(keys, v);
    if (rows) {  // the row list becomes the batch's row filter: 1 at the listed rows
        int32_t* mark = arena_alloc<int32_t>(ctx->scratch, v);
        if (!mark) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        ASR_HIP_CHECK(ctx, hipMemsetAsync(mark, 0, v * sizeof(int32_t), ctx->stream));
        ASR_TRY(check_row_list(ctx, rows, nrows, v, mark));
        b.owner[0] = mark;
    }
    i64* counts = arena_alloc<i64>(ctx->scratch, v + 1);
    if (!counts) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_TRY(nb_key_maps(ctx, b, [&]() -> int {
        k_neighbors_count_batch<<<grid_for(v + 1, BLK), BLK, 0, ctx->stream>>>(b, counts, nullptr, nullptr, nullptr);
        ASR_CHECK_LAUNCH(ctx);
        return scan_counts(ctx, ctx->scratch, counts, rs, v + 1);
    }, 0, &ctx->nb_grow));
    ctx->nb_grow_keys = keys;
    ctx->nb_grow_v = v;
    return read_i64(ctx, rs + v, num_pairs);
}
// rows: checked only; the rows that are not listed have no entries in rs and are skipped
int asr_geom_grid_neighbors_fill(asr_hip_context* ctx, const u64* keys, i64 v, const int32_t* rows, i64 nrows,
                                 const i64* rs, int32_t* idx, uint8_t* kidx) {
    if (v <= 0) return ASR_HIP_OK;
    if (rows) ASR_TRY(check_row_list(ctx, rows, nrows, v));
    NbBatch b = nb_one_grid(keys, v);
    b.idx[0] = idx;
    b.kidx[0] = kidx;
    // (the same keys as the _count call before: the enlargement its key map needed; a larger table never loses a key.
    // The note serves one _fill call: forgotten here, so that no later call on other keys at a reused address matches it)
    const int grow0 = ctx->nb_grow_keys == keys && ctx->nb_grow_v == v ? ctx->nb_grow : 0;
    ctx->nb_grow_keys = nullptr;
    ASR_TRY(nb_key_maps(ctx, b, [] { return ASR_HIP_OK; }, grow0));
    k_neighbors_fill_batch<<<grid_for(v + 1, BLK), BLK, 0, ctx->stream>>>(b, rs, nullptr, nullptr, nullptr);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

int asr_geom_neighbors_build_batch(asr_hip_context* ctx, Arena& out_arena, asr_nb_job* jobs, int n) {
    if (n < 1 || n > NB_MAX_JOBS) ASR_FAIL(ctx, ASR_HIP_EINVAL, "neighbors_build_batch: 1..%d jobs", NB_MAX_JOBS);
    NbBatch b;
    b.n = n;
    i64 total = 0;
    for (int j = 0; j < n; ++j) {
        if (jobs[j].v <= 0 || !jobs[j].keys) ASR_FAIL(ctx, ASR_HIP_EINVAL, "neighbors_build_batch: empty grid");
        b.base[j] = total;
        b.v[j] = jobs[j].v;
        b.keys[j] = jobs[j].keys;
        total += jobs[j].v + 1;
        jobs[j].rs = arena_alloc<i64>(out_arena, jobs[j].v + 1);
        if (!jobs[j].rs) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        b.rs[j] = jobs[j].rs;
        b.idx[j] = nullptr;
        b.kidx[j] = nullptr;
        b.owner[j] = jobs[j].owner;
        b.me[j] = jobs[j].me;
    }
    b.base[n] = total;
    i64* scan = nullptr;
    u64* masks = nullptr;
    int32_t* st_idx = nullptr;
    uint8_t* st_slot = nullptr;
    i64 host_totals[NB_MAX_JOBS];
    ASR_TRY(nb_key_maps(ctx, b, [&]() -> int {
        i64* counts = arena_alloc<i64>(ctx->scratch, total + 1);
        scan = arena_alloc<i64>(ctx->scratch, total + 1);
        masks = arena_alloc<u64>(ctx->scratch, total);
        st_idx = arena_alloc<int32_t>(ctx->scratch, (size_t)total * NB_STAGE);
        st_slot = arena_alloc<uint8_t>(ctx->scratch, (size_t)total * NB_STAGE);
        i64* totals = arena_alloc<i64>(ctx->scratch, NB_MAX_JOBS);
        if (!counts || !scan || !masks || !st_idx || !st_slot || !totals)
            ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        ASR_HIP_CHECK(ctx, hipMemsetAsync(counts + total, 0, sizeof(i64), ctx->stream));
        k_neighbors_count_batch<<<grid_for(total, BLK), BLK, 0, ctx->stream>>>(b, counts, masks, st_idx, st_slot);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(scan_counts(ctx, ctx->scratch, counts, scan, total + 1));
        k_nb_totals<<<1, 64, 0, ctx->stream>>>(b, scan, totals);
        ASR_CHECK_LAUNCH(ctx);
        // arrives with the read-back of the overflow flag
        ASR_HIP_CHECK(ctx, hipMemcpyAsync(host_totals, totals, n * sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
        return ASR_HIP_OK;
    }));
    for (int j = 0; j < n; ++j) {
        jobs[j].p = host_totals[j];
        jobs[j].idx = arena_alloc<int32_t>(out_arena, jobs[j].p);
        jobs[j].kidx = arena_alloc<uint8_t>(out_arena, jobs[j].p);
        if (!jobs[j].idx || !jobs[j].kidx) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        b.idx[j] = jobs[j].idx;
        b.kidx[j] = jobs[j].kidx;
    }
    k_neighbors_fill_batch<<<grid_for(total, BLK), BLK, 0, ctx->stream>>>(b, scan, masks, st_idx, st_slot);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

// what every key type ends with: ids_s = the rows in (job, segment, mask) order, masks = slot mask per row.  Option row_lpt:
// the 128-row chunks of every segment longest first (k_rg_chunk_keys; a list of one chunk keeps its order); then each
// job's permutation is written.
static int rg_finish(asr_hip_context* ctx, const RowGroupBatch& b, i64 total, i64 seg, int job_bits, int seg_bits,
                     const int32_t* ids_s, const u64* masks) {
    const i64 nc = total / 128;
    int32_t* ckey = arena_alloc<int32_t>(ctx->scratch, nc);
    int32_t* ckey_s = arena_alloc<int32_t>(ctx->scratch, nc);
    int32_t* cid = arena_alloc<int32_t>(ctx->scratch, nc);
    int32_t* cid_s = arena_alloc<int32_t>(ctx->scratch, nc);
    if (!ckey || !ckey_s || !cid || !cid_s) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    const int lpt = ctx->opt.row_lpt != 0;
    if (lpt) {
        if (job_bits + seg_bits + 7 > 31) ASR_FAIL(ctx, ASR_HIP_EINVAL, "row_groups: too many segments");
        k_rg_chunk_keys<<<grid_for(nc * 64, BLK), BLK, 0, ctx->stream>>>(b, seg, ids_s, masks, ckey, cid, seg_bits);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY((sort_pairs<int32_t, int32_t>(ctx, ctx->scratch, ckey, ckey_s, cid, cid_s, nc, job_bits + seg_bits + 7)));
    }
    k_rg_apply<<<grid_for(total, BLK), BLK, 0, ctx->stream>>>(b, ids_s, cid_s, lpt);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}
// The tiling orders of up to RG_MAX_JOBS lists: pack, masks, keys, sort, finish.  `ranked` set: keys on the rank of the mask;
// *ranked = false on return: they cannot be used (more than RG_MAX_MASKS distinct masks, a full mask set, a key of more than
// 32 bits), nothing is written and the caller sorts on full masks.  `ranked` null: keys on the mask itself, in one sort if
// job + segment + mask fit 64 bits, else by mask and then, stably, by (job, segment) with the ranked kernel and no rank.
static int rg_run(asr_hip_context* ctx, const asr_row_group_job* jobs, int n, i64 seg, int shift, bool* ranked) {
    RowGroupBatch b;
    b.n = 0;
    i64 total = 0, segments = 1;
    int kbits = 1;  // slot masks only use bits below the kernel size
    for (int j = 0; j < n; ++j) {
        if (jobs[j].v <= 0) continue;
        b.base[b.n] = total;
        b.v[b.n] = jobs[j].v;
        b.kidx[b.n] = jobs[j].kidx;
        b.rs[b.n] = jobs[j].rs;
        b.out[b.n] = jobs[j].perm_out;
        total += (jobs[j].v + 127) / 128 * 128;
        segments = std::max(segments, (jobs[j].v + seg - 1) / seg);
        kbits = std::max(kbits, jobs[j].kbits >= 1 && jobs[j].kbits <= 56 ? jobs[j].kbits : 56);
        ++b.n;
    }
    b.base[b.n] = total;
    if (b.n == 0) return ASR_HIP_OK;
    if (total >= (i64(1) << 31)) ASR_FAIL(ctx, ASR_HIP_EINVAL, "row_groups: too many rows");
    const int job_bits = b.n > 1 ? bits_for(b.n) : 0, seg_bits = bits_for(segments + 1), mask_bits = kbits - shift;
    u64* masks = arena_alloc<u64>(ctx->scratch, total);
    int32_t* ids = arena_alloc<int32_t>(ctx->scratch, total);
    int32_t* ids_s = arena_alloc<int32_t>(ctx->scratch, total);
    if (!masks || !ids || !ids_s) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    HashTab t{};
    if (ranked) {
        ASR_TRY(ensure_flags(ctx));
        ASR_TRY(make_table(ctx, ctx->scratch, RG_MASK_TAB, true, t));
        ASR_TRY(fresh_flags(ctx));
    }
    k_rg_masks<<<grid_for(total, BLK), BLK, 0, ctx->stream>>>(b, masks, ranked ? nullptr : ids, shift, t, ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    int low_bits = 0;  // of a 32-bit key below (job, segment): the rank of the mask, or nothing
    if (ranked) {
        u64* mlist = arena_alloc<u64>(ctx->scratch, RG_MAX_MASKS);
        int32_t* mslot = arena_alloc<int32_t>(ctx->scratch, RG_MAX_MASKS);
        if (!mlist || !mslot) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        k_rg_mask_collect<<<grid_for((i64)t.mask + 1, BLK), BLK, 0, ctx->stream>>>(t, mlist, mslot, ctx->d_flags);
        ASR_CHECK_LAUNCH(ctx);
        k_rg_mask_ranks<<<RG_MAX_MASKS / 256, 256, 0, ctx->stream>>>(t, mlist, mslot, ctx->d_flags);
        ASR_CHECK_LAUNCH(ctx);
        HostFlags host;
        ASR_TRY(read_flags(ctx, host));
        low_bits = bits_for(std::max(host[F_MASKS], 2));
        if (host[F_OVERFLOW] || host[F_MASKS] > RG_MAX_MASKS || job_bits + seg_bits + low_bits > 32) {
            *ranked = false;
            return ASR_HIP_OK;
        }
    } else if (job_bits + seg_bits + mask_bits <= 64) {
        u64* keys = arena_alloc<u64>(ctx->scratch, total);
        u64* keys_s = arena_alloc<u64>(ctx->scratch, total);
        if (!keys || !keys_s) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        k_rg_keys<<<grid_for(total, BLK), BLK, 0, ctx->stream>>>(b, seg, masks, keys, seg_bits, mask_bits, shift);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY((sort_pairs<u64, int32_t>(ctx, ctx->scratch, keys, keys_s, ids, ids_s, total, job_bits + seg_bits + mask_bits)));
        return rg_finish(ctx, b, total, seg, job_bits, seg_bits, ids_s, masks);
    } else {  // by mask first (the masks are their own keys), which leaves (job, segment): at most 4 + 28 bits
        u64* masks_s = arena_alloc<u64>(ctx->scratch, total);
        int32_t* ids_m = arena_alloc<int32_t>(ctx->scratch, total);
        if (!masks_s || !ids_m) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        ASR_TRY((sort_pairs<u64, int32_t>(ctx, ctx->scratch, masks, masks_s, ids, ids_m, total, shift + mask_bits, shift)));
        ids = ids_m;
    }
    unsigned* keys = arena_alloc<unsigned>(ctx->scratch, total);
    unsigned* keys_s = arena_alloc<unsigned>(ctx->scratch, total);
    if (!keys || !keys_s) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    k_rg_keys_ranked<<<grid_for(total, BLK), BLK, 0, ctx->stream>>>(b, seg, masks, ranked ? nullptr : ids, t, keys, ids,
                                                                    seg_bits, low_bits, shift);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY((sort_pairs<unsigned, int32_t>(ctx, ctx->scratch, keys, keys_s, ids, ids_s, total, job_bits + seg_bits + low_bits)));
    return rg_finish(ctx, b, total, seg, job_bits, seg_bits, ids_s, masks);
}
// lists with fewer than 16 rows per segment make no tile; more lists than one batch holds run in groups (no hierarchy has them)
int asr_geom_row_groups_batch(asr_hip_context* ctx, const asr_row_group_job* jobs, int n, i64 seg, int mask_shift, bool ranked) {
    if (seg < 16) seg = 16;
    for (; n > 0; jobs += RG_MAX_JOBS, n -= RG_MAX_JOBS) {
        const int g = std::min(n, RG_MAX_JOBS);
        if (ranked) {  // all lists in one sort on (job, segment, rank of the mask) keys
            bool done = true;
            ASR_TRY(rg_run(ctx, jobs, g, seg, mask_shift, &done));
            if (done) continue;
        }
        // The radix sort of the keys is what this routine costs.  Lists with few slots (the 9-slot up / down lists: more than
        // half of all rows of a hierarchy) go through it with short keys, three digit passes instead of eight.
        std::vector<asr_row_group_job> small_jobs, wide_jobs;
        for (int j = 0; j < g; ++j) (jobs[j].kbits <= 10 ? small_jobs : wide_jobs).push_back(jobs[j]);
        ASR_TRY(rg_run(ctx, small_jobs.data(), (int)small_jobs.size(), seg, mask_shift, nullptr));
        ASR_TRY(rg_run(ctx, wide_jobs.data(), (int)wide_jobs.size(), seg, mask_shift, nullptr));
    }
    return ASR_HIP_OK;
}

// CombineSiblings in two steps (k_coarsen_flags above); the keys are sorted and unique, as those of every grid.
// Step 1: flags -> exclusive scan of the packed counts (kept | heads << 32; both below 2^31) -> one read-back of the
// totals.  *pre (v + 2 entries, scratch) feeds step 2, *v_out = coarse voxels.
static int coarsen_scan(asr_hip_context* ctx, const u64* keys, i64 v, u64** pre, i64* v_out) {
    u64* packed = arena_alloc<u64>(ctx->scratch, v + 1);
    *pre = arena_alloc<u64>(ctx->scratch, v + 2);
    if (!packed || !*pre) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    k_coarsen_flags<<<grid_for(v + 1, BLK), BLK, 0, ctx->stream>>>(keys, v, packed);
    ASR_CHECK_LAUNCH(ctx);
    size_t tb = 0;
    ASR_HIP_CHECK(ctx, rocprim::exclusive_scan(nullptr, tb, packed, *pre, u64(0), (size_t)(v + 1), rocprim::plus<u64>(),
                                               ctx->stream));
    void* tmp = ctx->scratch.alloc(tb ? tb : 256);
    if (!tmp) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, rocprim::exclusive_scan(tmp, tb, packed, *pre, u64(0), (size_t)(v + 1), rocprim::plus<u64>(),
                                               ctx->stream));
    u64 totals = 0;
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(&totals, *pre + v, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *v_out = (i64)(totals & 0xffffffffu) + (i64)(totals >> 32);
    return ASR_HIP_OK;
}
// Step 2: the coarse keys, the up lists and, when down_rs is given, the down lists.  src: scratch int32[vo], the fine
// index of every coarse voxel.
static int coarsen_lists(asr_hip_context* ctx, const u64* keys, i64 v, const u64* pre, i64 vo, int32_t* src,
                         u64* out_keys, int32_t* up_idx, uint8_t* up_kidx, i64* up_rs, int32_t* down_idx,
                         uint8_t* down_kidx, i64* down_rs) {
    k_coarsen_place<<<grid_for(v, BLK), BLK, 0, ctx->stream>>>(keys, v, pre, out_keys, src);
    ASR_CHECK_LAUNCH(ctx);
    k_coarsen_up<<<grid_for(vo, BLK), BLK, 0, ctx->stream>>>(keys, v, src, vo, up_idx, up_kidx);
    ASR_CHECK_LAUNCH(ctx);
    k_iota64<<<grid_for(v + 1, BLK), BLK, 0, ctx->stream>>>(up_rs, v + 1);
    ASR_CHECK_LAUNCH(ctx);
    if (!down_rs) return ASR_HIP_OK;
    i64* cnt = arena_alloc<i64>(ctx->scratch, vo + 1);
    if (!cnt) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    k_coarsen_down_count<<<grid_for(vo + 1, BLK), BLK, 0, ctx->stream>>>(keys, v, src, vo, cnt);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, cnt, down_rs, vo + 1));
    k_coarsen_down_fill<<<grid_for(vo, BLK), BLK, 0, ctx->stream>>>(keys, v, src, vo, down_rs, down_idx, down_kidx);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

int asr_geom_coarsen_count(asr_hip_context* ctx, const u64* keys, i64 v, i64* v_out) {
    *v_out = 0;
    if (v <= 0) return ASR_HIP_OK;
    u64* pre;
    return coarsen_scan(ctx, keys, v, &pre, v_out);
}
int asr_geom_coarsen_fill(asr_hip_context* ctx, const u64* keys, i64 v, u64* out_keys, i64 v_out,
                          int32_t* up_idx, uint8_t* up_kidx, i64* up_rs) {
    if (v <= 0) return ASR_HIP_OK;
    u64* pre;
    i64 vo;
    ASR_TRY(coarsen_scan(ctx, keys, v, &pre, &vo));
    if (vo != v_out) ASR_FAIL(ctx, ASR_HIP_EINVAL, "grid_coarsen_fill: v_out = %lld, the keys give %lld", (long long)v_out,
                              (long long)vo);
    // zeroed: keys that break the sorted-unique rule leave positions unplaced, and the up lists index with them
    int32_t* src = arena_alloc<int32_t>(ctx->scratch, vo);
    if (!src) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, hipMemsetAsync(src, 0, vo * sizeof(int32_t), ctx->stream));
    return coarsen_lists(ctx, keys, v, pre, vo, src, out_keys, up_idx, up_kidx, up_rs, nullptr, nullptr, nullptr);
}
// whole-path variant: the outputs allocated from `keep`
int asr_geom_coarsen_build(asr_hip_context* ctx, Arena& keep, const u64* keys, i64 v, u64** out_keys, i64* v_out,
                           int32_t** up_idx, uint8_t** up_kidx, i64** up_rs, int32_t** down_idx, uint8_t** down_kidx,
                           i64** down_rs) {
    *v_out = 0;
    if (v <= 0) return ASR_HIP_OK;
    u64* pre;
    ASR_TRY(coarsen_scan(ctx, keys, v, &pre, v_out));
    const i64 vo = *v_out;
    int32_t* src = arena_alloc<int32_t>(ctx->scratch, vo);
    *out_keys = arena_alloc<u64>(keep, vo);
    *up_idx = arena_alloc<int32_t>(keep, v);
    *up_kidx = arena_alloc<uint8_t>(keep, v);
    *up_rs = arena_alloc<i64>(keep, v + 1);
    *down_idx = arena_alloc<int32_t>(keep, v);
    *down_kidx = arena_alloc<uint8_t>(keep, v);
    *down_rs = arena_alloc<i64>(keep, vo + 1);
    if (!src || !*out_keys || !*up_idx || !*up_kidx || !*up_rs || !*down_idx || !*down_kidx || !*down_rs)
        ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    return coarsen_lists(ctx, keys, v, pre, vo, src, *out_keys, *up_idx, *up_kidx, *up_rs, *down_idx, *down_kidx,
                         *down_rs);
}

int asr_geom_voxel_info(asr_hip_context* ctx, const asr_octree_frame* frame, const u64* keys,
                        i64 v, float* centers, float* sizes) {
    if (v <= 0) return ASR_HIP_OK;
    k_voxel_info<<<grid_for(v, BLK), BLK, 0, ctx->stream>>>(*frame, keys, v, centers, sizes);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

// the point index of a search; the context's own (rstate) is what asr_geom_radius_count parks for asr_geom_radius_fill
struct RadiusState {
    asr_octree_frame frame;
    float4* sorted = nullptr;  // points in Morton order, w = original index
    int32_t* ids = nullptr;    // original index of the point at each Morton position
    int32_t* rank = nullptr;   // inverse of ids (only when the caller asked for it)
    const u64* codes = nullptr;  // sorted level-21 codes (scratch arena: valid until the next reset)
    u64* codes_w = nullptr;      // the same, writable, and the unsorted inputs of the sort (deepen_point_index)
    const u64* codes_u = nullptr;
    const int32_t* ids_u = nullptr;
    int32_t* ids_w = nullptr;
    int lhash = ASR_MAX_LEVEL;   // finest level in the hash table (finer ones: binary search in codes)
    CellIndex index() const { return {tab, start, end, codes, (int)n, lhash}; }
    HashTab tab;
    int32_t* start = nullptr;
    int32_t* end = nullptr;
    i64 n = 0, v = 0;
    u64* tmp = nullptr;        // [v][RADIUS_LIGHT] sorted keys of the light rows
    int32_t* heavy = nullptr;  // rows with more than RADIUS_LIGHT hits or RADIUS_GIANT candidates
    uint8_t* is_heavy = nullptr;
    i64 num_heavy = 0;
    int* hc_pref = nullptr;    // cell ranges of the heavy rows (k_radius_heavy_cells)
    int* hc_beg = nullptr;
    float* srad = nullptr;     // radii in Morton order (when the count call was given them)
    const float* radii_src = nullptr;
    int lsort = 0;             // the points are sorted on the code bits down to this level
    int cell_grow = 0;         // log2 of the extra capacity of the cell table (sticky, raised after an overflow)
    bool aligned = false;      // queries are voxel centres of `aq.keys`: half-size cells + margin pairs (heavy rows)
    bool aligned_main = false; // ... in the per-voxel kernel as well (option search_half = 2)
    AlignedQ aq = {nullptr, nullptr, nullptr, -1};
};
struct DualState {  // what asr_geom_dual_count parks for asr_geom_dual_fill
    HashTab tab;                   // node key -> leaf index, -1 for an inner node
    const i64* offsets = nullptr;  // exclusive scan of the cells per leaf (nl + 1)
    const u64* leaves = nullptr;   // the caller's leaf array
    i64 nl = 0;
};
struct GeomState {
    RadiusState radius;  // also the home of the sticky cell_grow
    DualState dual;
};
static GeomState& gstate(asr_hip_context* ctx) {
    if (!ctx->geom_state) ctx->geom_state = new GeomState();
    return *(GeomState*)ctx->geom_state;
}
static RadiusState& rstate(asr_hip_context* ctx) { return gstate(ctx).radius; }
void asr_geom_release(asr_hip_context* ctx) {
    delete (GeomState*)ctx->geom_state;
    ctx->geom_state = nullptr;
}

// points sorted by level-21 Morton code (sort_points) + hash map (cell, level) -> [start, end) for levels
// lmin..lmax (build_cell_table)
// `keep`: arena for the arrays that outlive the search (Morton-ordered points, ids, rank); the scratch
// arena when null.  `want_rank`: also build the original index -> Morton position table.  `radii`: gathered into
// Morton order as well.  `lsort`: the points are grouped by their level-lsort cell (order inside such a cell:
// input order); `keep_all`: the sorted codes go to `keep` too (asr_geom_presort: they outlive this call).
static int sort_points(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts, i64 n, int lsort,
                       RadiusState& st, Arena* keep, bool want_rank, const float* radii, bool keep_all = false) {
    st.frame = *frame;
    st.n = n;
    st.lsort = lsort;
    Arena& ka = keep ? *keep : ctx->scratch;
    u64* codes_u = arena_alloc<u64>(ctx->scratch, n + 1);
    u64* codes = arena_alloc<u64>(keep_all ? ka : ctx->scratch, n + 1);
    int32_t* ids_u = arena_alloc<int32_t>(ctx->scratch, n + 1);
    int32_t* ids = arena_alloc<int32_t>(ka, n + 1);
    st.sorted = arena_alloc<float4>(ka, n + 1);
    st.ids = ids;
    st.codes = codes;
    st.codes_w = codes;
    st.codes_u = codes_u;
    st.ids_u = ids_u;
    st.ids_w = ids;
    st.rank = want_rank ? arena_alloc<int32_t>(ka, n + 1) : nullptr;
    st.srad = radii ? arena_alloc<float>(keep_all ? ka : ctx->scratch, n + 1) : nullptr;
    st.radii_src = radii;
    if (!codes_u || !codes || !ids_u || !ids || !st.sorted || (want_rank && !st.rank) || (radii && !st.srad))
        ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    if (n > 0) {
        k_point_codes<<<grid_for(n, BLK), BLK, 0, ctx->stream>>>(*frame, pts, n, codes_u, ids_u, ctx->d_flags);
        ASR_CHECK_LAUNCH(ctx);
        // the cell tables only cover levels up to lsort: sort the top 3*lsort bits of the 63-bit code only
        ASR_TRY((sort_pairs<u64, int32_t>(ctx, ctx->scratch, codes_u, codes, ids_u, ids, n, 63,
                                          3 * (ASR_MAX_LEVEL - std::max(lsort, 1)))));
        k_gather_points<<<grid_for(n, BLK), BLK, 0, ctx->stream>>>(pts, ids, n, st.sorted, st.rank, radii, st.srad);
        ASR_CHECK_LAUNCH(ctx);
    }
    return ASR_HIP_OK;
}
static int build_cell_table(asr_hip_context* ctx, i64 n, int lmin, int lmax, RadiusState& st, bool hash_all,
                            Arena* where = nullptr);
static int build_point_index(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts,
                             i64 n, int lmin, int lmax, RadiusState& st, Arena* keep = nullptr,
                             bool want_rank = false, bool hash_all = true, const float* radii = nullptr) {
    ASR_TRY(fresh_flags(ctx));
    ASR_TRY(sort_points(ctx, frame, pts, n, lmax, st, keep, want_rank, radii));
    return build_cell_table(ctx, n, lmin, lmax, st, hash_all);
}
static int build_cell_table(asr_hip_context* ctx, i64 n, int lmin, int lmax, RadiusState& st, bool hash_all, Arena* where) {
    Arena& arena = where ? *where : ctx->scratch;
    HostFlags host;
    const u64* codes = st.codes;
    HashTab dummy{nullptr, nullptr, 0};
    int* level_cnt = ctx->d_flags + FLAG_LEVEL_CELLS;  // cells per level
    int host_lvl[ASR_MAX_LEVEL + 1] = {0};
    if (n > 0) {
        ASR_HIP_CHECK(ctx, hipMemsetAsync(level_cnt, 0, (ASR_MAX_LEVEL + 1) * sizeof(int), ctx->stream));
        k_cell_bounds<true><<<std::min<unsigned>(grid_for(n + 1, BLK), 4096u), BLK, 0, ctx->stream>>>(
                codes, n, lmin, lmax, dummy, nullptr, nullptr, ctx->d_flags, level_cnt);
        ASR_CHECK_LAUNCH(ctx);
        ASR_HIP_CHECK(ctx, hipMemcpyAsync(host_lvl, level_cnt, sizeof(host_lvl), hipMemcpyDeviceToHost, ctx->stream));
    }
    ASR_TRY(read_flags(ctx, host));
    if (host[F_NONFINITE]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "points contain non-finite values");
    // Levels whose cells hold fewer than two points on average stay out of the hash table (a cloud with very dense
    // spots has query levels at which every point is a cell: 10^7 insertions per level); they are served by binary
    // search (cell_range).  Option search_hash_level forces the finest hashed level (tests).
    int lhash = lmax;
    if (!hash_all) {
        lhash = lmin;
        while (lhash < lmax && (i64)host_lvl[lhash + 1] * 2 <= n) ++lhash;
        if (ctx->opt.search_hash_level >= 0) lhash = (int)std::min<i64>(lmax, std::max<i64>(lmin - 1, ctx->opt.search_hash_level));
    }
    st.lhash = lhash;
    i64 cells = 0;
    for (int l = lmin; l <= lhash; ++l) cells += host_lvl[l];
    // cell_grow: enlarged after an overflow (keys whose low bits are concentrated on few values -- points on a
    // lattice -- crowd a few positions of the buckets, see TabProbe)
    u64 cap = next_pow2((u64)std::max<i64>(1024, 2 * cells)) << st.cell_grow;
    ASR_TRY(make_table(ctx, arena, cap, false, st.tab));
    st.start = arena_alloc<int32_t>(arena, cap);
    st.end = arena_alloc<int32_t>(arena, cap);
    if (!st.start || !st.end) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    if (n > 0) {
        k_cell_bounds<false><<<grid_for(n + 1, BLK), BLK, 0, ctx->stream>>>(
                codes, n, lmin, lhash, st.tab, st.start, st.end, ctx->d_flags, nullptr);
        ASR_CHECK_LAUNCH(ctx);
    }
    return ASR_HIP_OK;
}
// build_point_index that returns only with a table that lost no key: one that overflowed (lattice-like clouds crowd a few
// buckets, see TabProbe) is built again four times the size, in the same scratch.  The growth starts at the context's and is
// kept there, so that the next index of any entry point starts where this one ended.  The flag is read before any kernel
// walks the table: one that lost keys misses neighbours.  `what`: the failure message.
static int build_point_index_grown(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts, i64 n, int lmin,
                                   int lmax, RadiusState& st, const char* what, Arena* keep = nullptr, bool want_rank = false,
                                   bool hash_all = true, const float* radii = nullptr) {
    st.cell_grow = rstate(ctx).cell_grow;
    HostFlags host;
    ArenaMark mark;
    arena_mark(ctx->scratch, mark);
    for (;;) {
        ASR_TRY(build_point_index(ctx, frame, pts, n, lmin, lmax, st, keep, want_rank, hash_all, radii));
        ASR_TRY(read_flags(ctx, host));
        if (!host[F_OVERFLOW]) return ASR_HIP_OK;
        if (st.cell_grow >= 6) ASR_FAIL(ctx, ASR_HIP_ELOGIC, "%s", what);
        st.cell_grow += 2;
        rstate(ctx).cell_grow = st.cell_grow;
        ++ctx->table_regrows;
        arena_rewind(ctx->scratch, mark);
    }
}

constexpr int PRESORT_LEVEL = 13;  // the least depth of the early sort (five 8-bit passes either way)
// finest level a point can be inserted on (point_key: level_from_scale of its radius, capped at max_depth) = an upper bound
// of the octree's finest leaf level, before the octree exists
__global__ __launch_bounds__(256) void k_finest_point_level(asr_octree_frame f, const float* __restrict__ radii, i64 n,
                                                            float radius_scale, int max_depth, int* __restrict__ out) {
    int m = 0;
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        int l = level_from_scale(f, radius_scale * radii[i]);
        l = l < max_depth ? l : max_depth;
        m = max(m, l);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(out, m);
}
// radius_scale > 0: the sort goes one level below the finest level a point can be inserted on (capped at the deepest), so that
// the aggregation search of a cloud with very dense spots (leaves finer than level 12: BASELINE's mixed-density config) finds
// its cells in THIS order too instead of sorting the points again after the octree (3 ms at 10 M points)
int asr_geom_presort(asr_hip_context* ctx, Arena& keep, const asr_octree_frame* frame, const float* pts,
                     const float* radii, i64 n, float radius_scale, int max_depth) {
    ASR_TRY(ensure_flags(ctx));
    AsrPointIndex& pi = ctx->pindex;
    pi.valid = false;
    if (n <= 0 || n >= (i64(1) << 31)) return ASR_HIP_OK;
    int lsort = PRESORT_LEVEL;
    if (radius_scale > 0.f && radii) {
        HostFlags host;
        ASR_TRY(fresh_flags(ctx));
        k_finest_point_level<<<std::min<unsigned>(grid_for(n, BLK), 2048u), BLK, 0, ctx->stream>>>(
                *frame, radii, n, radius_scale, std::min(max_depth, ASR_MAX_LEVEL), ctx->d_flags + F_POINT_LEVEL);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(read_flags(ctx, host));
        lsort = std::max(PRESORT_LEVEL, std::min(ASR_MAX_LEVEL, host[F_POINT_LEVEL] + 1));
    }
    RadiusState st;
    ASR_TRY(sort_points(ctx, frame, pts, n, lsort, st, &keep, true, radii, true));
    pi.pts = pts;
    pi.radii = radii;
    pi.n = n;
    pi.lsort = lsort;
    pi.sorted = st.sorted;
    pi.ids = st.ids;
    pi.rank = st.rank;
    pi.srad = st.srad;
    pi.codes = st.codes_w;
    pi.valid = true;
    return ASR_HIP_OK;
}

// The aggregation search's cell table needs nothing from the octree either, only the range of levels its leaves can
// have: [1, PRESORT_LEVEL] covers every octree whose leaves are not finer than the sort (a root-only octree or a deeper
// one makes asr_geom_radius_count build its own table).  Host round trips: call it from the search's own thread.
int asr_geom_precells(asr_hip_context* ctx, Arena& keep) {
    AsrPointIndex& pi = ctx->pindex;
    pi.tab_keys = nullptr;
    if (!pi.valid || pi.n <= 0) return ASR_HIP_OK;
    RadiusState st;
    st.codes = st.codes_w = pi.codes;
    st.n = pi.n;
    st.cell_grow = rstate(ctx).cell_grow;
    ASR_TRY(fresh_flags(ctx));
    ASR_TRY(build_cell_table(ctx, pi.n, 1, pi.lsort, st, false, &keep));
    HostFlags host;
    ASR_TRY(read_flags(ctx, host));
    if (host[F_OVERFLOW]) {  // overflow: the query builds (and grows) its own table
        ++ctx->table_regrows;
        return ASR_HIP_OK;
    }
    pi.tab_grow = st.cell_grow;
    pi.tab_keys = st.tab.keys;
    pi.tab_mask = st.tab.mask;
    pi.tab_start = st.start;
    pi.tab_end = st.end;
    pi.tab_lmin = 1;
    pi.tab_lmax = pi.lsort;
    pi.tab_lhash = st.lhash;
    return ASR_HIP_OK;
}

// widen > 0: the range from the finest level a row starts on to the coarsest it reaches with its size times `widen`, over
// the rows that search at all (k_attr_levels); *lmin > *lmax when there is none
static int query_level_range(asr_hip_context* ctx, const asr_octree_frame* frame, const float* sizes,
                             i64 v, int* lmin, int* lmax, float widen = 0.f) {
    HostFlags host;
    ASR_TRY(fresh_flags(ctx));
    const int init[2] = {ASR_MAX_LEVEL, 0};  // F_LEVEL_MIN, F_LEVEL_MAX
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(ctx->d_flags + F_LEVEL_MIN, init, 2 * sizeof(int),
                                      hipMemcpyHostToDevice, ctx->stream));
    const unsigned grid = std::min<unsigned>(grid_for(v, BLK), 2048u);
    if (widen > 0.f)
        k_attr_levels<<<grid, BLK, 0, ctx->stream>>>(*frame, sizes, v, widen, ctx->d_flags);
    else
        k_query_levels<<<grid, BLK, 0, ctx->stream>>>(*frame, sizes, v, ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(read_flags(ctx, host));
    *lmin = host[F_LEVEL_MIN];
    *lmax = host[F_LEVEL_MAX];
    return ASR_HIP_OK;
}

int asr_geom_radius_count(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts,
                          i64 n, const float* centers, const float* sizes, i64 v, i64* rs,
                          i64* num_pairs, Arena* keep, const float* radii, const u64* voxel_keys, int lmin_hint,
                          int lmax_hint, const AsrPointIndex* pre) {
    pending_begin(ctx->pending);  // (the caller has recycled the scratch arena, or shares it with this search)
    ASR_TRY(ensure_flags(ctx));
    RadiusState& st = rstate(ctx);
    st.n = n, st.v = v;  // what the fill call must name again
    if (v <= 0) {
        *num_pairs = 0;
        if (rs) ASR_HIP_CHECK(ctx, hipMemsetAsync(rs, 0, sizeof(i64), ctx->stream));
        return count_done(ctx, PendingOp::MultiRadiusSearch);
    }
    if (n >= (i64(1) << 31)) ASR_FAIL(ctx, ASR_HIP_EINVAL, "too many points for int32 indices");
    HostFlags host;
    int lmin = lmin_hint, lmax = lmax_hint;
    if (lmin < 0 || lmax < lmin) ASR_TRY(query_level_range(ctx, frame, sizes, v, &lmin, &lmax));
    // aligned queries (voxel_keys): half-size cells of level L + 1 for the voxel levels L <= lhalf_max (see AlignedQ)
    // search_half 1 (default): half-size cells for the HEAVY rows only -- they walk 3.4x fewer candidates (0.90 -> 0.21 ms
    // at 10 M points) -- while the per-voxel kernel keeps the 27 full-size cells: its 64 look-ups with half-size cells
    // cost more (2.49 vs 1.23 ms) than the shorter candidate walk saves (0.45 vs 1.08 ms).  2: half-size cells everywhere.
    st.aligned = voxel_keys != nullptr && ctx->opt.search_half != 0;
    st.aligned_main = st.aligned && ctx->opt.search_half >= 2;
    ExtraParams ep;
    memset(&ep, 0, sizeof(ep));
    int lhalf_max = -1;
    if (st.aligned) {
        double M = 1;
        for (int d = 0; d < 3; ++d)
            M = std::max(M, std::max(std::fabs((double)frame->offset[d]), std::fabs((double)(1 << ASR_MAX_LEVEL) - frame->offset[d])));
        const int T = 2 + (int)std::floor(3.0 * (M + 1) / 16777216.0);
        lhalf_max = ASR_MAX_LEVEL - 1;
        while (lhalf_max >= 0 && (1 << (ASR_MAX_LEVEL - 1 - lhalf_max)) < 16 * T) --lhalf_max;
        ep.T = T;
        ep.lmin = lmin;
        ep.lmax = std::min(lmax, lhalf_max);
        for (int l = 0; l <= ASR_MAX_LEVEL; ++l)
            ep.rho[l] = (int)std::ceil(std::sqrt(2.0 * (double)(1 << (ASR_MAX_LEVEL - l)) * T)) + 2 * T + 1;
    }
    const int ltab = st.aligned ? std::min(ASR_MAX_LEVEL, std::min(lmax, lhalf_max) + 1) : lmax;
    if (pre && pre->valid && pre->pts == pts && pre->n == n && pre->lsort >= std::max(lmax, ltab) && (!radii || pre->srad)) {
        st.frame = *frame;  // the points are already in Morton order (asr_geom_presort)
        st.n = n;
        st.lsort = pre->lsort;
        st.sorted = pre->sorted;
        st.ids = pre->ids;
        st.rank = pre->rank;
        st.srad = radii ? pre->srad : nullptr;
        st.radii_src = radii;
        st.codes = st.codes_w = pre->codes;
        st.codes_u = nullptr;
        st.ids_u = nullptr;
        st.ids_w = pre->ids;
        ASR_TRY(fresh_flags(ctx));
        if (pre->tab_keys && pre->tab_grow == st.cell_grow && pre->tab_lmin <= lmin && pre->tab_lmax >= std::max(lmax, ltab)) {
            st.tab = HashTab{pre->tab_keys, nullptr, pre->tab_mask};  // built beside the octree (asr_geom_precells)
            st.start = pre->tab_start;
            st.end = pre->tab_end;
            st.lhash = pre->tab_lhash;
        } else {
            ASR_TRY(build_cell_table(ctx, n, lmin, std::max(lmax, ltab), st, false));
        }
    } else {
        ASR_TRY(build_point_index(ctx, frame, pts, n, lmin, std::max(lmax, ltab), st, keep, true, false, radii));
    }
    i64* counts = arena_alloc<i64>(ctx->scratch, v + 1);
    st.tmp = arena_alloc<u64>(ctx->scratch, (size_t)v * RADIUS_LIGHT);
    st.heavy = arena_alloc<int32_t>(ctx->scratch, v);
    st.is_heavy = arena_alloc<uint8_t>(ctx->scratch, v);
    int2* extras = arena_alloc<int2>(ctx->scratch, EXTRA_CAP);
    if (!counts || !st.tmp || !st.heavy || !st.is_heavy || !extras) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_flags + F_HEAVY, 0, sizeof(int), ctx->stream));
    ASR_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_flags + F_MARGIN_PAIRS, 0, sizeof(int), ctx->stream));
    st.aq = AlignedQ{voxel_keys, extras, ctx->d_flags + F_MARGIN_PAIRS, lhalf_max};
    // one pass: counts, the sorted light rows (fixed slots) and the list of heavy rows
    if (st.aligned && ep.lmax >= ep.lmin && n > 0) {
        k_radius_extras<<<grid_for(n, BLK), BLK, 0, ctx->stream>>>(st.codes, st.sorted, n, voxel_keys, v, centers, sizes,
                                                                  ep, extras, ctx->d_flags + F_MARGIN_PAIRS);
        ASR_CHECK_LAUNCH(ctx);
    }
    const unsigned qgrid = grid_for(v + 1, 4);
    if (st.aligned_main)
        k_radius_query<2, true><<<qgrid, BLK, 0, ctx->stream>>>(*frame, st.sorted, centers, sizes, v, st.index(), st.aq, counts,
                                                                st.tmp, st.heavy, ctx->d_flags + F_HEAVY, st.is_heavy);
    else
        k_radius_query<2, false><<<qgrid, BLK, 0, ctx->stream>>>(*frame, st.sorted, centers, sizes, v, st.index(), st.aq, counts,
                                                                 st.tmp, st.heavy, ctx->d_flags + F_HEAVY, st.is_heavy);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(read_flags(ctx, host));
    if (host[F_OVERFLOW]) {  // retry with a table four times the size
        if (st.cell_grow >= 6) ASR_FAIL(ctx, ASR_HIP_ELOGIC, "radius search cell table overflow");
        st.cell_grow += 2;
        ++ctx->table_regrows;
        return asr_geom_radius_count(ctx, frame, pts, n, centers, sizes, v, rs, num_pairs, keep, radii, voxel_keys,
                                     lmin_hint, lmax_hint, pre);
    }
    if (host[F_MARGIN_PAIRS] > EXTRA_CAP) ASR_FAIL(ctx, ASR_HIP_ELOGIC, "radius search: %d pairs in the rounding margin (cap %d)", host[F_MARGIN_PAIRS], EXTRA_CAP);
    ctx->search_extras = host[F_MARGIN_PAIRS];
    st.num_heavy = host[F_HEAVY];
    if (st.num_heavy > 0) {
        st.hc_pref = arena_alloc<int>(ctx->scratch, (size_t)st.num_heavy * HC_LD);
        st.hc_beg = arena_alloc<int>(ctx->scratch, (size_t)st.num_heavy * HC_LD);
        if (!st.hc_pref || !st.hc_beg) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        const unsigned cgrid = grid_for(st.num_heavy, 4);
        if (st.aligned) {
            k_radius_heavy_cells<true><<<cgrid, BLK, 0, ctx->stream>>>(*frame, centers, sizes, st.heavy, (int)st.num_heavy,
                                                                       st.index(), st.aq, st.hc_pref, st.hc_beg);
            k_radius_heavy<false, true><<<dim3((unsigned)st.num_heavy, RADIUS_SPLIT), BLK, 0, ctx->stream>>>(
                    *frame, st.sorted, centers, sizes, st.heavy, st.index(), st.aq, counts, nullptr, nullptr, nullptr, nullptr,
                    st.hc_pref, st.hc_beg, 0);
        } else {
            k_radius_heavy_cells<false><<<cgrid, BLK, 0, ctx->stream>>>(*frame, centers, sizes, st.heavy, (int)st.num_heavy,
                                                                        st.index(), st.aq, st.hc_pref, st.hc_beg);
            k_radius_heavy<false, false><<<dim3((unsigned)st.num_heavy, RADIUS_SPLIT), BLK, 0, ctx->stream>>>(
                    *frame, st.sorted, centers, sizes, st.heavy, st.index(), st.aq, counts, nullptr, nullptr, nullptr, nullptr,
                    st.hc_pref, st.hc_beg, 0);
        }
        ASR_CHECK_LAUNCH(ctx);
    }
    ASR_TRY(scan_counts(ctx, ctx->scratch, counts, rs, v + 1));
    ASR_TRY(read_i64(ctx, rs + v, num_pairs));
    return count_done(ctx, PendingOp::MultiRadiusSearch);
}

// KDTree::ComputeRadiusNeighbors (cpp/lib/nsearch.cpp:88-105): per point the number of points with
// squared distance < radius_i^2 (the point itself included)
int asr_geom_radius_neighbor_count(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts,
                                   const float* radii, i64 n, i64* counts_out) {
    ASR_TRY(ensure_flags(ctx));
    if (n <= 0) return ASR_HIP_OK;
    if (n >= (i64(1) << 31)) ASR_FAIL(ctx, ASR_HIP_EINVAL, "too many points for int32 indices");
    RadiusState st;
    int lmin, lmax;
    ASR_TRY(query_level_range(ctx, frame, radii, n, &lmin, &lmax));
    ASR_TRY(build_point_index_grown(ctx, frame, pts, n, lmin, lmax, st, "cell table overflow", nullptr, false, false));
    i64* counts = arena_alloc<i64>(ctx->scratch, n + 1);
    if (!counts) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    k_radius_query<0, false><<<grid_for(n + 1, 4), BLK, 0, ctx->stream>>>(
            *frame, st.sorted, pts, radii, n, st.index(), st.aq, counts, nullptr, nullptr, nullptr, nullptr);
    ASR_CHECK_LAUNCH(ctx);
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(counts_out, counts, n * sizeof(i64), hipMemcpyDeviceToDevice,
                                      ctx->stream));
    return ASR_HIP_OK;
}

// asr_hip_point_attributes_at: the search's point index (Morton-ordered points and radii, cell table for the levels the
// queries can reach), the attributes permuted into that order, then one fused search-and-blend launch.  Scratch: what the
// index takes plus 4 CP n bytes; nothing per pair.  The index build reads its cell counts back (build_cell_table), as the
// search's does; the blend itself is enqueued and not waited for.
int asr_geom_attributes_at(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts, const float* radii, i64 n,
                           const float* attr, int c, const float* positions, const float* sizes, i64 m, int max_widen,
                           float min_weight, float fill, float* out, float* weight_out, int8_t* widen_out) {
    ASR_TRY(ensure_flags(ctx));
    if (m <= 0) return ASR_HIP_OK;
    if (n >= (i64(1) << 31)) ASR_FAIL(ctx, ASR_HIP_EINVAL, "too many points for int32 indices");
    int lmin, lmax;
    ASR_TRY(query_level_range(ctx, frame, sizes, m, &lmin, &lmax, std::ldexp(1.f, max_widen)));
    if (lmin > lmax) lmin = lmax = 0;  // no searchable row at all
    const int cp = c <= 1 ? 1 : c <= 2 ? 2 : c <= 4 ? 4 : c <= 8 ? 8 : 16;
    RadiusState st;
    ASR_TRY(build_point_index_grown(ctx, frame, pts, n, lmin, lmax, st, "radius search cell table overflow", nullptr, false,
                                    false, radii));
    float* sattr = arena_alloc<float>(ctx->scratch, (size_t)(n + 1) * cp);
    if (!sattr) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
#define ASR_ATTR_BLEND(CP_)                                                                                                  \
    do {                                                                                                                     \
        if (n > 0) k_attr_permute<CP_><<<grid_for(n * CP_, BLK), BLK, 0, ctx->stream>>>(attr, st.ids, n, c, sattr);         \
        k_attr_blend<CP_><<<grid_for(m, 4), BLK, 0, ctx->stream>>>(*frame, st.sorted, st.srad, sattr, st.index(), positions, \
                                                                   sizes, m, c, max_widen, min_weight, fill, out,            \
                                                                   weight_out, widen_out);                                   \
    } while (0)
    switch (cp) {
        case 1: ASR_ATTR_BLEND(1); break;
        case 2: ASR_ATTR_BLEND(2); break;
        case 4: ASR_ATTR_BLEND(4); break;
        case 8: ASR_ATTR_BLEND(8); break;
        default: ASR_ATTR_BLEND(16); break;
    }
#undef ASR_ATTR_BLEND
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

// Re-sorts the points on the code bits down to level `ldeep` (they were sorted down to the table's finest level): the
// cell ranges of the table stay what they are (a stable sort on more bits only reorders points inside those cells), and
// cells of finer levels become contiguous, i.e. searchable (cell_range).
static int deepen_point_index(asr_hip_context* ctx, const float* pts, RadiusState& st, int ldeep) {
    ASR_TRY((sort_pairs<u64, int32_t>(ctx, ctx->scratch, st.codes_u, st.codes_w, st.ids_u, st.ids_w, st.n, 63,
                                      3 * (ASR_MAX_LEVEL - ldeep))));
    k_gather_points<<<grid_for(st.n, BLK), BLK, 0, ctx->stream>>>(pts, st.ids_w, st.n, st.sorted, st.rank);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}
// finest level of the kNN / nearest-point index: about one point per cell if the cloud filled the cube
static int knn_fine_level(i64 n) {
    int lfine = 1;
    while (lfine < ASR_MAX_LEVEL - 1 && (i64(1) << (3 * lfine)) < n) ++lfine;
    return lfine;
}
// Dense spots: a finest-level cell with thousands of points makes every one of them walk thousands of candidates.  Such
// clouds get their points sorted eight levels deeper (option knn_deep), and the points of crowded cells start on a finer
// level.  *ldeep = the level the points are sorted down to.  One read-back (the largest cell population).
static int deepen_crowded_index(asr_hip_context* ctx, const float* pts, RadiusState& st, int lfine, int* ldeep) {
    HostFlags host;
    *ldeep = lfine;
    ASR_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_flags + F_MAX_CELL_POP, 0, sizeof(int), ctx->stream));
    k_max_cell_pop<<<grid_for((i64)st.tab.mask + 1, BLK), BLK, 0, ctx->stream>>>(st.tab, st.start, st.end, lfine,
                                                                               ctx->d_flags + F_MAX_CELL_POP);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(read_flags(ctx, host));
    if (host[F_MAX_CELL_POP] > KNN_CROWD && ctx->opt.knn_deep) {
        *ldeep = std::min<int>(ASR_MAX_LEVEL, lfine + 8);
        ASR_TRY(deepen_point_index(ctx, pts, st, *ldeep));
    }
    return ASR_HIP_OK;
}
// The index of the nearest-neighbour searches: levels 0..lfine hashed, the points of a crowded cloud sorted down to ldeep.
// Host round trips: the cell counts of the build and the largest cell population.
struct KnnIndex {
    RadiusState st;
    int lfine = 0, ldeep = 0;
};
static int build_knn_index(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts, i64 n, int lfine,
                           const char* what, KnnIndex& ix) {
    ix.lfine = lfine;
    ASR_TRY(build_point_index_grown(ctx, frame, pts, n, 0, lfine, ix.st, what));
    ix.st.lhash = lfine;
    return deepen_crowded_index(ctx, pts, ix.st, lfine, &ix.ldeep);
}
// The queries' Morton order: alloc(), a kernel that fills codes_u / ids_u (k_query_codes, k_icp_codes), then sort() on the
// bits the index is hashed on; `ids` is the order.  Two steps so that a caller's own arrays keep their place in the arena.
struct QueryOrder {
    u64 *codes_u = nullptr, *codes = nullptr;
    int32_t *ids_u = nullptr, *ids = nullptr;
    bool alloc(asr_hip_context* ctx, i64 m) {
        codes_u = arena_alloc<u64>(ctx->scratch, m);
        codes = arena_alloc<u64>(ctx->scratch, m);
        ids_u = arena_alloc<int32_t>(ctx->scratch, m);
        ids = arena_alloc<int32_t>(ctx->scratch, m);
        return codes_u && codes && ids_u && ids;
    }
    int sort(asr_hip_context* ctx, i64 m, int lfine) {
        return sort_pairs<u64, int32_t>(ctx, ctx->scratch, codes_u, codes, ids_u, ids, m, 63, 3 * (ASR_MAX_LEVEL - lfine));
    }
};

// KDTree::ComputeKRadius / ComputeInlier (cpp/lib/nsearch.cpp:30-86)
int asr_geom_knn(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts, i64 n, int k,
                 const float* radii_in, float radius_fraction, int outlier_threshold, float* radii_out,
                 uint8_t* inlier_out) {
    ASR_TRY(ensure_flags(ctx));
    if (n <= 0) return ASR_HIP_OK;
    if (k < 1) ASR_FAIL(ctx, ASR_HIP_EINVAL, "knn: k must be >= 1");
    if (n >= (i64(1) << 31)) ASR_FAIL(ctx, ASR_HIP_EINVAL, "too many points for int32 indices");
    KnnIndex ix;
    HostFlags host;
    ASR_TRY(build_knn_index(ctx, frame, pts, n, knn_fine_level(n), "cell table overflow", ix));
    const RadiusState& st = ix.st;
    const int lfine = ix.lfine, ldeep = ix.ldeep;
    const bool fast = !inlier_out && radii_out && k <= 32 && n >= k && ctx->opt.knn_cells;
    if (fast) {
        // cell-parallel pass, then the wave-per-point kernel for what it could not certify
        int32_t* cells = arena_alloc<int32_t>(ctx->scratch, n + 1);
        int32_t* fallback = arena_alloc<int32_t>(ctx->scratch, n + 1);
        if (!cells || !fallback) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        ASR_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_flags + F_KNN_CELLS, 0, 2 * sizeof(int), ctx->stream));  // + F_KNN_FALLBACK
        k_cell_list<<<grid_for(n, 4096), BLK, 0, ctx->stream>>>(st.codes, n, lfine, cells, ctx->d_flags + F_KNN_CELLS);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(read_flags(ctx, host));
        const i64 ncells = host[F_KNN_CELLS];
#define ASR_KNN_CELLS(K_)                                                                                           \
    k_knn_cells<K_><<<grid_for(ncells, 4), BLK, 0, ctx->stream>>>(*frame, st.sorted, n, st.tab, st.start, st.end, lfine, \
                                                                   k, cells, ncells, radii_out, fallback,            \
                                                                   ctx->d_flags + F_KNN_FALLBACK)
        if (k <= 8)
            ASR_KNN_CELLS(8);
        else if (k <= 16)
            ASR_KNN_CELLS(16);
        else if (k <= 24)
            ASR_KNN_CELLS(24);
        else
            ASR_KNN_CELLS(32);
#undef ASR_KNN_CELLS
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(read_flags(ctx, host));
        const i64 nfb = host[F_KNN_FALLBACK];
        if (nfb > 0) {
            k_knn<<<grid_for(nfb, 4), BLK, 0, ctx->stream>>>(*frame, st.sorted, n, st.index(), lfine, ldeep, k, radii_in,
                                                             radius_fraction, outlier_threshold, radii_out, nullptr,
                                                             fallback, nfb);
            ASR_CHECK_LAUNCH(ctx);
        }
    } else {
        k_knn<<<grid_for(n, 4), BLK, 0, ctx->stream>>>(*frame, st.sorted, n, st.index(), lfine, ldeep, k, radii_in,
                                                       radius_fraction, outlier_threshold, radii_out, inlier_out,
                                                       nullptr, 0);
        ASR_CHECK_LAUNCH(ctx);
    }
    return ASR_HIP_OK;
}

// asr_hip_nearest_point: the index, the queries' Morton order, one k_nearest launch.  The search itself is enqueued and not
// waited for.
int asr_geom_nearest(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts, i64 n, const float* queries,
                     i64 m, int32_t* index_out, float* sqdist_out) {
    ASR_TRY(ensure_flags(ctx));
    if (m <= 0 || (!index_out && !sqdist_out)) return ASR_HIP_OK;
    KnnIndex ix;
    ASR_TRY(build_knn_index(ctx, frame, pts, n, knn_fine_level(n), "nearest point: cell table overflow", ix));
    QueryOrder qo;
    if (!qo.alloc(ctx, m)) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    k_query_codes<<<grid_for(m, BLK), BLK, 0, ctx->stream>>>(*frame, queries, m, qo.codes_u, qo.ids_u);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(qo.sort(ctx, m, ix.lfine));
    k_nearest<<<grid_for(m, 4), BLK, 0, ctx->stream>>>(*frame, ix.st.sorted, ix.st.index(), ix.lfine, ix.ldeep, queries,
                                                       qo.ids, m, index_out, sqdist_out);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

// asr_hip_icp_step / asr_hip_register_points: asr_geom_nearest's index of the target, built once per call; per step the
// transformed queries and their Morton order, one k_icp_pairs launch, k_icp_fold and the read-back of the sums.
static_assert(offsetof(asr_icp_sums, atb) == 21 * 8 && offsetof(asr_icp_sums, sq_residual) == 27 * 8 &&
                      offsetof(asr_icp_sums, sq_distance) == 28 * 8 && offsetof(asr_icp_sums, pairs) == 29 * 8,
              "k_icp_fold writes the sums in the struct's order");
// one step on a built index; its temporaries are taken from the scratch arena and given back
static int icp_step_indexed(asr_hip_context* ctx, const asr_octree_frame* frame, const KnnIndex& ix, const float* target,
                            const float* normals, const float* source, i64 m, const double transform[12],
                            const double origin[3], float max_distance, asr_icp_sums* sums, int32_t* index_out) {
    memset(sums, 0, sizeof(*sums));
    sums->mode = normals ? 1 : 0;
    if (m <= 0) return ASR_HIP_OK;
    ArenaMark mark;
    arena_mark(ctx->scratch, mark);
    const i64 nb = (m + 4 * ICP_RUN - 1) / (4 * ICP_RUN);
    float* q = arena_alloc<float>(ctx->scratch, 3 * m);
    QueryOrder qo;
    const bool qo_ok = qo.alloc(ctx, m);
    double* partial = arena_alloc<double>(ctx->scratch, nb * ICP_STRIDE);
    double* dsums = arena_alloc<double>(ctx->scratch, ICP_STRIDE);
    if (!q || !qo_ok || !partial || !dsums) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    IcpTransform x;
    memcpy(x.t, transform, sizeof(x.t));
    memcpy(x.o, origin, sizeof(x.o));
    k_icp_codes<<<grid_for(m, BLK), BLK, 0, ctx->stream>>>(*frame, x, source, m, q, qo.codes_u, qo.ids_u);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(qo.sort(ctx, m, ix.lfine));
    const float cap2 = max_distance * max_distance;
    if (normals)
        k_icp_pairs<true><<<(unsigned)nb, BLK, 0, ctx->stream>>>(*frame, ix.st.sorted, ix.st.index(), ix.lfine, ix.ldeep, q,
                                                                 qo.ids, m, target, normals, x.o[0], x.o[1], x.o[2], cap2,
                                                                 index_out, partial);
    else
        k_icp_pairs<false><<<(unsigned)nb, BLK, 0, ctx->stream>>>(*frame, ix.st.sorted, ix.st.index(), ix.lfine, ix.ldeep, q,
                                                                  qo.ids, m, target, nullptr, x.o[0], x.o[1], x.o[2], cap2,
                                                                  index_out, partial);
    ASR_CHECK_LAUNCH(ctx);
    k_icp_fold<<<1, 32 * ICP_FOLD, 0, ctx->stream>>>(partial, nb, dsums);
    ASR_CHECK_LAUNCH(ctx);
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(sums, dsums, ICP_TERMS * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    arena_rewind(ctx->scratch, mark);
    return ASR_HIP_OK;
}
int asr_geom_icp_step(asr_hip_context* ctx, const asr_octree_frame* frame, const float* target, i64 n, const float* normals,
                      const float* source, i64 m, const double transform[12], const double origin[3], float max_distance,
                      asr_icp_sums* sums, int32_t* index_out) {
    ASR_TRY(ensure_flags(ctx));
    KnnIndex ix;
    if (m > 0) ASR_TRY(build_knn_index(ctx, frame, target, n, knn_fine_level(n), "icp: cell table overflow", ix));
    return icp_step_indexed(ctx, frame, ix, target, normals, source, m, transform, origin, max_distance, sums, index_out);
}
int asr_geom_register(asr_hip_context* ctx, const asr_octree_frame* frame, const float* target, i64 n, const float* normals,
                      const float* source, i64 m, const asr_icp_params* params, double transform[12],
                      asr_icp_report* report) {
    ASR_TRY(ensure_flags(ctx));
    KnnIndex ix;
    if (m > 0) ASR_TRY(build_knn_index(ctx, frame, target, n, knn_fine_level(n), "icp: cell table overflow", ix));
    double origin[3];
    for (int a = 0; a < 3; ++a)
        origin[a] = (double)((1 << (ASR_MAX_LEVEL - 1)) - frame->offset[a]) * (double)frame->voxel_size[ASR_MAX_LEVEL];
    memset(report, 0, sizeof(*report));
    for (int it = 1; it <= params->max_iterations; ++it) {
        asr_icp_sums sums;
        ASR_TRY(icp_step_indexed(ctx, frame, ix, target, normals, source, m, transform, origin, params->max_distance, &sums,
                                 nullptr));
        report->iterations = it;
        report->pairs = sums.pairs;
        report->rmse = sums.pairs > 0 ? std::sqrt(sums.sq_distance / (double)sums.pairs) : 0.0;
        report->fitness = m > 0 ? (double)sums.pairs / (double)m : 0.0;
        double xi[6];
        if (asr_hip_icp_update(&sums, origin, transform, xi) != 0) {
            report->degenerate = 1;
            break;
        }
        const double w = std::sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
        const double v = std::sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
        if (w <= params->rotation_tolerance && v <= params->translation_tolerance) {
            report->converged = 1;
            break;
        }
    }
    return ASR_HIP_OK;
}

// asr_hip_knn_index: the index, one level finer, and one k_knn_index launch.  The search itself is enqueued and not waited
// for.
int asr_geom_knn_index(asr_hip_context* ctx, const asr_octree_frame* frame, const float* pts, i64 n, int k,
                       int32_t* index_out, float* sqdist_out) {
    ASR_TRY(ensure_flags(ctx));
    // One level finer than the radius search's index: knn_fine_level is about one point per cell of a cloud that fills the
    // cube, a scanned SURFACE has dozens of points in its occupied cells there and a wave would walk a few hundred
    // candidates per point; one level down it is a quarter.  Where that block holds fewer than k points (a cloud that does
    // fill the cube) the walk moves up after the 27 look-ups.
    KnnIndex ix;
    ASR_TRY(build_knn_index(ctx, frame, pts, n, std::min(ASR_MAX_LEVEL, knn_fine_level(n) + 1),
                            "knn index: cell table overflow", ix));
    if (!index_out && !sqdist_out) return ASR_HIP_OK;  // (the points have been checked)
    k_knn_index<<<grid_for(n, 4), BLK, 0, ctx->stream>>>(*frame, ix.st.sorted, n, ix.st.index(), ix.lfine, ix.ldeep, k,
                                                         index_out, sqdist_out);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

int asr_geom_radius_fill(asr_hip_context* ctx, const float* pts, const float* radii, i64 n,
                         const float* centers, const float* sizes, i64 v, const i64* rs,
                         int32_t* idx, float* dist, float* compat, int32_t* spos, const float4** sorted_out) {
    RadiusState& st = rstate(ctx);
    (void)pts;
    if (sorted_out) *sorted_out = nullptr;
    if (!fill_begin(ctx, PendingOp::MultiRadiusSearch) || st.n != n || st.v != v)
        ASR_FAIL(ctx, ASR_HIP_EINVAL,
                 "asr_hip_multi_radius_search_fill must follow the matching _count call");
    if (v <= 0) return ASR_HIP_OK;
    if (sorted_out) *sorted_out = st.sorted;
    float* srad = st.srad;  // gathered with the points when the count call had the radii
    if (compat && !srad) {
        srad = arena_alloc<float>(ctx->scratch, n + 1);
        if (!srad) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        if (n > 0) {
            k_gather_radii<<<grid_for(n, BLK), BLK, 0, ctx->stream>>>(radii, st.ids, n, srad);
            ASR_CHECK_LAUNCH(ctx);
        }
    }
    // light rows: already sorted in their fixed slots, copy them to the CSR positions.  (Round 4: on a side stream beside the
    // heavy rows' fill / sort / unpack below -- measured, no gain: the build's two chains already fill the GPU, what one
    // kernel gains the ones beside it lose.)
    k_radius_place<<<grid_for(v * 16, BLK), BLK, 0, ctx->stream>>>(st.tmp, rs, st.is_heavy, v, sizes, st.ids, srad, idx,
                                                                   spos, dist, compat);
    ASR_CHECK_LAUNCH(ctx);
    const i64 nh = st.num_heavy;
    if (nh > 0) {
        // heavy rows (> RADIUS_LIGHT hits): gather keys per row, segmented sort by (squared distance,
        // index) -- distances are >= 0 so their float bits order like unsigned integers
        i64* hcnt = arena_alloc<i64>(ctx->scratch, nh + 1);
        i64* hoff = arena_alloc<i64>(ctx->scratch, nh + 1);
        if (!hcnt || !hoff) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        k_heavy_counts<<<grid_for(nh + 1, BLK), BLK, 0, ctx->stream>>>(st.heavy, nh, rs, hcnt);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(scan_counts(ctx, ctx->scratch, hcnt, hoff, nh + 1));
        i64 hp = 0;
        ASR_TRY(read_i64(ctx, hoff + nh, &hp));
        if (hp >= (i64(1) << 32)) ASR_FAIL(ctx, ASR_HIP_EINVAL, "too many aggregation pairs");
        // One key per hit when (row, 31 distance bits, index) fits 64 bits: a single keys-only radix sort over exactly those
        // bits orders all heavy rows by (squared distance, index) -- distances are >= 0, their float bits order like
        // unsigned integers.  Otherwise two stable sorts: by the (distance, index) key, then by the row (a segmented sort
        // spends 1.6 ms on the few 10^4-entry rows).
        const int row_bits = bits_for(nh + 1);
        int idx_bits = bits_for(std::max<i64>(n, 2));
        if (row_bits + 31 + idx_bits > 64) idx_bits = 0;
        u64* k_u = arena_alloc<u64>(ctx->scratch, hp);
        u64* k_s = arena_alloc<u64>(ctx->scratch, hp);
        int32_t* t_row = idx_bits ? nullptr : arena_alloc<int32_t>(ctx->scratch, hp);
        if (!k_u || !k_s || (!idx_bits && !t_row)) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        int* cursor = arena_alloc<int>(ctx->scratch, nh);
        if (!cursor) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        ASR_HIP_CHECK(ctx, hipMemsetAsync(cursor, 0, (size_t)nh * sizeof(int), ctx->stream));
        if (st.aligned)
            k_radius_heavy<true, true><<<dim3((unsigned)nh, RADIUS_SPLIT), BLK, 0, ctx->stream>>>(
                    st.frame, st.sorted, centers, sizes, st.heavy, st.index(), st.aq, nullptr, hoff, cursor, k_u, t_row,
                    st.hc_pref, st.hc_beg, idx_bits);
        else
            k_radius_heavy<true, false><<<dim3((unsigned)nh, RADIUS_SPLIT), BLK, 0, ctx->stream>>>(
                    st.frame, st.sorted, centers, sizes, st.heavy, st.index(), st.aq, nullptr, hoff, cursor, k_u, t_row,
                    st.hc_pref, st.hc_beg, idx_bits);
        ASR_CHECK_LAUNCH(ctx);
        if (idx_bits) {
            ASR_TRY(sort_keys(ctx, ctx->scratch, k_u, k_s, hp, row_bits + 31 + idx_bits));
        } else {
            int32_t* t_row_s = arena_alloc<int32_t>(ctx->scratch, hp);
            if (!t_row_s) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
            ASR_TRY((sort_pairs<u64, int32_t>(ctx, ctx->scratch, k_u, k_s, t_row, t_row_s, hp, 64)));
            ASR_TRY((sort_pairs<int32_t, u64>(ctx, ctx->scratch, t_row_s, t_row, k_s, k_u, hp, bits_for(nh + 1))));
            k_s = k_u;  // sorted keys; t_row holds the sorted rows
        }
        k_radius_unpack_heavy<<<grid_for(hp, BLK), BLK, 0, ctx->stream>>>(k_s, t_row, hp, st.heavy, hoff, rs, sizes,
                                                                        radii, st.rank, idx, spos, dist, compat, idx_bits);
        ASR_CHECK_LAUNCH(ctx);
    }
    return ASR_HIP_OK;
}

// Dual cells of the LAST octree build (ctx->nodes / ctx->leaves).  count: number of cells; fill:
// [D,8] leaf indices, leaf order x corner order.
int asr_geom_dual_count(asr_hip_context* ctx, const u64* nodes, i64 nn, const u64* leaves, i64 nl, i64* num_cells) {
    ASR_TRY(count_begin(ctx));
    *num_cells = 0;
    DualState& st = gstate(ctx).dual;
    st = DualState();
    st.leaves = leaves;
    st.nl = nl;
    if (nl <= 0) return count_done(ctx, PendingOp::DualCells);
    HashTab t;
    u64 cap = next_pow2((u64)std::max<i64>(1024, 2 * nn));
    ASR_TRY(make_table(ctx, ctx->scratch, cap, true, t));
    ASR_HIP_CHECK(ctx, hipMemsetAsync(t.vals, 0xFF, cap * sizeof(int32_t), ctx->stream));  // -1 = inner
    int32_t* keep = t.vals;
    t.vals = arena_alloc<int32_t>(ctx->scratch, cap);  // throw-away values for the node pass
    if (!t.vals) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    k_map_build<<<grid_for(nn, BLK), BLK, 0, ctx->stream>>>(nodes, nn, t, ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    t.vals = keep;
    k_map_build<<<grid_for(nl, BLK), BLK, 0, ctx->stream>>>(leaves, nl, t, ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    i64* counts = arena_alloc<i64>(ctx->scratch, nl + 1);
    i64* offsets = arena_alloc<i64>(ctx->scratch, nl + 1);
    if (!counts || !offsets) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    k_dual_count<<<grid_for(nl + 1, BLK), BLK, 0, ctx->stream>>>(leaves, nl, t, counts);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, counts, offsets, nl + 1));
    ASR_TRY(read_i64(ctx, offsets + nl, num_cells));
    st.tab = t;
    st.offsets = offsets;
    return count_done(ctx, PendingOp::DualCells);
}
int asr_geom_dual_fill(asr_hip_context* ctx, i64* out) {
    if (!fill_begin(ctx, PendingOp::DualCells))
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "dual_fill must follow the matching dual_count call");
    const DualState& st = gstate(ctx).dual;
    if (st.nl <= 0) return ASR_HIP_OK;
    HostFlags host;
    k_dual_fill<<<grid_for(st.nl, BLK), BLK, 0, ctx->stream>>>(st.leaves, st.nl, st.tab, st.offsets, out, ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(read_flags(ctx, host));
    // (F_OVERFLOW: the node map of the _count call lost a key -- the same block when nothing took fresh flags in between)
    if (host[F_DUAL_KEY] || host[F_OVERFLOW]) ASR_FAIL(ctx, ASR_HIP_ELOGIC, "invalid key after searching for node (cpp/lib/grid.cpp:435-440)");
    return ASR_HIP_OK;
}

int asr_geom_invert(asr_hip_context* ctx, i64 num_points, const int32_t* idx, const i64* rs,
                    i64 num_rows, const uint8_t* attr, int32_t* out_idx, i64* out_rs,
                    uint8_t* out_attr, i64 known_pairs) {
    i64 p = known_pairs;  // >= 0: the caller knows rs[num_rows] (no read-back)
    if (p < 0) {
        p = 0;
        if (num_rows > 0) ASR_TRY(read_i64(ctx, rs + num_rows, &p));
    }
    i64* counts = arena_alloc<i64>(ctx->scratch, num_points + 1);
    if (!counts) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, (num_points + 1) * sizeof(i64), ctx->stream));
    if (p > 0) {
        k_invert_hist<<<grid_for(p, BLK), BLK, 0, ctx->stream>>>(idx, p, counts, num_points);
        ASR_CHECK_LAUNCH(ctx);
    }
    ASR_TRY(scan_counts(ctx, ctx->scratch, counts, out_rs, num_points + 1));
    if (p > 0) {
        int32_t* src = arena_alloc<int32_t>(ctx->scratch, p);
        int32_t* src_s = arena_alloc<int32_t>(ctx->scratch, p);
        int32_t* key_s = arena_alloc<int32_t>(ctx->scratch, p);
        if (!src || !src_s || !key_s) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        k_iota32<<<grid_for(p, BLK), BLK, 0, ctx->stream>>>(src, p);
        ASR_CHECK_LAUNCH(ctx);
        // stable LSD radix sort by target row == "fill in query order" 
        ASR_TRY((sort_pairs<int32_t, int32_t>(ctx, ctx->scratch, idx, key_s, src, src_s, p,
                                              bits_for(num_points + 1))));
        k_invert_fill<<<grid_for(p, BLK), BLK, 0, ctx->stream>>>(src_s, p, rs, num_rows, attr,
                                                                out_idx, out_attr);
        ASR_CHECK_LAUNCH(ctx);
    }
    return ASR_HIP_OK;
}

// ==========================================================================================
// row-group plans for the plan-driven sparse conv (layout: asr_common.h, consumer: asr_conv16.hip)
// ==========================================================================================
namespace {
constexpr i64 PLAN_DUP_FLAG = i64(1) << 40;
__global__ void k_plan_masks(const uint8_t* __restrict__ kidx, const i64* __restrict__ rs,
                             const int32_t* __restrict__ perm, i64 num_out, int K, i64 groups_pad,
                             uint4* __restrict__ hdr, i64* __restrict__ counts) {
    const i64 row = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    unsigned long long m = 0;
    int dup = 0;  // a slot that occurs twice in a row: the plan holds ONE neighbour per (row, slot)
    if (row < num_out) {
        const i64 q = perm ? perm[row] : row;
        int n = 0;
        for (i64 p = rs[q], pe = rs[q + 1]; p < pe; ++p) {
            const int k = kidx[p];
            if (k < K) {
                m |= 1ull << k;
                ++n;
            }
        }
        dup = n != __popcll(m);
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        m |= __shfl_xor(m, o, 64);
        dup |= __shfl_xor(dup, o, 64);
    }
    const i64 grp = row >> 4;
    if ((threadIdx.x & 15) == 0 && grp < groups_pad) {
        hdr[grp] = make_uint4((unsigned)m, (unsigned)(m >> 32), 0u, 0u);
        counts[grp] = (i64)__popcll(m) + (dup ? PLAN_DUP_FLAG : 0);  // the host sees the flag in the block total
    }
}

__global__ void k_plan_fill(const int32_t* __restrict__ nidx, const uint8_t* __restrict__ kidx,
                            const i64* __restrict__ rs, const int32_t* __restrict__ perm, i64 num_out, int K,
                            i64 groups_pad, const i64* __restrict__ offs, uint4* __restrict__ hdr, int32_t* __restrict__ pool) {
    const i64 row = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    const i64 grp = row >> 4;
    if (grp >= groups_pad) return;
    const unsigned off = (unsigned)offs[grp];
    if ((row & 15) == 0) hdr[grp].z = off;
    if (row >= num_out) return;
    const uint2 h = *reinterpret_cast<const uint2*>(&hdr[grp]);
    const unsigned long long m = (unsigned long long)h.x | ((unsigned long long)h.y << 32);
    const i64 q = perm ? perm[row] : row;
    for (i64 p = rs[q], pe = rs[q + 1]; p < pe; ++p) {
        const int k = kidx[p];
        if (k >= K) continue;
        const int j = __popcll(m & ((1ull << k) - 1));
        pool[((i64)off + j) * 16 + (row & 15)] = nidx[p];
    }
}


}  // namespace

int asr_geom_conv_plan_count(asr_hip_context* ctx, Arena& keep, const int32_t* nidx, const uint8_t* kidx, const i64* rs,
                             const int32_t* perm, i64 num_out, int K, asr_conv_plan* plan) {
    *plan = asr_conv_plan();
    plan->nidx = nidx;
    plan->kidx = kidx;
    plan->rs = rs;
    plan->perm = perm;
    plan->num_out = num_out;
    plan->K = K;
    if (num_out <= 0) return ASR_HIP_OK;
    plan->groups = (num_out + 15) / 16;
    plan->groups_pad = (plan->groups + 15) / 16 * 16;  // whole 256-row tiles
    plan->hdr = (uint4*)keep.alloc(plan->groups_pad * sizeof(uint4));
    plan->offs = (i64*)keep.alloc((plan->groups_pad + 1) * sizeof(i64));
    i64* counts = (i64*)ctx->scratch.alloc((plan->groups_pad + 1) * sizeof(i64));
    if (!plan->hdr || !plan->offs || !counts) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, hipMemsetAsync(counts + plan->groups_pad, 0, sizeof(i64), ctx->stream));
    k_plan_masks<<<grid_for(plan->groups_pad * 16, BLK), BLK, 0, ctx->stream>>>(kidx, rs, perm, num_out, K,
                                                                              plan->groups_pad, plan->hdr, counts);
    ASR_CHECK_LAUNCH(ctx);
    return asr_prim::scan_counts(ctx, ctx->scratch, counts, plan->offs, plan->groups_pad + 1);
}

int asr_geom_conv_plan_fill(asr_hip_context* ctx, Arena& keep, asr_conv_plan* plan, i64 blocks) {
    if (plan->num_out <= 0) return ASR_HIP_OK;
    plan->blocks = blocks;
    plan->pool = (int32_t*)keep.alloc((size_t)(blocks > 0 ? blocks : 1) * 64);
    if (!plan->pool) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, hipMemsetAsync(plan->pool, 0xFF, (size_t)(blocks > 0 ? blocks : 1) * 64, ctx->stream));
    k_plan_fill<<<grid_for(plan->groups_pad * 16, BLK), BLK, 0, ctx->stream>>>(
            plan->nidx, plan->kidx, plan->rs, plan->perm, plan->num_out, plan->K, plan->groups_pad, plan->offs,
            plan->hdr, plan->pool);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

// All lists of a build in one pass: one slot-set kernel, one scan, one read-back, one fill over the concatenated
// row ranges.  The plans share one pool (their headers hold positions in it).
namespace {
constexpr int PLAN_MAX_JOBS = 16;
struct PlanBatch {
    int n;
    i64 base[PLAN_MAX_JOBS + 1];  // first (padded) row of each job, multiples of 256; base[n] = total
    i64 rows[PLAN_MAX_JOBS];
    int K[PLAN_MAX_JOBS];
    const int32_t* nidx[PLAN_MAX_JOBS];
    const uint8_t* kidx[PLAN_MAX_JOBS];
    const i64* rs[PLAN_MAX_JOBS];
    const int32_t* perm[PLAN_MAX_JOBS];
};
__global__ void k_plan_masks_batch(PlanBatch b, uint4* __restrict__ hdr, i64* __restrict__ counts) {
    const i64 grow = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (grow >= b.base[b.n]) return;
    const int j = job_of(b, grow);
    const i64 row = grow - b.base[j];
    unsigned long long m = 0;
    if (row < b.rows[j]) {
        const i64 q = b.perm[j] ? b.perm[j][row] : row;
        const uint8_t* kidx = b.kidx[j];
        for (i64 p = b.rs[j][q], pe = b.rs[j][q + 1]; p < pe; ++p) {
            const int k = kidx[p];
            if (k < b.K[j]) m |= 1ull << k;
        }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) m |= __shfl_xor(m, o, 64);
    if ((threadIdx.x & 15) == 0) {
        hdr[grow >> 4] = make_uint4((unsigned)m, (unsigned)(m >> 32), 0u, 0u);
        counts[grow >> 4] = (i64)__popcll(m);
    }
}
// Thread r of a 16-thread group owns column r (its row) of every 64-byte line of the group: it walks the group's slot set
// and its own row together (rows list their slots in ascending order, cpp/lib/grid.cpp:99-170,229-240) and writes the
// neighbour or -1, so the 16 threads complete one line per store instruction and no line needs an initialising memset.
__global__ void k_plan_fill_batch(PlanBatch b, const i64* __restrict__ offs, uint4* __restrict__ hdr,
                                  int32_t* __restrict__ pool) {
    const i64 grow = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    if (grow >= b.base[b.n]) return;
    const i64 grp = grow >> 4;
    const unsigned off = (unsigned)offs[grp];
    if ((grow & 15) == 0) hdr[grp].z = off;
    const int j = job_of(b, grow);
    const i64 row = grow - b.base[j];
    const uint2 h = *reinterpret_cast<const uint2*>(&hdr[grp]);
    unsigned long long m = (unsigned long long)h.x | ((unsigned long long)h.y << 32);
    i64 p = 0, pe = 0;
    const uint8_t* kidx = b.kidx[j];
    const int32_t* nidx = b.nidx[j];
    if (row < b.rows[j]) {
        const i64 q = b.perm[j] ? b.perm[j][row] : row;
        p = b.rs[j][q];
        pe = b.rs[j][q + 1];
    }
    int32_t* line = pool + (i64)off * 16 + (grow & 15);
    while (m) {
        const int k = __builtin_ctzll(m);
        m &= m - 1;
        while (p < pe && kidx[p] < k) ++p;
        int32_t v = -1;
        if (p < pe && kidx[p] == k) v = nidx[p++];
        *line = v;
        line += 16;
    }
}
}  // namespace

int asr_geom_conv_plan_batch(asr_hip_context* ctx, Arena& keep, asr_conv_plan* const* plans, int n) {
    if (n > PLAN_MAX_JOBS) ASR_FAIL(ctx, ASR_HIP_EINVAL, "conv_plan_batch: too many lists");
    PlanBatch b;
    memset(&b, 0, sizeof(b));
    b.n = 0;
    i64 total = 0;
    int which[PLAN_MAX_JOBS];
    for (int j = 0; j < n; ++j) {
        asr_conv_plan& pl = *plans[j];
        pl.hdr = nullptr;
        pl.pool = nullptr;
        pl.offs = nullptr;
        pl.groups = pl.groups_pad = pl.blocks = 0;
        if (pl.num_out <= 0) continue;
        pl.groups = (pl.num_out + 15) / 16;
        pl.groups_pad = (pl.groups + 15) / 16 * 16;
        which[b.n] = j;
        b.base[b.n] = total;
        b.rows[b.n] = pl.num_out;
        b.K[b.n] = pl.K;
        b.nidx[b.n] = pl.nidx;
        b.kidx[b.n] = pl.kidx;
        b.rs[b.n] = pl.rs;
        b.perm[b.n] = pl.perm;
        total += pl.groups_pad * 16;
        ++b.n;
    }
    b.base[b.n] = total;
    if (b.n == 0) return ASR_HIP_OK;
    const i64 groups = total / 16;
    uint4* hdr = (uint4*)keep.alloc(groups * sizeof(uint4));
    i64* offs = (i64*)keep.alloc((groups + 1) * sizeof(i64));
    i64* counts = (i64*)ctx->scratch.alloc((groups + 1) * sizeof(i64));
    if (!hdr || !offs || !counts) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    ASR_HIP_CHECK(ctx, hipMemsetAsync(counts + groups, 0, sizeof(i64), ctx->stream));
    k_plan_masks_batch<<<grid_for(total, BLK), BLK, 0, ctx->stream>>>(b, hdr, counts);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(asr_prim::scan_counts(ctx, ctx->scratch, counts, offs, groups + 1));
    i64 blocks = 0;
    ASR_TRY(asr_prim::read_i64(ctx, offs + groups, &blocks));
    int32_t* pool = (int32_t*)keep.alloc((size_t)(blocks > 0 ? blocks : 1) * 64);
    if (!pool) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    k_plan_fill_batch<<<grid_for(total, BLK), BLK, 0, ctx->stream>>>(b, offs, hdr, pool);
    ASR_CHECK_LAUNCH(ctx);
    for (int t = 0; t < b.n; ++t) {
        asr_conv_plan& pl = *plans[which[t]];
        pl.hdr = hdr + b.base[t] / 16;
        pl.offs = offs + b.base[t] / 16;
        pl.pool = pool;
        pl.blocks = blocks;
    }
    return ASR_HIP_OK;
}

int asr_geom_conv_plan_build(asr_hip_context* ctx, Arena& keep, const int32_t* nidx, const uint8_t* kidx, const i64* rs,
                             const int32_t* perm, i64 num_out, int K, asr_conv_plan* plan) {
    ASR_TRY(asr_geom_conv_plan_count(ctx, keep, nidx, kidx, rs, perm, num_out, K, plan));
    if (num_out <= 0) return ASR_HIP_OK;
    i64 blocks = 0;
    ASR_TRY(asr_prim::read_i64(ctx, plan->offs + plan->groups_pad, &blocks));
    if (blocks >= PLAN_DUP_FLAG)
        ASR_FAIL(ctx, ASR_HIP_EINVAL,
                 "sparse_conv plan: a row lists a kernel slot twice; the 16-bit kernels take one neighbour per (row, slot) "
                 "(use asr_hip_sparse_conv_f32 with algo = 1 for such lists)");
    return asr_geom_conv_plan_fill(ctx, keep, plan, blocks);
}
