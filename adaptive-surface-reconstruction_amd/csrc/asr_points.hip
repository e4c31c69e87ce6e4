// asr_points.hip -- point merge: one point per occupied octree cell (contract: include/asr_hip.h; not in
// the reference).
//   keys       one thread per point: key of its cell (k_simp_keys' arithmetic), 0 for a point that is dropped
//   sort       stable radix sort of (key, index): the members of a cell are one run in ascending input index, the
//              dropped points lie in front
//   sides      (split_sides) every position looks up the first member of its cell and takes its side bit; ONE exclusive
//              scan of the side-0 flags over the whole list and one scatter partition every cell stably into its side-0
//              and its side-1 members -- no further sort
//   heads      cluster heads + scan give the output index of every position and the first position of every cluster
//   reduce     clusters of at most ASR_MERGE_LONG_CLUSTER members: one thread each, a sequential f64 chain; longer ones:
//              one workgroup each with a fixed tree.  No atomics on floats: the same bits on every run.
//   map        a scatter writes the cluster of every input point
// Compiled with -ffp-contract=off: the cell arithmetic and the side test round like their numpy restatement.
#include <cmath>
#include <cstring>

#include "asr_common.h"
#include "asr_prim.h"

namespace {
using namespace asr_prim;

constexpr int BLK = 256;
constexpr int CUT = ASR_MERGE_LONG_CLUSTER;

// counter += number of lanes of the wave with pred (one atomic per wave)
__device__ inline void wave_add(int* counter, bool pred) {
    const unsigned long long m = __ballot(pred);
    if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(counter, __popcll(m));
}

__global__ void k_merge_keys(asr_octree_frame f, const float* pts, i64 n, const int8_t* levels, int level, u64* keys,
                             int32_t* ids, int* flags) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int l = levels ? (int)levels[i] : level;
    int x = 0, y = 0, z = 0;
    u64 key = 0;
    if (l < 0 || l > ASR_MAX_LEVEL) {
        atomicOr(&flags[F_BAD_LEVEL], 1);  // the call fails before anything reads the key
    } else if (frame_coord21_checked(f, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], x, y, z)) {
        const int s = ASR_MAX_LEVEL - l;
        key = asr_coord_key(x >> s, y >> s, z >> s, l);
    }
    keys[i] = key;
    ids[i] = (int32_t)i;
    wave_add(&flags[F_MERGE_DROPPED], key == 0);
}
// head[r] = 1 where a cell starts in the sorted list (r = 0..n; the dropped points, key 0, start none)
__global__ void k_merge_cell_heads(const u64* keys, i64 n, i64* head) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    head[r] = (r < n && keys[r] != 0 && (r == 0 || keys[r] != keys[r - 1])) ? 1 : 0;
}
// off: exclusive scan of the head flags; position r lies in run off[r + 1] - 1.  starts[c] = first position of run c,
// starts[number of runs] = n.  total (may be null) receives the number of runs.
__global__ void k_merge_starts(const i64* off, i64 n, i64* starts, int* total) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    if (r == n) {
        starts[off[n]] = n;
        if (total) *total = (int)off[n];
        return;
    }
    if (off[r + 1] != off[r]) starts[off[r]] = r;
}
// side bit of every position against the first member of its cell; zero[r] = 1 for the side-0 members
__global__ void k_merge_sides(const u64* keys, const int32_t* ids, i64 n, const i64* off, const i64* starts,
                              const float* nrm, uint8_t* side, i64* zero) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    if (r == n || keys[r] == 0) {
        if (r < n) side[r] = 0;
        zero[r] = 0;
        return;
    }
    const float* a = nrm + 3 * (i64)ids[r];
    const float* b = nrm + 3 * (i64)ids[starts[off[r + 1] - 1]];
    const float d = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    const bool s = d < 0.f;  // false for NaN
    side[r] = s ? 1 : 0;
    zero[r] = s ? 0 : 1;
}
// zoff: exclusive scan of zero.  The side-0 members of a cell keep their order at its front, the side-1 members follow.
__global__ void k_merge_partition(const u64* keys, const int32_t* ids, const uint8_t* side, i64 n, const i64* off,
                                  const i64* starts, const i64* zoff, int32_t* ids_out, uint8_t* side_out) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    i64 to = r;
    if (keys[r] != 0) {
        const i64 c = off[r + 1] - 1;
        const i64 h = starts[c], e = starts[c + 1];
        const i64 before = zoff[r] - zoff[h], zeros = zoff[e] - zoff[h];
        to = side[r] ? h + zeros + ((r - h) - before) : h + before;
    }
    ids_out[to] = ids[r];
    side_out[to] = side[r];
}
// a cluster starts where a cell starts and where the side changes inside a cell
__global__ void k_merge_cluster_heads(const u64* keys, const i64* cell_head, const uint8_t* side, i64 n, i64* head,
                                      int* flags) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    bool h = false, split = false;
    if (r < n && keys[r] != 0) {
        h = cell_head[r] != 0;
        split = !h && side[r] != side[r - 1];  // not a cell head: r - 1 lies in the same cell
    }
    head[r] = (h || split) ? 1 : 0;
    wave_add(&flags[F_MERGE_SPLIT], split);
}
// the largest cluster and the list of the long ones, from the last position of every cluster
__global__ void k_merge_stats(const u64* keys, const i64* off, const i64* starts, i64 n, int* flags, int32_t* long_list) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    int len = 0;
    // the last position of a cluster: the list ends behind it, or r + 1 is a head (off[r + 2] > off[r + 1])
    if (r < n && keys[r] != 0 && (r + 1 == n || off[r + 2] != off[r + 1])) {
        const i64 c = off[r + 1] - 1;
        len = (int)(r + 1 - starts[c]);
        if (len > CUT) long_list[atomicAdd(&flags[F_MERGE_LONG], 1)] = (int32_t)c;
    }
    int m = len;
    for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
    // One atomic per wave only while the wave can still raise the maximum: the counter settles after a few waves, and
    // 150 000 atomics on one address cost 1.7 ms at 10 M points.  A stale read only costs an atomic that changes nothing.
    if ((threadIdx.x & 63) == 0 &&
        m > __hip_atomic_load(&flags[F_MERGE_LARGEST], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(&flags[F_MERGE_LARGEST], m);
}

struct MergeIO {
    const float *pts, *nrm, *rad, *att;
    float *pts_out, *nrm_out, *rad_out, *att_out;
    int32_t* cnt_out;
    int c;
};

// the normal of a cluster from the f64 sum of its members' normals; `first`: the normal of its first member
__device__ inline void write_normal(float* out, double sx, double sy, double sz, const float* first) {
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    if (len > 0.0 && len <= 1.79769313486231570815e308) {  // not 0, inf or NaN
        out[0] = (float)(sx / len), out[1] = (float)(sy / len), out[2] = (float)(sz / len);
    } else {
        out[0] = first[0], out[1] = first[1], out[2] = first[2];
    }
}

// one thread per cluster of at most CUT members: sequential f64 sums in ascending input index
__global__ __launch_bounds__(BLK) void k_merge_reduce(MergeIO io, const int32_t* __restrict__ ids,
                                                      const i64* __restrict__ starts, i64 nc) {
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const i64 b = starts[c], e = starts[c + 1];
    const i64 len = e - b;
    if (len > CUT) return;  // k_merge_reduce_long writes this cluster
    if (io.cnt_out) io.cnt_out[c] = (int32_t)len;
    const i64 first = ids[b];
    if (len == 1) {  // the member's bits
        if (io.pts_out)
            for (int a = 0; a < 3; ++a) io.pts_out[3 * c + a] = io.pts[3 * first + a];
        if (io.nrm_out)
            for (int a = 0; a < 3; ++a) io.nrm_out[3 * c + a] = io.nrm[3 * first + a];
        if (io.rad_out) io.rad_out[c] = io.rad[first];
        if (io.att_out)
            for (int a = 0; a < io.c; ++a) io.att_out[c * io.c + a] = io.att[first * io.c + a];
        return;
    }
    const double d = (double)len;
    {  // position, normal and radius in one walk over the members: their gathers are in flight together
        double px = 0.0, py = 0.0, pz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0, rs = 0.0;
        for (i64 j = b; j < e; ++j) {
            const i64 i = ids[j];
            if (io.pts_out) px += (double)io.pts[3 * i], py += (double)io.pts[3 * i + 1], pz += (double)io.pts[3 * i + 2];
            if (io.nrm_out) nx += (double)io.nrm[3 * i], ny += (double)io.nrm[3 * i + 1], nz += (double)io.nrm[3 * i + 2];
            if (io.rad_out) rs += (double)io.rad[i];
        }
        if (io.pts_out)
            io.pts_out[3 * c] = (float)(px / d), io.pts_out[3 * c + 1] = (float)(py / d), io.pts_out[3 * c + 2] = (float)(pz / d);
        if (io.nrm_out) write_normal(io.nrm_out + 3 * c, nx, ny, nz, io.nrm + 3 * first);
        if (io.rad_out) io.rad_out[c] = (float)(rs / d);
    }
    if (io.att_out) {
        for (int c0 = 0; c0 < io.c; c0 += 4) {  // four channels per walk over the members: the sums stay in registers
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            for (i64 j = b; j < e; ++j) {
                const float* p = io.att + (i64)ids[j] * io.c + c0;
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    if (c0 + a < io.c) s[a] += (double)p[a];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (c0 + a < io.c) io.att_out[c * io.c + c0 + a] = (float)(s[a] / d);
        }
    }
}

// Sum over the block of one value per thread: the 64 lanes of a wave pairwise (xor 32 .. 1: every lane ends with the same
// bits), the four waves as (w0 + w1) + (w2 + w3).  Every thread gets the total.
__device__ inline double block_sum(double v, double* lds) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();  // the previous call's readers are done
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}
// one column of a long cluster: thread t adds the members t, t + BLK, ... in order
__device__ inline double column_sum(const float* src, int stride, const int32_t* ids, i64 b, i64 e, double* lds) {
    double s = 0.0;
    for (i64 j = b + threadIdx.x; j < e; j += BLK) s += (double)src[(i64)ids[j] * stride];
    return block_sum(s, lds);
}
// one workgroup per cluster of more than CUT members
__global__ __launch_bounds__(BLK) void k_merge_reduce_long(MergeIO io, const int32_t* __restrict__ ids,
                                                           const i64* __restrict__ starts,
                                                           const int32_t* __restrict__ long_list) {
    __shared__ double lds[BLK / 64];
    const i64 c = long_list[blockIdx.x];
    const i64 b = starts[c], e = starts[c + 1];
    const double d = (double)(e - b);
    const bool writer = threadIdx.x == 0;
    if (writer && io.cnt_out) io.cnt_out[c] = (int32_t)(e - b);
    if (io.pts_out) {
        for (int a = 0; a < 3; ++a) {
            const double s = column_sum(io.pts + a, 3, ids, b, e, lds);
            if (writer) io.pts_out[3 * c + a] = (float)(s / d);
        }
    }
    if (io.nrm_out) {
        const double sx = column_sum(io.nrm, 3, ids, b, e, lds);
        const double sy = column_sum(io.nrm + 1, 3, ids, b, e, lds);
        const double sz = column_sum(io.nrm + 2, 3, ids, b, e, lds);
        if (writer) write_normal(io.nrm_out + 3 * c, sx, sy, sz, io.nrm + 3 * (i64)ids[b]);
    }
    if (io.rad_out) {
        const double s = column_sum(io.rad, 1, ids, b, e, lds);
        if (writer) io.rad_out[c] = (float)(s / d);
    }
    if (io.att_out) {
        for (int a = 0; a < io.c; ++a) {
            const double s = column_sum(io.att + a, io.c, ids, b, e, lds);
            if (writer) io.att_out[c * io.c + a] = (float)(s / d);
        }
    }
}
__global__ void k_merge_map(const u64* keys, const int32_t* ids, const i64* off, i64 n, int32_t* map) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    map[ids[r]] = keys[r] == 0 ? -1 : (int32_t)(off[r + 1] - 1);
}

#define MERGE_ALLOC(var, T, count)                          \
    T* var = arena_alloc<T>(ctx->scratch, (size_t)(count)); \
    if (!var) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed")

}  // namespace

int asr_points_merge_count(asr_hip_context* ctx, const asr_octree_frame* frame, const float* points, i64 n,
                           const float* normals, const float* radii, const float* attributes, int c, const int8_t* levels,
                           int level, int split_sides, i64* num_clusters, asr_points_merge_report* report) {
    AsrMergeState& st = ctx->merge;
    st = AsrMergeState();
    *num_clusters = 0;
    if (report) *report = asr_points_merge_report{0, 0, 0, 0};
    st.points = points, st.normals = normals, st.radii = radii, st.attributes = attributes, st.channels = c;
    st.n = n;
    if (n == 0) {
        st.valid = true;
        return ASR_HIP_OK;
    }
    ctx->scratch.reset();
    hipStream_t s = ctx->stream;
    ASR_TRY(fresh_flags(ctx));
    int* flags = ctx->d_flags;
    MERGE_ALLOC(keys, u64, n);
    MERGE_ALLOC(ids, int32_t, n);
    MERGE_ALLOC(keys_s, u64, n);
    MERGE_ALLOC(ids_s, int32_t, n);
    MERGE_ALLOC(head, i64, n + 1);
    MERGE_ALLOC(off, i64, n + 1);
    MERGE_ALLOC(starts, i64, n + 1);
    MERGE_ALLOC(long_list, int32_t, n / (CUT + 1) + 1);
    k_merge_keys<<<grid_for(n, BLK), BLK, 0, s>>>(*frame, points, n, levels, level, keys, ids, flags);
    ASR_CHECK_LAUNCH(ctx);
    // the marker bit of a level-l key is bit 3 l
    ASR_TRY(sort_pairs(ctx, ctx->scratch, keys, keys_s, ids, ids_s, n, levels ? 64 : 3 * level + 1));
    k_merge_cell_heads<<<grid_for(n + 1, BLK), BLK, 0, s>>>(keys_s, n, head);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, head, off, n + 1));
    const int32_t* members = ids_s;
    if (split_sides) {
        MERGE_ALLOC(side, uint8_t, n);
        MERGE_ALLOC(side_p, uint8_t, n);
        MERGE_ALLOC(ids_p, int32_t, n);
        MERGE_ALLOC(zero, i64, n + 1);
        MERGE_ALLOC(zoff, i64, n + 1);
        k_merge_starts<<<grid_for(n + 1, BLK), BLK, 0, s>>>(off, n, starts, nullptr);  // of the cells
        ASR_CHECK_LAUNCH(ctx);
        k_merge_sides<<<grid_for(n + 1, BLK), BLK, 0, s>>>(keys_s, ids_s, n, off, starts, normals, side, zero);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(scan_counts(ctx, ctx->scratch, zero, zoff, n + 1));
        k_merge_partition<<<grid_for(n, BLK), BLK, 0, s>>>(keys_s, ids_s, side, n, off, starts, zoff, ids_p, side_p);
        ASR_CHECK_LAUNCH(ctx);
        i64* cluster_head = zero;  // free again
        k_merge_cluster_heads<<<grid_for(n + 1, BLK), BLK, 0, s>>>(keys_s, head, side_p, n, cluster_head, flags);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(scan_counts(ctx, ctx->scratch, cluster_head, off, n + 1));
        members = ids_p;
    }
    k_merge_starts<<<grid_for(n + 1, BLK), BLK, 0, s>>>(off, n, starts, flags + F_MERGE_CLUSTERS);
    ASR_CHECK_LAUNCH(ctx);
    k_merge_stats<<<grid_for(n, BLK), BLK, 0, s>>>(keys_s, off, starts, n, flags, long_list);
    ASR_CHECK_LAUNCH(ctx);
    HostFlags host;
    ASR_TRY(read_flags(ctx, host));
    if (host[F_BAD_LEVEL]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "points_merge: a point level is not in 0..%d", ASR_MAX_LEVEL);
    st.clusters = host[F_MERGE_CLUSTERS];
    st.num_long = host[F_MERGE_LONG];
    st.keys = keys_s, st.ids = members, st.offsets = off, st.starts = starts, st.long_list = long_list;
    st.valid = true;
    *num_clusters = st.clusters;
    if (report)
        *report = asr_points_merge_report{st.clusters, (i64)host[F_MERGE_DROPPED], (i64)host[F_MERGE_LARGEST],
                                          (i64)host[F_MERGE_SPLIT]};
    return ASR_HIP_OK;
}

int asr_points_merge_fill(asr_hip_context* ctx, float* points_out, float* normals_out, float* radii_out,
                          float* attributes_out, int32_t* counts_out, int32_t* cluster_out) {
    AsrMergeState& st = ctx->merge;
    if (!st.valid) ASR_FAIL(ctx, ASR_HIP_EINVAL, "points_merge_fill must follow the matching points_merge_count call");
    st.valid = false;
    if (st.n == 0) return ASR_HIP_OK;
    hipStream_t s = ctx->stream;
    // an output whose input was not given stays unwritten
    MergeIO io{st.points,  st.normals, st.radii, st.attributes, points_out, st.normals ? normals_out : nullptr,
               st.radii ? radii_out : nullptr, st.attributes ? attributes_out : nullptr, counts_out, st.channels};
    if (st.clusters > 0 && (io.pts_out || io.nrm_out || io.rad_out || io.att_out || io.cnt_out)) {
        k_merge_reduce<<<grid_for(st.clusters, BLK), BLK, 0, s>>>(io, st.ids, st.starts, st.clusters);
        ASR_CHECK_LAUNCH(ctx);
        if (st.num_long > 0) {
            k_merge_reduce_long<<<(unsigned)st.num_long, BLK, 0, s>>>(io, st.ids, st.starts, st.long_list);
            ASR_CHECK_LAUNCH(ctx);
        }
    }
    if (cluster_out) {
        k_merge_map<<<grid_for(st.n, BLK), BLK, 0, s>>>(st.keys, st.ids, st.offsets, st.n, cluster_out);
        ASR_CHECK_LAUNCH(ctx);
    }
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(s));
    return ASR_HIP_OK;
}
