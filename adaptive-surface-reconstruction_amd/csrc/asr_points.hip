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
// Below the merge: PCA normals over given neighbour lists and their orientation (k_point_normals, k_orient_*; contract:
// include/asr_hip.h).
// Compiled with -ffp-contract=off: the cell arithmetic, the side test and the orientation's dot products round like
// their numpy restatements.
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

// ------------------------------------------------------------------------------------------
// Point normals (asr_hip_point_normals): one thread per point, everything in f64 from the f32
// coordinates.  Two passes over the row: the mean of the m valid neighbours, then the six centred sums, both in slot order
// (the same bits on every run).  The symmetric 3 x 3 is diagonalised by cyclic Jacobi sweeps on named scalars (no indexed
// private arrays: nothing goes to scratch memory); a rotation whose off-diagonal element is exactly zero is not made, so
// a cloud in an axis plane keeps its exact zero eigenvalue and axis normal.
// ------------------------------------------------------------------------------------------
// one Jacobi rotation in the (p, q) plane; r is the third axis.  After Rutishauser (Numerical Recipes' jacobi).
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq, double& vxp, double& vxq,
                                  double& vyp, double& vyq, double& vzp, double& vzq, bool late) {
    if (apq == 0.0) return;
    const double g = 100.0 * fabs(apq);
    if (late && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
        apq = 0.0;
        return;
    }
    const double h = aqq - app;
    double t;
    if (fabs(h) + g == fabs(h)) {
        t = apq / h;
    } else {
        const double theta = 0.5 * h / apq;
        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
        if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    double a = arp, b = arq;
    arp = a - s * (b + a * tau);
    arq = b + s * (a - b * tau);
    a = vxp, b = vxq;
    vxp = a - s * (b + a * tau);
    vxq = b + s * (a - b * tau);
    a = vyp, b = vyq;
    vyp = a - s * (b + a * tau);
    vyq = b + s * (a - b * tau);
    a = vzp, b = vzq;
    vzp = a - s * (b + a * tau);
    vzq = b + s * (a - b * tau);
}
__global__ __launch_bounds__(BLK) void k_point_normals(const float* __restrict__ pts, i64 n, const int32_t* __restrict__ index,
                                                       int k, float* __restrict__ normals, float* __restrict__ eig,
                                                       uint8_t* __restrict__ ok_out, int* flags) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t* row = index + i * k;
    double mx = 0.0, my = 0.0, mz = 0.0;
    int m = 0;
    bool bad = false;
    for (int s = 0; s < k; ++s) {
        const i64 j = row[s];
        if (j == -1) continue;
        if (j < 0 || j >= n) {
            bad = true;
            continue;
        }
        mx += (double)pts[3 * j], my += (double)pts[3 * j + 1], mz += (double)pts[3 * j + 2];
        ++m;
    }
    if (bad) atomicOr(&flags[F_BAD_INDEX], 1);  // the call fails; what is written below is not handed out
    double axx = 0.0, ayy = 0.0, azz = 0.0, axy = 0.0, axz = 0.0, ayz = 0.0;
    if (m > 0) {
        mx /= m, my /= m, mz /= m;
        for (int s = 0; s < k; ++s) {
            const i64 j = row[s];
            if (j < 0 || j >= n) continue;
            const double dx = (double)pts[3 * j] - mx, dy = (double)pts[3 * j + 1] - my, dz = (double)pts[3 * j + 2] - mz;
            axx += dx * dx, ayy += dy * dy, azz += dz * dz;
            axy += dx * dy, axz += dx * dz, ayz += dy * dz;
        }
        axx /= m, ayy /= m, azz /= m, axy /= m, axz /= m, ayz /= m;
    }
    // columns of v: the eigenvectors of the diagonal entries axx, ayy, azz
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < 50; ++sweep) {
        if (axy == 0.0 && axz == 0.0 && ayz == 0.0) break;
        const bool late = sweep >= 4;
        jacobi_rot(axx, ayy, axy, axz, ayz, v00, v01, v10, v11, v20, v21, late);  // (0, 1), third axis 2
        jacobi_rot(axx, azz, axz, axy, ayz, v00, v02, v10, v12, v20, v22, late);  // (0, 2), third axis 1
        jacobi_rot(ayy, azz, ayz, axy, axz, v01, v02, v11, v12, v21, v22, late);  // (1, 2), third axis 0
    }
    // ascending eigenvalues; e0's vector is the normal
    double l0 = axx, l1 = ayy, l2 = azz, nx = v00, ny = v10, nz = v20;
    const bool first = l1 < l0;  // (selects on values: a choice of column by index would put v into scratch memory)
    nx = first ? v01 : nx, ny = first ? v11 : ny, nz = first ? v21 : nz;
    const double a0 = first ? l1 : l0, a1 = first ? l0 : l1;
    const bool second = l2 < a0;
    nx = second ? v02 : nx, ny = second ? v12 : ny, nz = second ? v22 : nz;
    l0 = second ? l2 : a0;
    const double b2 = second ? a0 : l2;
    l1 = b2 < a1 ? b2 : a1;
    l2 = b2 < a1 ? a1 : b2;
    l0 = fmax(l0, 0.0), l1 = fmax(l1, 0.0), l2 = fmax(l2, 0.0);  // a covariance has no negative eigenvalue
    const bool ok = m >= 3 && l1 > 1e-10 * l2;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    if (ok) {
        const double len = sqrt(nx * nx + ny * ny + nz * nz);
        fx = (float)(nx / len), fy = (float)(ny / len), fz = (float)(nz / len);
        // the component of largest magnitude is positive, ties go to the lowest axis
        const float ax = fabsf(fx), ay = fabsf(fy), az = fabsf(fz);
        const float lead = (ax >= ay && ax >= az) ? fx : (ay >= az ? fy : fz);
        if (lead < 0.f) fx = -fx, fy = -fy, fz = -fz;
    }
    normals[3 * i] = fx, normals[3 * i + 1] = fy, normals[3 * i + 2] = fz;
    if (eig) eig[3 * i] = (float)l0, eig[3 * i + 1] = (float)l1, eig[3 * i + 2] = (float)l2;
    if (ok_out) ok_out[i] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// Orientation (asr_hip_normals_orient).  Viewpoint mode is one pass.  Propagation mode: Boruvka rounds
// over a signed union-find.  Between rounds the forest is FLAT: parent[i] is the root of i and par[i] the parity of i
// against that root (1: i has to be flipped when the root is not).  A round
//   offer   every directed slot e = i k + s whose ends lie in different trees offers its key (weight bits << 32 | e) to
//           the roots of both ends, a 64-bit atomicMin per root;
//   hook    every root with an offer hooks along its winner to the root on the other side -- of a mutual pair (both roots
//           chose the same slot) the smaller root stays -- and writes (hook, hook parity) beside the flat forest, which
//           this kernel only reads;
//   chase   every old root follows the hooks (read only) to its new root and writes (new root, parity) to a third pair
//           of arrays;
//   apply   every point composes its flat entry with its old root's: in place, but on its own entry only.
// No kernel reads what another thread of the same launch writes, so the result does not depend on scheduling.  With
// distinct keys every root's lightest outgoing edge is an edge of THE minimum spanning forest and the hooks form no cycle
// longer than the mutual pairs.
// ------------------------------------------------------------------------------------------
__device__ inline bool zero3(const float* v, i64 i) { return v[3 * i] == 0.f && v[3 * i + 1] == 0.f && v[3 * i + 2] == 0.f; }
__device__ inline float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    float s = ax * bx;
    s = s + ay * by;
    s = s + az * bz;
    return s;
}
__global__ void k_orient_viewpoint(const float* __restrict__ pts, const float* nrm, i64 n, const float* __restrict__ view,
                                   int per_point, float* nrm_out, uint8_t* __restrict__ flips, int* counters) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
    const bool skip = nx == 0.f && ny == 0.f && nz == 0.f;
    const float* v = view + (per_point ? 3 * i : 0);
    const bool flip = !skip && dot3(nx, ny, nz, v[0] - pts[3 * i], v[1] - pts[3 * i + 1], v[2] - pts[3 * i + 2]) < 0.f;
    nrm_out[3 * i] = flip ? -nx : nx, nrm_out[3 * i + 1] = flip ? -ny : ny, nrm_out[3 * i + 2] = flip ? -nz : nz;
    if (flips) flips[i] = flip ? 1 : 0;
    wave_add(&counters[F_ORIENT_SKIPPED], skip);
    wave_add(&counters[F_ORIENT_FLIPPED], flip);
}
__global__ void k_orient_init(const float* __restrict__ nrm, i64 n, int32_t* parent, uint8_t* par, int* counters) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    parent[i] = (int32_t)i;
    par[i] = 0;
    wave_add(&counters[F_ORIENT_SKIPPED], zero3(nrm, i));
}
__global__ void k_orient_clear(u64* best, i64 n) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) best[i] = ~u64(0);
}
// the edge of slot e: false when the slot holds none.  j: the other end, dot: of the two normals.
__device__ inline bool orient_edge(const float* __restrict__ nrm, const int32_t* __restrict__ index, i64 n, int k, i64 e,
                                   i64& i, i64& j, float& dot, bool& bad) {
    i = e / k;
    j = index[e];
    bad = j < -1 || j >= n;
    if (j < 0 || j >= n || j == i) return false;
    if (zero3(nrm, i) || zero3(nrm, j)) return false;
    dot = dot3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2]);
    return true;
}
__global__ void k_orient_offer(const float* __restrict__ nrm, const int32_t* __restrict__ index, i64 n, int k,
                               const int32_t* __restrict__ parent, u64* best, int* flags) {
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * k) return;
    i64 i, j;
    float dot;
    bool bad;
    const bool edge = orient_edge(nrm, index, n, k, e, i, j, dot, bad);
    if (bad) atomicOr(&flags[F_BAD_INDEX], 1);
    if (!edge) return;
    const int32_t ri = parent[i], rj = parent[j];
    if (ri == rj) return;
    const float w = fmaxf(0.f, 1.f - fabsf(dot));
    const u64 key = ((u64)__float_as_uint(w) << 32) | (u64)e;
    atomicMin((unsigned long long*)&best[ri], (unsigned long long)key);
    atomicMin((unsigned long long*)&best[rj], (unsigned long long)key);
}
__global__ void k_orient_hook(const float* __restrict__ nrm, const int32_t* __restrict__ index, i64 n, int k,
                              const int32_t* __restrict__ parent, const uint8_t* __restrict__ par,
                              const u64* __restrict__ best, int32_t* __restrict__ hook, uint8_t* __restrict__ hook_par,
                              int* counters) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    if (parent[r] != (int32_t)r) return;  // hooks are read at roots only
    int32_t to = (int32_t)r;
    uint8_t p = 0;
    const u64 key = best[r];
    if (key != ~u64(0)) {
        const i64 e = (i64)(key & 0xffffffffull);
        i64 i, j;
        float dot;
        bool bad;
        orient_edge(nrm, index, n, k, e, i, j, dot, bad);  // (an edge: it was offered)
        const int32_t ri = parent[i], rj = parent[j];
        const int32_t other = ri == (int32_t)r ? rj : ri;
        if (!(best[other] == key && (int32_t)r < other)) {
            to = other;
            p = par[i] ^ par[j] ^ (dot < 0.f ? 1 : 0);
        }
    }
    hook[r] = to;
    hook_par[r] = p;
    wave_add(&counters[F_ORIENT_HOOKED], to != (int32_t)r);
}
__global__ void k_orient_chase(i64 n, const int32_t* __restrict__ parent, const int32_t* __restrict__ hook,
                               const uint8_t* __restrict__ hook_par, int32_t* __restrict__ root, uint8_t* __restrict__ root_par) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n || parent[r] != (int32_t)r) return;
    int32_t x = (int32_t)r;
    uint8_t p = 0;
    for (int32_t h = hook[x]; h != x; h = hook[x]) {
        p ^= hook_par[x];
        x = h;
    }
    root[r] = x;
    root_par[r] = p;
}
__global__ void k_orient_apply(i64 n, int32_t* parent, uint8_t* par, const int32_t* __restrict__ root,
                               const uint8_t* __restrict__ root_par) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t r0 = parent[i];
    parent[i] = root[r0];
    par[i] ^= root_par[r0];
}
// the member with the largest z (ties: the smallest index) per tree: one packed atomicMax of (orderable z bits, ~index)
__global__ void k_orient_top(const float* __restrict__ pts, const float* __restrict__ nrm, i64 n,
                             const int32_t* __restrict__ parent, u64* top, int* counters) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool skip = zero3(nrm, i);
    wave_add(&counters[F_ORIENT_TREES], !skip && parent[i] == (int32_t)i);
    if (skip) return;
    const u32 b = __float_as_uint(pts[3 * i + 2] + 0.f);  // (-0 + 0 = +0: equal z, equal bits)
    const u32 ord = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
    // An atomic only while this point can still raise its tree's maximum: a scan is a few trees, and 10^7 atomics on four
    // addresses cost 53 ms.  The maximum only grows, so a stale read costs an atomic that changes nothing, never a result.
    const u64 key = ((u64)ord << 32) | (u32)~(u32)i;
    u64* slot = &top[parent[i]];
    if (key > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax((unsigned long long*)slot, (unsigned long long)key);
}
// flips first (a point reads the normal of its tree's top point), the normals after them in a launch of their own, in
// which every point touches its own normal only: normals_out may be normals
__global__ void k_orient_flips(const float* __restrict__ nrm, i64 n, const int32_t* __restrict__ parent,
                               const uint8_t* __restrict__ par, const u64* __restrict__ top, uint8_t* __restrict__ flips,
                               int* counters) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
    bool flip = false;
    if (!(nx == 0.f && ny == 0.f && nz == 0.f)) {
        const i64 t = (i64)(u32)~(u32)(top[parent[i]] & 0xffffffffull);
        const float tz = par[t] ? -nrm[3 * t + 2] : nrm[3 * t + 2];  // the top point's normal as its root has it
        flip = (par[i] != 0) != (tz < 0.f);
    }
    flips[i] = flip ? 1 : 0;
    wave_add(&counters[F_ORIENT_FLIPPED], flip);
}
__global__ void k_orient_flip(const float* nrm, i64 n, const uint8_t* __restrict__ flips, float* nrm_out) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool flip = flips[i] != 0;
    const float nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
    nrm_out[3 * i] = flip ? -nx : nx, nrm_out[3 * i + 1] = flip ? -ny : ny, nrm_out[3 * i + 2] = flip ? -nz : nz;
}

}  // namespace

int asr_points_merge_count(asr_hip_context* ctx, const asr_octree_frame* frame, const float* points, i64 n,
                           const float* normals, const float* radii, const float* attributes, int c, const int8_t* levels,
                           int level, int split_sides, i64* num_clusters, asr_points_merge_report* report) {
    ASR_TRY(count_begin(ctx));
    AsrMergeState& st = ctx->merge;
    st = AsrMergeState();
    *num_clusters = 0;
    if (report) *report = asr_points_merge_report{0, 0, 0, 0};
    st.points = points, st.normals = normals, st.radii = radii, st.attributes = attributes, st.channels = c;
    st.n = n;
    if (n == 0) return count_done(ctx, PendingOp::PointsMerge);
    hipStream_t s = ctx->stream;
    int* flags = ctx->d_flags;
    SCRATCH_ALLOC(keys, u64, n);
    SCRATCH_ALLOC(ids, int32_t, n);
    SCRATCH_ALLOC(keys_s, u64, n);
    SCRATCH_ALLOC(ids_s, int32_t, n);
    SCRATCH_ALLOC(head, i64, n + 1);
    SCRATCH_ALLOC(off, i64, n + 1);
    SCRATCH_ALLOC(starts, i64, n + 1);
    SCRATCH_ALLOC(long_list, int32_t, n / (CUT + 1) + 1);
    k_merge_keys<<<grid_for(n, BLK), BLK, 0, s>>>(*frame, points, n, levels, level, keys, ids, flags);
    ASR_CHECK_LAUNCH(ctx);
    // the marker bit of a level-l key is bit 3 l
    ASR_TRY(sort_pairs(ctx, ctx->scratch, keys, keys_s, ids, ids_s, n, levels ? 64 : 3 * level + 1));
    k_merge_cell_heads<<<grid_for(n + 1, BLK), BLK, 0, s>>>(keys_s, n, head);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, head, off, n + 1));
    const int32_t* members = ids_s;
    if (split_sides) {
        SCRATCH_ALLOC(side, uint8_t, n);
        SCRATCH_ALLOC(side_p, uint8_t, n);
        SCRATCH_ALLOC(ids_p, int32_t, n);
        SCRATCH_ALLOC(zero, i64, n + 1);
        SCRATCH_ALLOC(zoff, i64, n + 1);
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
    *num_clusters = st.clusters;
    if (report)
        *report = asr_points_merge_report{st.clusters, (i64)host[F_MERGE_DROPPED], (i64)host[F_MERGE_LARGEST],
                                          (i64)host[F_MERGE_SPLIT]};
    return count_done(ctx, PendingOp::PointsMerge);
}

int asr_points_merge_fill(asr_hip_context* ctx, float* points_out, float* normals_out, float* radii_out,
                          float* attributes_out, int32_t* counts_out, int32_t* cluster_out) {
    AsrMergeState& st = ctx->merge;
    if (!fill_begin(ctx, PendingOp::PointsMerge))
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "points_merge_fill must follow the matching points_merge_count call");
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

// asr_hip_point_normals: one launch and one read-back (the index check)
int asr_points_normals(asr_hip_context* ctx, const float* points, i64 n, const int32_t* index, int k, float* normals_out,
                       float* eigenvalues_out, uint8_t* ok_out) {
    if (n == 0) return ASR_HIP_OK;
    ASR_TRY(fresh_flags(ctx));
    k_point_normals<<<grid_for(n, BLK), BLK, 0, ctx->stream>>>(points, n, index, k, normals_out, eigenvalues_out, ok_out,
                                                               ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    HostFlags host;
    ASR_TRY(read_flags(ctx, host));
    if (host[F_BAD_INDEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "point_normals: a neighbour index is neither -1 nor in [0, n)");
    return ASR_HIP_OK;
}

// asr_hip_normals_orient.  Viewpoint mode: one launch, one read-back (the counts).  Propagation mode: four launches and
// one read-back per Boruvka round, at most ceil(log2 n) + 1 rounds that hook (every one at least halves the number of
// trees that still have an outgoing edge) and one that finds nothing left.
int asr_points_orient(asr_hip_context* ctx, const float* points, const float* normals, i64 n, const int32_t* index, int k,
                      const float* viewpoints, i64 num_viewpoints, float* normals_out, uint8_t* flips_out, i64 report[4]) {
    report[0] = report[1] = report[2] = report[3] = 0;
    if (n == 0) return ASR_HIP_OK;
    ctx->scratch.reset();
    hipStream_t s = ctx->stream;
    ASR_TRY(fresh_flags(ctx));
    int* flags = ctx->d_flags;
    HostFlags host;
    if (num_viewpoints > 0) {
        k_orient_viewpoint<<<grid_for(n, BLK), BLK, 0, s>>>(points, normals, n, viewpoints, num_viewpoints == n,
                                                            normals_out, flips_out, flags);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(read_flags(ctx, host));
        report[1] = host[F_ORIENT_FLIPPED];
        report[2] = host[F_ORIENT_SKIPPED];
        return ASR_HIP_OK;
    }
    SCRATCH_ALLOC(parent, int32_t, n);
    SCRATCH_ALLOC(par, uint8_t, n);
    SCRATCH_ALLOC(hook, int32_t, n);
    SCRATCH_ALLOC(hook_par, uint8_t, n);
    SCRATCH_ALLOC(root, int32_t, n);
    SCRATCH_ALLOC(root_par, uint8_t, n);
    SCRATCH_ALLOC(best, u64, n);
    SCRATCH_ALLOC(flips_tmp, uint8_t, n);
    u64* top = best;  // the offers are over when the top points are looked for
    uint8_t* flips = flips_out ? flips_out : flips_tmp;
    k_orient_init<<<grid_for(n, BLK), BLK, 0, s>>>(normals, n, parent, par, flags);
    ASR_CHECK_LAUNCH(ctx);
    int max_rounds = 2;
    while ((i64(1) << (max_rounds - 2)) < n) ++max_rounds;  // ceil(log2 n) + 2: the last one hooks nothing
    int hooked = 0, rounds = 0;
    for (;;) {
        k_orient_clear<<<grid_for(n, BLK), BLK, 0, s>>>(best, n);
        ASR_CHECK_LAUNCH(ctx);
        k_orient_offer<<<grid_for(n * k, BLK), BLK, 0, s>>>(normals, index, n, k, parent, best, flags);
        ASR_CHECK_LAUNCH(ctx);
        if (rounds == 0) {  // no slot is followed before the lists have been checked
            ASR_TRY(read_flags(ctx, host));
            if (host[F_BAD_INDEX])
                ASR_FAIL(ctx, ASR_HIP_EINVAL, "normals_orient: a neighbour index is neither -1 nor in [0, n)");
        }
        k_orient_hook<<<grid_for(n, BLK), BLK, 0, s>>>(normals, index, n, k, parent, par, best, hook, hook_par, flags);
        ASR_CHECK_LAUNCH(ctx);
        k_orient_chase<<<grid_for(n, BLK), BLK, 0, s>>>(n, parent, hook, hook_par, root, root_par);
        ASR_CHECK_LAUNCH(ctx);
        k_orient_apply<<<grid_for(n, BLK), BLK, 0, s>>>(n, parent, par, root, root_par);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(read_flags(ctx, host));
        if (host[F_ORIENT_HOOKED] == hooked) break;
        hooked = host[F_ORIENT_HOOKED];
        if (++rounds >= max_rounds) ASR_FAIL(ctx, ASR_HIP_ELOGIC, "normals_orient: the forest did not settle in %d rounds", rounds);
    }
    ASR_HIP_CHECK(ctx, hipMemsetAsync(top, 0, (size_t)n * sizeof(u64), s));
    k_orient_top<<<grid_for(n, BLK), BLK, 0, s>>>(points, normals, n, parent, top, flags);
    ASR_CHECK_LAUNCH(ctx);
    k_orient_flips<<<grid_for(n, BLK), BLK, 0, s>>>(normals, n, parent, par, top, flips, flags);
    ASR_CHECK_LAUNCH(ctx);
    k_orient_flip<<<grid_for(n, BLK), BLK, 0, s>>>(normals, n, flips, normals_out);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(read_flags(ctx, host));
    report[0] = host[F_ORIENT_TREES];
    report[1] = host[F_ORIENT_FLIPPED];
    report[2] = host[F_ORIENT_SKIPPED];
    report[3] = rounds;
    return ASR_HIP_OK;
}
