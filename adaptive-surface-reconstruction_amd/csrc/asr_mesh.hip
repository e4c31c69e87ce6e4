// asr_mesh.hip -- dual contouring and component filter on the GPU ("next" rows D.2 / D.3); further down, not in the
// reference: mesh sampling, simplification and adjacency -- edge table, topology, smoothing (4.9).
//
// Replaces asr::CreateTriangleMesh (cpp/lib/contouring.cpp:29-460) and
// asr::RemoveConnectedComponents (cpp/lib/postprocess.cpp:27-201).  The reference walks the dual
// cells serially; its output order is a pure function of the inputs (vertices in dual order, fan
// centres appended in emission order, triangles in (dual, owned edge) order), so every stage here
// is a data-parallel map + exclusive scan that lands each item at the index the serial loop gives.
// Compiled with -ffp-contract=off: the crossing points are double sums that must round like the
// reference's.
#include <cmath>
#include <cstring>
#include <algorithm>

#include "asr_common.h"
#include "asr_prim.h"
#include "asr_uset.h"

namespace {
using namespace asr_prim;

constexpr int BLK = 256;

// contouring.cpp:53-79
__constant__ int c_cube_edges[12][2] = {{0, 1}, {1, 3}, {3, 2}, {2, 0}, {4, 5}, {5, 7},
                                        {7, 6}, {6, 4}, {0, 4}, {1, 5}, {3, 7}, {2, 6}};
__constant__ int c_cube_faces[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {1, 5, 7, 3},
                                       {2, 3, 7, 6}, {0, 2, 6, 4}, {0, 4, 5, 1}};
__constant__ int c_owned_edges[3][2] = {{0, 1}, {1, 3}, {1, 5}};  // edge subset {0,1,9}

// What each _count call parks for its _fill: the caller's inputs and arrays in the scratch arena.  Which of them is live
// is ctx->pending's business (asr_pending.h), never a field's.
struct ContourState {
    const float* values = nullptr;
    const i64* duals = nullptr;
    i64 num_active = 0, num_extra = 0, num_tri = 0;
    float thr = 0;
    int32_t* active = nullptr;  // vertex -> dual
    float* vtx = nullptr;       // [num_active,3]
    i64* adj_rs = nullptr;      // voxel -> active duals (vertex indices, ascending)
    int32_t* adj = nullptr;
    i64* tri_off = nullptr;  // per (vertex, owned edge)
    i64* extra_off = nullptr;
};
struct ComponentsState {
    const float* in_vtx = nullptr;
    const int32_t* in_tri = nullptr;
    i64 nv = 0, nt = 0, nv_out = 0, nt_out = 0;
    i64* v_off = nullptr;  // exclusive scan of the vertex keep flags (nv+1)
    i64* t_off = nullptr;  // same for triangles
};
struct SimplifyState {
    const int32_t* in_tri = nullptr;
    i64 nv = 0, nt = 0, nv_out = 0, nt_out = 0;
    i64 nc = 0;                        // clusters
    const int32_t* cluster = nullptr;  // vertex -> cluster
    const float* cpos = nullptr;       // [nc,3] position of every cluster
    i64* c_off = nullptr;              // exclusive scan of the clusters a surviving triangle references (nc+1)
    i64* t_off = nullptr;              // exclusive scan of the surviving triangles (nt+1)
};
struct EdgesState {
    i64 num_edges = 0;
    const u64* keys = nullptr;   // sorted side keys
    const i64* start = nullptr;  // first side of every edge (num_edges+1)
    const i64* count = nullptr;  // the number of edges, on the device
};
struct FillHolesState {  // nv_out - nv hubs, nt_out - nt new triangles
    const float* in_vtx = nullptr;
    const int32_t* in_tri = nullptr;
    i64 nv = 0, nt = 0, nv_out = 0, nt_out = 0;
    i64 rim_vertices = 0, num_long = 0;  // vertices on filled rims; filled rims longer than FILL_CUT
    const u64* keys = nullptr;           // (rim id << 32) | vertex of the vertices on filled rims, sorted
    const int* len = nullptr;            // per rim id: its number of boundary edges
    const int* succ = nullptr;           // tail -> head of the boundary edge that leaves a vertex
    const int* start = nullptr;          // per filled rim id: its first entry in keys
    const i64* hub_off = nullptr;        // exclusive scan over the rim ids: hubs (nv+1)
    const i64* tri_off = nullptr;        // the same for the new triangles
    const int32_t* hub_rims = nullptr;   // hub -> rim id
    const int32_t* long_rims = nullptr;  // the filled rims a whole wave sums
};
struct MeshState {
    ContourState contour;
    ComponentsState components;
    SimplifyState simplify;
    EdgesState edges;
    FillHolesState fill_holes;
};

__device__ inline bool crossing(const float* values, float thr, i64 a, i64 b) {  // :81-111
    const float2 va = ((const float2*)values)[a], vb = ((const float2*)values)[b];
    if (va.y > thr && vb.y > thr) return false;
    return (va.x < 0 && vb.x > 0) || (va.x > 0 && vb.x < 0);
}

// one thread per dual cell: active flag and number of distinct corner voxels.  A cell with a corner outside
// [0, nv) raises flags[F_BAD_INDEX] and counts as inactive: no later kernel loads through its indices.
__global__ void k_contour_active(const float* values, i64 nv, const i64* duals, i64 nd, float thr, i64* flag,
                                 i64* npairs, int* flags) {
    i64 d = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > nd) return;
    if (d == nd) {
        flag[d] = 0;
        npairs[d] = 0;
        return;
    }
    i64 c[8];
    bool in_range = true;
    for (int k = 0; k < 8; ++k) {
        c[k] = duals[d * 8 + k];
        in_range &= c[k] >= 0 && c[k] < nv;
    }
    if (!in_range) {
        atomicOr(&flags[F_BAD_INDEX], 1);
        flag[d] = 0;
        npairs[d] = 0;
        return;
    }
    bool act = false;
    for (int e = 0; e < 12; ++e) act |= crossing(values, thr, c[c_cube_edges[e][0]], c[c_cube_edges[e][1]]);
    int distinct = 0;
    for (int k = 0; k < 8; ++k) {
        bool first = true;
        for (int j = 0; j < k; ++j) first &= c[j] != c[k];
        distinct += first;
    }
    flag[d] = act ? 1 : 0;
    npairs[d] = act ? distinct : 0;
}

// vertex of an active dual (:114-142) + its (voxel, vertex) adjacency pairs
__global__ void k_contour_vertices(const float* values, const i64* duals, i64 nd, const float* pos, float thr,
                                   const i64* voff, const i64* poff, int32_t* active, float* vtx, u64* pairs) {
    i64 d = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= nd) return;
    const i64 vid = voff[d];
    if (voff[d + 1] == vid) return;
    active[vid] = (int32_t)d;
    i64 c[8];
    for (int k = 0; k < 8; ++k) c[k] = duals[d * 8 + k];
    double px = 0, py = 0, pz = 0;
    int count = 0;
    for (int e = 0; e < 12; ++e) {
        const i64 a = c[c_cube_edges[e][0]], b = c[c_cube_edges[e][1]];
        const float2 va = ((const float2*)values)[a], vb = ((const float2*)values)[b];
        if (va.y > thr && vb.y > thr) continue;
        const double v1 = va.x, v2 = vb.x;
        if ((v1 < 0 && v2 > 0) || (v1 > 0 && v2 < 0)) {
            double t = -v1 / (v2 - v1);
            if (!isfinite(t) || t < 0 || t > 1) t = 0.5;
            px += (1 - t) * (double)pos[a * 3 + 0] + t * (double)pos[b * 3 + 0];
            py += (1 - t) * (double)pos[a * 3 + 1] + t * (double)pos[b * 3 + 1];
            pz += (1 - t) * (double)pos[a * 3 + 2] + t * (double)pos[b * 3 + 2];
            ++count;
        }
    }
    vtx[vid * 3 + 0] = (float)(px / count);
    vtx[vid * 3 + 1] = (float)(py / count);
    vtx[vid * 3 + 2] = (float)(pz / count);
    i64 o = poff[d];
    for (int k = 0; k < 8; ++k) {
        bool first = true;
        for (int j = 0; j < k; ++j) first &= c[j] != c[k];
        if (first) pairs[o++] = ((u64)c[k] << 32) | (u64)vid;
    }
}

// row splits of the sorted (voxel, vertex) pairs by binary search + payload extraction
__global__ void k_adj_splits(const u64* pairs, i64 np, i64 nv, i64* rs) {
    i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v > nv) return;
    const u64 key = (u64)v << 32;
    i64 lo = 0, hi = np;
    while (lo < hi) {
        i64 mid = (lo + hi) >> 1;
        if (pairs[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    rs[v] = lo;
}
__global__ void k_adj_payload(const u64* pairs, i64 np, int32_t* adj) {
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < np) adj[i] = (int32_t)(u32)pairs[i];
}

// active duals containing both voxels (:202-213): intersection of two ascending lists, in
// ascending order (== the insertion order into the reference's unordered_set)
__device__ inline int edge_duals(const i64* rs, const int32_t* adj, i64 a, i64 b, u32* out, int cap) {
    i64 i = rs[a], ie = rs[a + 1], j = rs[b], je = rs[b + 1];
    int n = 0;
    while (i < ie && j < je) {
        const int32_t x = adj[i], y = adj[j];
        if (x == y) {
            if (n < cap) out[n] = (u32)x;
            ++n;
            ++i;
            ++j;
        } else if (x < y)
            ++i;
        else
            ++j;
    }
    return n;
}

struct Face4 {  // smallset.h: sorted, duplicate free
    i64 d[4];
    int n;
};
__device__ inline void face_insert(Face4& f, i64 v) {
    int i = 0;
    while (i < f.n && f.d[i] < v) ++i;
    if (i < f.n && f.d[i] == v) return;
    for (int j = f.n; j > i; --j) f.d[j] = f.d[j - 1];
    f.d[i] = v;
    ++f.n;
}
__device__ inline Face4 face_of(const i64* c, int fi) {
    Face4 f;
    f.n = 0;
    for (int k = 0; k < 4; ++k) face_insert(f, c[c_cube_faces[fi][k]]);
    return f;
}
__device__ inline bool face_eq(const Face4& a, const Face4& b) {
    if (a.n != b.n) return false;
    for (int i = 0; i < a.n; ++i)
        if (a.d[i] != b.d[i]) return false;
    return true;
}
// :216-232
__device__ inline Face4 face_with_oriented_edge(const i64* c, i64 e0, i64 e1) {
    for (int fi = 0; fi < 6; ++fi)
        for (int j = 0; j < 4; ++j)
            if (c[c_cube_faces[fi][j]] == e0 && c[c_cube_faces[fi][(j + 1) & 3]] == e1) {
                Face4 f = face_of(c, fi);
                if (f.n >= 3) return f;
            }
    Face4 none;
    none.n = 0;
    return none;
}
__device__ inline bool dual_has_face(const i64* c, const Face4& face) {  // :235-244
    for (int fi = 0; fi < 6; ++fi)
        if (face_eq(face_of(c, fi), face)) return true;
    return false;
}
__device__ inline void load_dual(const i64* duals, const int32_t* active, u32 vid, i64* c) {
    const i64 d = active[vid];
    for (int k = 0; k < 8; ++k) c[k] = duals[d * 8 + k];
}

// One thread per (active dual, owned edge).  COUNT: number of triangles / fan centres it emits.
// FILL: orders the duals around the edge (:247-299) and writes the triangles (:364-451).
template <bool FILL>
__global__ __launch_bounds__(BLK) void k_contour_edges(const float* values, const i64* duals, float thr,
                                                       const int32_t* active, i64 na, const i64* rs,
                                                       const int32_t* adj, i64* tri_cnt, i64* extra_cnt,
                                                       const i64* tri_off, const i64* extra_off, float* vtx,
                                                       int32_t* tri, int* flags) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (!FILL && t == na * 3) {
        tri_cnt[t] = 0;
        extra_cnt[t] = 0;
    }
    if (t >= na * 3) return;
    const i64 vid = t / 3;
    const int e = (int)(t - vid * 3);
    const i64 d = active[vid];
    i64 a = duals[d * 8 + c_owned_edges[e][0]], b = duals[d * 8 + c_owned_edges[e][1]];
    u32 xs[ASR_USET_CAP];
    int n = 0;
    if (a != b && crossing(values, thr, a, b)) n = edge_duals(rs, adj, a, b, xs, ASR_USET_CAP);
    if (!FILL) {
        tri_cnt[t] = n == 3 ? 1 : (n == 4 ? 2 : (n > 4 ? n : 0));
        extra_cnt[t] = n > 4 ? 1 : 0;
        if (n > ASR_USET_CAP) atomicOr(&flags[F_DUAL_FAN], 1);
        return;
    }
    // n == 2 emits nothing but is sorted all the same: the reference sorts before it looks at n (:360-369), and two
    // cells without a common face end it there
    if (n < 2 || n > ASR_USET_CAP) return;
    if (values[a * 2] > values[b * 2]) {  // :357-358 orient from the lower to the higher value
        i64 s = a;
        a = b;
        b = s;
    }
    u32 rest[ASR_USET_CAP], sorted[ASR_USET_CAP];
    asr_uset_order(xs, n, rest);
    int nrest = n - 1, ns = 1;
    sorted[0] = rest[n - 1];
    bool reverse_again = false;
    for (int it = 0; it < n * n && nrest > 0; ++it) {
        i64 c1[8];
        load_dual(duals, active, sorted[ns - 1], c1);
        const Face4 face = face_with_oriented_edge(c1, a, b);
        int found = -1;
        for (int j = 0; j < nrest && found < 0; ++j) {
            i64 c2[8];
            load_dual(duals, active, rest[j], c2);
            if (dual_has_face(c2, face)) found = j;
        }
        if (found >= 0) {
            sorted[ns++] = rest[found];
            for (int j = found; j + 1 < nrest; ++j) rest[j] = rest[j + 1];
            --nrest;
        } else {
            for (int j = 0; j < ns / 2; ++j) {
                u32 s = sorted[j];
                sorted[j] = sorted[ns - 1 - j];
                sorted[ns - 1 - j] = s;
            }
            i64 s = a;
            a = b;
            b = s;
            reverse_again = !reverse_again;
        }
    }
    if (reverse_again)
        for (int j = 0; j < ns / 2; ++j) {
            u32 s = sorted[j];
            sorted[j] = sorted[ns - 1 - j];
            sorted[ns - 1 - j] = s;
        }
    if (ns != n) {  // "this should not happen: cannot sort duals" (:366-370)
        atomicOr(&flags[F_DUAL_SORT], 1);
        return;
    }
    if (n < 3) return;
    int32_t* out = tri + tri_off[t] * 3;
    if (n == 3) {
        out[0] = (int32_t)sorted[0];
        out[1] = (int32_t)sorted[1];
        out[2] = (int32_t)sorted[2];
    } else if (n == 4) {
        float p[4][3];
        for (int i = 0; i < 4; ++i)
            for (int q = 0; q < 3; ++q) p[i][q] = vtx[(i64)sorted[i] * 3 + q];
        // Eigen's unrolled sum for a 3-vector: x*x + (y*y + z*z)
        const float d0x = p[0][0] - p[2][0], d0y = p[0][1] - p[2][1], d0z = p[0][2] - p[2][2];
        const float d1x = p[1][0] - p[3][0], d1y = p[1][1] - p[3][1], d1z = p[1][2] - p[3][2];
        const float q02 = d0x * d0x + (d0y * d0y + d0z * d0z);
        const float q13 = d1x * d1x + (d1y * d1y + d1z * d1z);
        if (q02 > q13) {
            out[0] = (int32_t)sorted[0]; out[1] = (int32_t)sorted[1]; out[2] = (int32_t)sorted[3];
            out[3] = (int32_t)sorted[1]; out[4] = (int32_t)sorted[2]; out[5] = (int32_t)sorted[3];
        } else {
            out[0] = (int32_t)sorted[0]; out[1] = (int32_t)sorted[1]; out[2] = (int32_t)sorted[2];
            out[3] = (int32_t)sorted[0]; out[4] = (int32_t)sorted[2]; out[5] = (int32_t)sorted[3];
        }
    } else {
        float cx = 0, cy = 0, cz = 0;
        for (int i = 0; i < n; ++i) {
            cx += vtx[(i64)sorted[i] * 3 + 0];
            cy += vtx[(i64)sorted[i] * 3 + 1];
            cz += vtx[(i64)sorted[i] * 3 + 2];
        }
        const i64 ci = na + extra_off[t];
        vtx[ci * 3 + 0] = cx / (float)n;
        vtx[ci * 3 + 1] = cy / (float)n;
        vtx[ci * 3 + 2] = cz / (float)n;
        for (int i = 0; i < n; ++i) {
            out[i * 3 + 0] = (int32_t)sorted[i];
            out[i * 3 + 1] = (int32_t)sorted[(i + 1) % n];
            out[i * 3 + 2] = (int32_t)ci;
        }
    }
}

// ------------------------------------------------------------------------------------------
// connected components: lock-free union-find, the root of a set is its smallest vertex, so the
// rank of a root among the roots is the label the reference's DFS over i = 0..nv-1 assigns
// (postprocess.cpp:57-80)
// ------------------------------------------------------------------------------------------
__device__ inline int uf_find(int* parent, int x) {
    while (true) {
        int p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
        if (p == x) return x;
        int gp = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
        if (gp != p) __atomic_store_n(&parent[x], gp, __ATOMIC_RELAXED);  // path halving
        x = p;
    }
}
__device__ inline void uf_union(int* parent, int a, int b) {
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) {
            int s = a;
            a = b;
            b = s;
        }
        if (atomicCAS(&parent[a], a, b) == a) return;  // hang the larger root below the smaller
    }
}
__global__ void k_uf_init(int* parent, i64 n) {
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) parent[i] = (int)i;
}
__global__ void k_uf_link(const int32_t* tri, i64 nt, i64 nv, int* parent, int* flags) {
    i64 f = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nt) return;
    const int a = tri[f * 3], b = tri[f * 3 + 1], c = tri[f * 3 + 2];
    if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) {
        atomicOr(&flags[F_BAD_INDEX], 1);
        return;
    }
    uf_union(parent, a, b);
    uf_union(parent, b, c);
}
__global__ void k_uf_roots(int* parent, i64 n, i64* is_root) {
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        is_root[i] = 0;
        return;
    }
    const int r = uf_find(parent, (int)i);
    is_root[i] = r == (int)i ? 1 : 0;
}
// after k_uf_roots all paths are short; flatten and count members per component label
__global__ void k_comp_sizes(int* parent, i64 n, const i64* label_of_root, int32_t* comp, int* sizes) {
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;  // (exited lanes are inactive below: readfirstlane / ballot see active lanes only)
    const int r = uf_find(parent, (int)i);
    const int c = (int)label_of_root[r];
    comp[i] = c;
    // one atomic per distinct label in the wave (a mesh is mostly one component: 10^6 atomics on one
    // address would take 12 ms)
    bool todo = true;
    while (todo) {
        const int lead = __builtin_amdgcn_readfirstlane(c);
        const unsigned long long same = __ballot(c == lead);
        if (c == lead) {
            if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(&sizes[lead], __popcll(same));
            todo = false;
        }
    }
}
__global__ void k_comp_keys(const int* sizes, i64 nc, u64* keys) {
    i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < nc) keys[c] = ((u64)(u32)sizes[c] << 32) | (u64)c;  // std::greater on (size, label)
}
__global__ void k_comp_keep(const u64* sorted_desc, i64 nc, i64 keep_n, i64 min_size, uint8_t* keep) {
    i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nc) return;
    const u64 k = sorted_desc[r];
    keep[(u32)k] = (r < keep_n && (i64)(k >> 32) >= min_size) ? 1 : 0;
}
__global__ void k_vertex_keep(const int32_t* comp, const uint8_t* keep, i64 nv, i64* flag) {
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nv) return;
    flag[i] = (i < nv && keep[comp[i]]) ? 1 : 0;
}
__global__ void k_tri_keep(const int32_t* tri, i64 nt, const i64* voff, i64* flag) {
    i64 f = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (f > nt) return;
    bool k = false;
    if (f < nt) {
        k = true;
        for (int q = 0; q < 3; ++q) {
            const i64 v = tri[f * 3 + q];
            k &= voff[v + 1] > voff[v];
        }
    }
    flag[f] = k ? 1 : 0;
}
__global__ void k_compact_vertices(const float* in, i64 nv, const i64* voff, float* out) {
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv || voff[i + 1] == voff[i]) return;
    const i64 o = voff[i];
    out[o * 3 + 0] = in[i * 3 + 0];
    out[o * 3 + 1] = in[i * 3 + 1];
    out[o * 3 + 2] = in[i * 3 + 2];
}
__global__ void k_compact_triangles(const int32_t* in, i64 nt, const i64* voff, const i64* toff, int32_t* out) {
    i64 f = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nt || toff[f + 1] == toff[f]) return;
    const i64 o = toff[f];
    for (int q = 0; q < 3; ++q) out[o * 3 + q] = (int32_t)voff[in[f * 3 + q]];
}

// ------------------------------------------------------------------------------------------
// asr_hip_mesh_sample: stratified, area-weighted points on a triangle mesh.
// Areas are f64 from the f32 corners, P = their inclusive prefix sums (fixed summation order), A = P[last].  Sample s owns
// the stratum [s, s + 1) A / S of the parameter line: u = (s + r0) A / S, its triangle is the first t with P[t] > u -- a
// zero-area triangle has P[t] == P[t - 1] and is never that one.  Inside the triangle b1 = sqrt(r1) (1 - r2),
// b2 = sqrt(r1) r2 (uniform: the sqrt undoes the linear density of the distance to corner 0) and, in f32 without
// contraction, p = v0 + b1 (v1 - v0) + b2 (v2 - v0): a coordinate all three corners share comes out exactly.
// r0, r1, r2 are functions of (seed, s, stream) alone -- no state, no dependence on the launch:
//   h = fmix64(fmix64(seed + 0x9E3779B97F4A7C15 (stream + 1)) ^ (s * 0xBF58476D1CE4E5B9)),  fmix64 = murmur3's finaliser
//   r0 = (h >> 11) 2^-53 (f64, stream 0);  r1, r2 = (h >> 40) 2^-24 (f32, streams 1 and 2)
// One thread per sample; the binary search reads log2(T) prefix sums, the top levels of which stay in L2.
// ------------------------------------------------------------------------------------------
__device__ inline u64 sample_hash(u64 seed, u64 s, u64 stream) {
    return asr_hash64(asr_hash64(seed + 0x9E3779B97F4A7C15ull * (stream + 1)) ^ (s * 0xBF58476D1CE4E5B9ull));
}
__global__ void k_tri_areas(const float* vtx, i64 nv, const int32_t* tri, i64 nt, double* area, int* flags) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const int a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
    if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) {
        atomicOr(&flags[F_BAD_INDEX], 1);
        area[t] = 0.0;
        return;
    }
    const double ax = vtx[3 * (i64)a], ay = vtx[3 * (i64)a + 1], az = vtx[3 * (i64)a + 2];
    const double ux = vtx[3 * (i64)b] - ax, uy = vtx[3 * (i64)b + 1] - ay, uz = vtx[3 * (i64)b + 2] - az;
    const double wx = vtx[3 * (i64)c] - ax, wy = vtx[3 * (i64)c + 1] - ay, wz = vtx[3 * (i64)c + 2] - az;
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const double ar = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
    area[t] = ar > 0.0 ? ar : 0.0;  // NaN corners: no area (an infinite one makes the total infinite: refused)
}
__global__ void k_mesh_sample(const float* __restrict__ vtx, const int32_t* __restrict__ tri, i64 nt,
                              const double* __restrict__ prefix, i64 num_samples, u64 seed, float* points,
                              float* normals, int32_t* tri_out) {
    const i64 s = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= num_samples) return;
    const double total = prefix[nt - 1];
    const double r0 = (double)(sample_hash(seed, (u64)s, 0) >> 11) * 0x1p-53;
    const float r1 = (float)(sample_hash(seed, (u64)s, 1) >> 40) * 0x1p-24f;
    const float r2 = (float)(sample_hash(seed, (u64)s, 2) >> 40) * 0x1p-24f;
    double u = ((double)s + r0) * total / (double)num_samples;
    if (!(u < total)) u = total * (1.0 - 0x1p-52);  // rounding at the top end: the last triangle with an area
    i64 lo = 0, hi = nt - 1;  // first t with prefix[t] > u (prefix[nt - 1] = total > u)
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if (prefix[mid] > u)
            hi = mid;
        else
            lo = mid + 1;
    }
    const i64 a = tri[lo * 3], b = tri[lo * 3 + 1], c = tri[lo * 3 + 2];
    const float ax = vtx[3 * a], ay = vtx[3 * a + 1], az = vtx[3 * a + 2];
    const float ux = vtx[3 * b] - ax, uy = vtx[3 * b + 1] - ay, uz = vtx[3 * b + 2] - az;
    const float wx = vtx[3 * c] - ax, wy = vtx[3 * c + 1] - ay, wz = vtx[3 * c + 2] - az;
    const float sr = sqrtf(r1);
    const float b1 = sr * (1.f - r2), b2 = sr * r2;
    points[3 * s] = ax + b1 * ux + b2 * wx;
    points[3 * s + 1] = ay + b1 * uy + b2 * wy;
    points[3 * s + 2] = az + b1 * uz + b2 * wz;
    if (tri_out) tri_out[s] = (int32_t)lo;
    if (normals) {
        const double nx = (double)uy * wz - (double)uz * wy, ny = (double)uz * wx - (double)ux * wz,
                     nz = (double)ux * wy - (double)uy * wx;
        const double inv = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);  // > 0: the triangle has an area
        normals[3 * s] = (float)(nx * inv);
        normals[3 * s + 1] = (float)(ny * inv);
        normals[3 * s + 2] = (float)(nz * inv);
    }
}

// ------------------------------------------------------------------------------------------
// asr_hip_mesh_simplify: octree vertex clustering with quadric placement (contract: include/asr_hip.h).
//   keys      one thread per vertex: key of its cell, checks of the level and of the position
//   clusters  stable radix sort of (key, vertex); run heads + scan give the cluster ids in ascending key order
//   corners   (cluster, 3t + j) pairs, stable radix sort: the corners of a cluster are one segment in ascending 3t + j
//   solve     one wave per cluster: lane l takes the items l, l + 64, ... of the vertex and of the corner segment in
//             order, a xor butterfly adds the 64 partial sums (a + b == b + a: every lane ends with the same bits), the
//             3x3 system is solved with an LDL^T factorisation.  No atomics: the same bits on every run.
//   triangles two stable sort passes over the sorted cluster triple (largest id, then the other two as one key) with the
//             input index as payload: equal triples become runs in ascending input index, the run heads survive
//   compact   scans of the survivor flags and of the referenced clusters
// ------------------------------------------------------------------------------------------
__global__ void k_simp_keys(asr_octree_frame f, const float* vtx, i64 nv, const int8_t* levels, int level, u64* keys,
                            int32_t* ids, int* flags) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const int l = levels ? (int)levels[i] : level;
    int x = 0, y = 0, z = 0;
    u64 key = 1;  // the root: what a refused vertex gets (the call fails before anything reads it)
    if (l < 0 || l > ASR_MAX_LEVEL) {
        atomicOr(&flags[F_BAD_LEVEL], 1);
    } else if (!frame_coord21_checked(f, vtx[3 * i], vtx[3 * i + 1], vtx[3 * i + 2], x, y, z)) {
        atomicOr(&flags[F_OUTSIDE], 1);
    } else {
        const int s = ASR_MAX_LEVEL - l;
        key = asr_coord_key(x >> s, y >> s, z >> s, l);
    }
    keys[i] = key;
    ids[i] = (int32_t)i;
}
__global__ void k_simp_heads(const u64* keys, i64 n, i64* head) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    head[r] = (r < n && (r == 0 || keys[r] != keys[r - 1])) ? 1 : 0;
}
// hoff: exclusive scan of the head flags; position r of the sorted list lies in cluster hoff[r + 1] - 1
__global__ void k_simp_clusters(const u64* keys, const int32_t* ids, i64 n, const i64* hoff, int32_t* cluster,
                                u64* ckey, i64* cstart) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    if (r == n) {
        cstart[hoff[n]] = n;
        return;
    }
    const i64 c = hoff[r + 1] - 1;
    cluster[ids[r]] = (int32_t)c;
    if (hoff[r + 1] != hoff[r]) {
        ckey[c] = keys[r];
        cstart[c] = r;
    }
}
__global__ void k_simp_corner_keys(const int32_t* tri, i64 ncorner, i64 nv, const int32_t* cluster, u32* ck, u32* cv,
                                   int* flags) {
    const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ncorner) return;
    const int v = tri[q];
    u32 c = 0;
    if (v < 0 || v >= nv)
        atomicOr(&flags[F_BAD_INDEX], 1);
    else
        c = (u32)cluster[v];
    ck[q] = c;
    cv[q] = (u32)q;
}
// kstart[c] = first position of the sorted corner list with cluster >= c (c = 0..nc)
__global__ void k_simp_corner_starts(const u32* ck, i64 ncorner, i64 nc, i64* kstart) {
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nc) return;
    i64 lo = 0, hi = ncorner;
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if ((i64)ck[mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    kstart[c] = lo;
}
__device__ inline double wave_sum(double v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__global__ void __launch_bounds__(BLK) k_simp_solve(asr_octree_frame f, const float* __restrict__ vtx,
                                                    const int32_t* __restrict__ tri, const int32_t* __restrict__ ids,
                                                    const u64* __restrict__ ckey, const i64* __restrict__ cstart,
                                                    const u32* __restrict__ corner, const i64* __restrict__ kstart,
                                                    i64 nc, float* __restrict__ cpos) {
    const i64 c = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (c >= nc) return;  // whole waves leave: the shuffles below see 64 lanes
    const i64 v0 = cstart[c], v1 = cstart[c + 1];
    if (v1 - v0 == 1) {  // a vertex alone in its cell keeps its bits
        if (lane < 3) cpos[3 * c + lane] = vtx[3 * (i64)ids[v0] + lane];
        return;
    }
    int cx, cy, cz, l;
    asr_key_coord(ckey[c], cx, cy, cz, l);
    const int s = ASR_MAX_LEVEL - l;
    const double vs = (double)f.voxel_size[ASR_MAX_LEVEL], half = 0.5 * (double)(i64(1) << s);
    const double ctr[3] = {((double)((cx << s) - f.offset[0]) + half) * vs,
                           ((double)((cy << s) - f.offset[1]) + half) * vs,
                           ((double)((cz << s) - f.offset[2]) + half) * vs};
    double m[3] = {0, 0, 0}, A[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};  // A: xx xy xz yy yz zz
    for (i64 r = v0 + lane; r < v1; r += 64) {
        const i64 v = ids[r];
        for (int d = 0; d < 3; ++d) m[d] += (double)vtx[3 * v + d] - ctr[d];
    }
    for (i64 k = kstart[c] + lane; k < kstart[c + 1]; k += 64) {
        const i64 t = corner[k] / 3;
        double p[3][3];
        for (int j = 0; j < 3; ++j) {
            const i64 v = tri[3 * t + j];
            for (int d = 0; d < 3; ++d) p[j][d] = (double)vtx[3 * v + d] - ctr[d];
        }
        const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
        const double wx = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wz = p[2][2] - p[0][2];
        const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        const double len = sqrt(nx * nx + ny * ny + nz * nz);
        if (!(len > 0.0)) continue;
        const double w = 2.0 * len, d = -(nx * p[0][0] + ny * p[0][1] + nz * p[0][2]);
        A[0] += nx * nx / w;
        A[1] += nx * ny / w;
        A[2] += nx * nz / w;
        A[3] += ny * ny / w;
        A[4] += ny * nz / w;
        A[5] += nz * nz / w;
        b[0] += d * nx / w;
        b[1] += d * ny / w;
        b[2] += d * nz / w;
    }
    for (int d = 0; d < 3; ++d) m[d] = wave_sum(m[d]) / (double)(v1 - v0);
    for (int d = 0; d < 6; ++d) A[d] = wave_sum(A[d]);
    for (int d = 0; d < 3; ++d) b[d] = wave_sum(b[d]);
    double x[3] = {m[0], m[1], m[2]};
    const double trA = A[0] + A[3] + A[5];
    if (trA > 0.0) {
        const double eps = 1e-3 * trA / 3.0;
        const double r0 = -b[0] + eps * m[0], r1 = -b[1] + eps * m[1], r2 = -b[2] + eps * m[2];
        // (A + eps I) = L D L^T, symmetric positive definite
        const double d0 = A[0] + eps, l10 = A[1] / d0, l20 = A[2] / d0;
        const double d1 = (A[3] + eps) - l10 * A[1];
        const double e21 = A[4] - l20 * A[1], l21 = e21 / d1;
        const double d2 = (A[5] + eps) - l20 * A[2] - l21 * e21;
        const double y0 = r0, y1 = r1 - l10 * y0, y2 = r2 - l20 * y0 - l21 * y1;
        x[2] = y2 / d2;
        x[1] = y1 / d1 - l21 * x[2];
        x[0] = y0 / d0 - l10 * x[1] - l20 * x[2];
    }
    const double hh = 0.5 * (double)f.voxel_size[l];
    if (lane < 3) {
        double xv = lane == 0 ? x[0] : lane == 1 ? x[1] : x[2];
        const double cv = lane == 0 ? ctr[0] : lane == 1 ? ctr[1] : ctr[2];
        xv = xv < -hh ? -hh : xv > hh ? hh : xv;
        cpos[3 * c + lane] = (float)(cv + xv);
    }
}
// sorted cluster triple of every triangle: hi[t] (pass one's key), lomid[t] = lo << bits | mid; degenerate[t]
__global__ void k_simp_triples(const int32_t* tri, i64 nt, const int32_t* cluster, int bits, u32* hi, u64* lomid,
                               u32* tid) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    u32 a = (u32)cluster[tri[3 * t]], b = (u32)cluster[tri[3 * t + 1]], c = (u32)cluster[tri[3 * t + 2]];
    if (a > b) { const u32 s = a; a = b; b = s; }
    if (b > c) { const u32 s = b; b = c; c = s; }
    if (a > b) { const u32 s = a; a = b; b = s; }
    hi[t] = c;
    lomid[t] = ((u64)a << bits) | (u64)b;
    tid[t] = (u32)t;
}
__global__ void k_simp_gather_lomid(const u64* lomid, const u32* order, i64 nt, u64* out) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nt) out[r] = lomid[order[r]];
}
// order: triangles sorted on their triple, equal triples in ascending input index; the head of a run survives unless
// two of its corners share a cluster
__global__ void k_simp_survivors(const u32* order, const u64* lomid_sorted, const u32* hi, i64 nt, int bits, i64* flag) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nt) return;
    if (r == nt) {
        flag[nt] = 0;
        return;
    }
    const u32 t = order[r];
    const u64 lm = lomid_sorted[r];
    const u32 c = hi[t], a = (u32)(lm >> bits), b = (u32)(lm & ((u64(1) << bits) - 1));
    bool head = r == 0 || lomid_sorted[r - 1] != lm || hi[order[r - 1]] != c;
    flag[t] = (head && a != b && b != c) ? 1 : 0;
}
__global__ void k_simp_mark(const int32_t* tri, i64 nt, const i64* toff, const int32_t* cluster, i64* cref) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || toff[t + 1] == toff[t]) return;
    for (int j = 0; j < 3; ++j) cref[cluster[tri[3 * t + j]]] = 1;  // every writer stores the same value
}
__global__ void k_simp_out_vertices(const float* cpos, i64 nc, const i64* coff, float* out) {
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc || coff[c + 1] == coff[c]) return;
    const i64 o = coff[c];
    for (int d = 0; d < 3; ++d) out[3 * o + d] = cpos[3 * c + d];
}
__global__ void k_simp_out_triangles(const int32_t* tri, i64 nt, const i64* toff, const int32_t* cluster,
                                     const i64* coff, int32_t* out) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || toff[t + 1] == toff[t]) return;
    const i64 o = toff[t];
    for (int j = 0; j < 3; ++j) out[3 * o + j] = (int32_t)coff[cluster[tri[3 * t + j]]];
}
// cluster == nullptr: no triangle survived, nothing is referenced
__global__ void k_simp_vertex_map(const int32_t* cluster, const i64* coff, i64 nv, int32_t* map) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    int32_t o = -1;
    if (cluster) {
        const i64 c = cluster[i];
        if (coff[c + 1] != coff[c]) o = (int32_t)coff[c];
    }
    map[i] = o;
}

// ------------------------------------------------------------------------------------------
// Mesh adjacency (contract: include/asr_hip.h): edge table, topology report, Taubin smoothing.
// Every side of a non-degenerate triangle becomes the key (lo << 32) | (hi << 1) | forward; sorted, the runs of equal
// (lo, hi) are the edges in ascending order and, inside a run, the backward uses come before the forward ones.  The sides
// of degenerate triangles (and of triangles with a corner out of range, which fail the call) get the key nv << 32 and
// sort behind every edge.
// ------------------------------------------------------------------------------------------
constexpr int SMOOTH_CUT = 128;  // rows longer than this are summed by a whole wave (k_smooth_step_long)
enum { TOPO_DEGENERATE = 0, TOPO_EDGES, TOPO_BOUNDARY, TOPO_NONMANIFOLD, TOPO_INCONSISTENT, TOPO_USED, TOPO_COMPONENTS,
       TOPO_LOOPS, TOPO_COUNTERS };
typedef unsigned long long ull;

// one atomic per wave: the lanes that return early are not active here and are left out of the ballot
__device__ inline void wave_count(ull* counter, bool pred) {
    const ull m = __ballot(pred);
    if (pred && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(counter, (ull)__popcll(m));
}
__global__ void k_adj_edge_keys(const int32_t* tri, i64 nq, i64 nv, u64* keys, int* flags, ull* degenerate) {
    const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const i64 t = q / 3;
    const int j = (int)(q - 3 * t);
    const int c0 = tri[3 * t], c1 = tri[3 * t + 1], c2 = tri[3 * t + 2];
    u64 key = (u64)nv << 32;
    bool degen = false;
    if (c0 < 0 || c1 < 0 || c2 < 0 || c0 >= nv || c1 >= nv || c2 >= nv) {
        if (j == 0) atomicOr(&flags[F_BAD_INDEX], 1);
    } else if (c0 == c1 || c1 == c2 || c0 == c2) {
        degen = j == 0;
    } else {
        const int u = j == 0 ? c0 : j == 1 ? c1 : c2, v = j == 0 ? c1 : j == 1 ? c2 : c0;
        const int lo = u < v ? u : v, hi = u < v ? v : u;
        key = ((u64)(u32)lo << 32) | ((u64)(u32)hi << 1) | (u64)(u < v ? 1 : 0);
    }
    keys[q] = key;
    if (degenerate) wave_count(degenerate, degen);
}
// head[i] = 1 where an edge's run starts (i <= nq, head[nq] = 0); *nvalid = the number of sides that belong to edges
__global__ void k_adj_edge_heads(const u64* keys, i64 nq, i64 nv, i64* head, i64* nvalid) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nq) return;
    const bool prev_edge = i > 0 && (i64)(keys[i - 1] >> 32) < nv;
    if (i == nq) {
        head[i] = 0;
        if (nq == 0 || prev_edge) *nvalid = nq;
        return;
    }
    const u64 k = keys[i];
    if ((i64)(k >> 32) >= nv) {
        head[i] = 0;
        if (i == 0 || prev_edge) *nvalid = i;
        return;
    }
    head[i] = (i == 0 || (keys[i - 1] >> 1) != (k >> 1)) ? 1 : 0;
}
__global__ void k_adj_edge_starts(const i64* eoff, i64 nq, const i64* nvalid, i64* estart) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nq) return;
    if (i == nq)
        estart[eoff[nq]] = *nvalid;
    else if (eoff[i + 1] > eoff[i])
        estart[eoff[i]] = i;
}
// the table from the run bounds; cap >= the number of edges (the launch's size), any output may be null
__global__ void k_adj_edge_out(const u64* keys, const i64* estart, const i64* ecount, i64 cap, int32_t* edges, int32_t* uses,
                               int32_t* forward) {
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cap || e >= *ecount) return;
    const i64 b = estart[e], end = estart[e + 1];
    if (edges) {
        const u64 k = keys[b];
        edges[2 * e] = (int32_t)(k >> 32);
        edges[2 * e + 1] = (int32_t)((k >> 1) & 0x7fffffffu);
    }
    if (uses) uses[e] = (int32_t)(end - b);
    if (forward) {  // the first forward use of the run
        i64 lo = b, hi = end;
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (keys[mid] & 1)
                hi = mid;
            else
                lo = mid + 1;
        }
        forward[e] = (int32_t)(end - lo);
    }
}
__global__ void k_adj_topo_edges(const int32_t* uses, const int32_t* forward, const i64* ecount, i64 cap, ull* cnt) {
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) cnt[TOPO_EDGES] = (ull)*ecount;
    if (e >= cap || e >= *ecount) return;
    const int u = uses[e];
    wave_count(&cnt[TOPO_BOUNDARY], u == 1);
    wave_count(&cnt[TOPO_NONMANIFOLD], u >= 3);
    wave_count(&cnt[TOPO_INCONSISTENT], u == 2 && forward[e] != 1);
}
// k_uf_link for an edge list: boundary_only = 1 links the edges with one use only; mark[v] = 1 for every linked vertex
__global__ void k_uf_link_edges(const int32_t* edges, const int32_t* uses, const i64* ecount, i64 cap, int boundary_only,
                                int* parent, uint8_t* mark) {
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cap || e >= *ecount) return;
    if (boundary_only && uses[e] != 1) return;
    const int a = edges[2 * e], b = edges[2 * e + 1];
    mark[a] = 1;
    mark[b] = 1;
    uf_union(parent, a, b);
}
__global__ void k_adj_topo_vertices(int* parent_all, const uint8_t* used, int* parent_bnd, const uint8_t* on_bnd, i64 nv,
                                    ull* cnt) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const bool u = used[i] != 0, b = on_bnd[i] != 0;
    wave_count(&cnt[TOPO_USED], u);
    wave_count(&cnt[TOPO_COMPONENTS], u && uf_find(parent_all, (int)i) == (int)i);
    wave_count(&cnt[TOPO_LOOPS], b && uf_find(parent_bnd, (int)i) == (int)i);
}
// both directions of every edge as (source << 32) | (target << 1) | feature; feature vertices are marked
__global__ void k_adj_csr_pairs(const int32_t* edges, const int32_t* uses, i64 ne, u64* pairs, uint8_t* vfeat) {
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const u32 a = (u32)edges[2 * e], b = (u32)edges[2 * e + 1];
    const u64 feat = uses[e] != 2 ? 1 : 0;
    pairs[2 * e] = ((u64)a << 32) | ((u64)b << 1) | feat;
    pairs[2 * e + 1] = ((u64)b << 32) | ((u64)a << 1) | feat;
    if (feat) {
        vfeat[a] = 1;
        vfeat[b] = 1;
    }
}
__global__ void k_smooth_long_flags(const i64* rs, i64 nv, i64* flag) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nv) return;
    flag[i] = (i < nv && rs[i + 1] - rs[i] > SMOOTH_CUT) ? 1 : 0;
}
__global__ void k_smooth_long_list(const i64* loff, i64 nv, int32_t* list) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nv && loff[i + 1] > loff[i]) list[loff[i]] = (int32_t)i;
}
// positions: three doubles per vertex (24-byte slots; slots padded to 32 bytes and read as two aligned 16-byte loads were
// measured slower)
__device__ inline void pos_load(const double* p, i64 i, double& x, double& y, double& z) {
    x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
}
__device__ inline void pos_store(double* p, i64 i, double x, double y, double z) {
    p[3 * i] = x, p[3 * i + 1] = y, p[3 * i + 2] = z;
}
__global__ void k_smooth_load(const float* vtx, i64 nv, double* pos, int* flags) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const float x = vtx[3 * i], y = vtx[3 * i + 1], z = vtx[3 * i + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) atomicOr(&flags[F_BAD_VERTEX], 1);
    pos_store(pos, i, (double)x, (double)y, (double)z);
}
__global__ void k_smooth_store(const double* pos, i64 nv, float* vtx) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    double x, y, z;
    pos_load(pos, i, x, y, z);
    vtx[3 * i] = (float)x, vtx[3 * i + 1] = (float)y, vtx[3 * i + 2] = (float)z;
}
// which entries of vertex i's row count: none (-1, the vertex stays), the feature entries only (1), all (0)
__device__ inline int smooth_row_filter(int mode, const uint8_t* vfeat, i64 i) {
    if (mode == 0 || !vfeat[i]) return 0;
    return mode == 1 ? -1 : 1;
}
__device__ inline void smooth_update(double& px, double& py, double& pz, double sx, double sy, double sz, i64 n, double f) {
    if (n == 0) return;
    const double d = (double)n;
    px = px + f * (sx / d - px);
    py = py + f * (sy / d - py);
    pz = pz + f * (sz / d - pz);
}
// one step, one thread per row of at most SMOOTH_CUT entries: a sequential sum in ascending neighbour order
__global__ __launch_bounds__(BLK) void k_smooth_step(const double* __restrict__ pin, double* __restrict__ pout, i64 nv,
                                                     const i64* __restrict__ rs, const int32_t* __restrict__ adj,
                                                     const uint8_t* __restrict__ vfeat, int mode, double f) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const i64 b = rs[i], e = rs[i + 1];
    if (e - b > SMOOTH_CUT) return;  // k_smooth_step_long writes this row
    double px, py, pz;
    pos_load(pin, i, px, py, pz);
    const int filter = smooth_row_filter(mode, vfeat, i);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    i64 n = 0;
    if (filter >= 0)
        for (i64 k = b; k < e; ++k) {
            const u32 a = (u32)adj[k];
            if (filter && !(a & 1)) continue;
            double x, y, z;
            pos_load(pin, (i64)(a >> 1), x, y, z);
            sx += x, sy += y, sz += z;
            ++n;
        }
    smooth_update(px, py, pz, sx, sy, sz, n, f);
    pos_store(pout, i, px, py, pz);
}
// the rows longer than SMOOTH_CUT, one wave per row: lane l sums the entries l, l + 64, ... in order, then the 64 partial
// sums are added pairwise (xor 32, 16, ... 1): a fixed shape
__global__ __launch_bounds__(BLK) void k_smooth_step_long(const double* __restrict__ pin, double* __restrict__ pout,
                                                          const int32_t* __restrict__ rows, i64 nrows,
                                                          const i64* __restrict__ rs, const int32_t* __restrict__ adj,
                                                          const uint8_t* __restrict__ vfeat, int mode, double f) {
    const i64 w = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (w >= nrows) return;  // whole waves leave together
    const i64 i = rows[w];
    const i64 b = rs[i], e = rs[i + 1];
    const int filter = smooth_row_filter(mode, vfeat, i);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int n = 0;
    if (filter >= 0)
        for (i64 k = b + lane; k < e; k += 64) {
            const u32 a = (u32)adj[k];
            if (filter && !(a & 1)) continue;
            double x, y, z;
            pos_load(pin, (i64)(a >> 1), x, y, z);
            sx += x, sy += y, sz += z;
            ++n;
        }
    for (int m = 32; m >= 1; m >>= 1) {
        sx += __shfl_xor(sx, m);
        sy += __shfl_xor(sy, m);
        sz += __shfl_xor(sz, m);
        n += __shfl_xor(n, m);
    }
    if (lane != 0) return;
    double px, py, pz;
    pos_load(pin, i, px, py, pz);
    smooth_update(px, py, pz, sx, sy, sz, (i64)n, f);
    pos_store(pout, i, px, py, pz);
}

// ------------------------------------------------------------------------------------------
// Hole filling (contract: include/asr_hip.h).  The boundary edges (uses == 1) are directed tail -> head
// as their one triangle runs through them; a rim is a set of the union-find over the boundary edges alone and its id the
// set's root, its smallest vertex.  A rim is simple when every vertex of it leaves and enters exactly once; the simple
// rims of at most max_edges edges get a fan: the sorted keys (rim id << 32) | vertex give the ascending vertex order
// the hub sums in and the order of the new triangles.
// ------------------------------------------------------------------------------------------
constexpr int FILL_CUT = SMOOTH_CUT;  // rims longer than this are summed by a whole wave (k_fill_hub_long)
enum { FILL_RIMS = 0, FILL_FILLED, FILL_TOO_LONG, FILL_NOT_SIMPLE, FILL_RIM_VERTICES, FILL_COUNTERS };

__global__ void k_fill_degrees(const int32_t* edges, const int32_t* uses, const int32_t* forward, const i64* ecount, i64 cap,
                               int* out_deg, int* in_deg, int* succ) {
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cap || e >= *ecount) return;
    if (uses[e] != 1) return;
    const int lo = edges[2 * e], hi = edges[2 * e + 1];
    const bool fw = forward[e] == 1;
    const int tail = fw ? lo : hi, head = fw ? hi : lo;
    atomicAdd(&out_deg[tail], 1);
    atomicAdd(&in_deg[head], 1);
    succ[tail] = head;  // one writer per tail on a simple rim; the others are never walked
}
// per boundary vertex: its rim, the rim's length (the edges that leave its vertices) and whether it is not simple
__global__ void k_fill_rim_stats(int* parent, const uint8_t* on_bnd, const int* out_deg, const int* in_deg, i64 nv,
                                 int* root_of, int* len, int* bad) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    if (!on_bnd[i]) {
        root_of[i] = -1;
        return;
    }
    const int r = uf_find(parent, (int)i);
    root_of[i] = r;
    const int od = out_deg[i];
    if (od != 1 || in_deg[i] != 1) atomicOr(&bad[r], 1);
    if (od > 1) atomicAdd(&len[r], od);
    // the vertices that leave once: one atomic per distinct rim in the wave (an outer border has 10^5 of them)
    bool todo = od == 1;
    while (todo) {
        const int lead = __builtin_amdgcn_readfirstlane(r);
        const unsigned long long same = __ballot(r == lead);
        if (r == lead) {
            if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(&len[lead], __popcll(same));
            todo = false;
        }
    }
}
// the decision per rim id (i <= nv; the entries of the vertices that are no rim id, and entry nv, are 0)
__global__ void k_fill_select(const uint8_t* on_bnd, const int* root_of, const int* len, const int* bad, i64 nv,
                              int max_edges, uint8_t* filled_rim, i64* hub_flag, i64* tri_count, i64* long_flag, ull* cnt) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nv) return;
    if (i == nv) {
        hub_flag[i] = tri_count[i] = long_flag[i] = 0;
        return;
    }
    const bool rim = on_bnd[i] && root_of[i] == (int)i;
    const int n = rim ? len[i] : 0;
    const bool simple = rim && !bad[i];
    const bool filled = simple && n <= max_edges;
    filled_rim[i] = filled ? 1 : 0;
    hub_flag[i] = filled && n >= 4 ? 1 : 0;
    tri_count[i] = filled ? (n == 3 ? 1 : n) : 0;
    long_flag[i] = filled && n > FILL_CUT ? 1 : 0;
    wave_count(&cnt[FILL_RIMS], rim);
    wave_count(&cnt[FILL_FILLED], filled);
    wave_count(&cnt[FILL_TOO_LONG], simple && !filled);
    wave_count(&cnt[FILL_NOT_SIMPLE], rim && !simple);
    if (filled) atomicAdd(&cnt[FILL_RIM_VERTICES], (ull)n);
}
// (rim id << 32) | vertex for the vertices of the filled rims -- the only vertices whose coordinates are read -- and
// nv << 32, which sorts behind them, for all others
__global__ void k_fill_keys(const float* vtx, const int* root_of, const uint8_t* filled_rim, i64 nv, u64* keys, int* flags) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const int r = root_of[i];
    u64 key = (u64)nv << 32;
    if (r >= 0 && filled_rim[r]) {
        const float x = vtx[3 * i], y = vtx[3 * i + 1], z = vtx[3 * i + 2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) atomicOr(&flags[F_BAD_VERTEX], 1);
        key = ((u64)(u32)r << 32) | (u64)(u32)i;
    }
    keys[i] = key;
}
__global__ void k_fill_starts(const u64* keys, i64 nv, int* start) {
    const i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nv) return;
    const i64 rim = (i64)(keys[p] >> 32);
    if (rim >= nv) return;
    if (p == 0 || (i64)(keys[p - 1] >> 32) != rim) start[rim] = (int)p;
}
__global__ void k_fill_lists(const i64* hub_off, const i64* long_off, i64 nv, int32_t* hub_rims, int32_t* long_rims) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    if (hub_off[i + 1] > hub_off[i]) hub_rims[hub_off[i]] = (int32_t)i;
    if (long_off[i + 1] > long_off[i]) long_rims[long_off[i]] = (int32_t)i;
}
// the hub of a rim of at most FILL_CUT vertices, one thread per hub: a sequential sum in ascending vertex order
__global__ __launch_bounds__(BLK) void k_fill_hub(const float* __restrict__ vtx, const u64* __restrict__ keys,
                                                  const int* __restrict__ len, const int* __restrict__ start,
                                                  const int32_t* __restrict__ hub_rims, i64 nhubs, float* __restrict__ hubs) {
    const i64 h = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= nhubs) return;
    const int rim = hub_rims[h];
    const int n = len[rim];
    if (n > FILL_CUT) return;  // k_fill_hub_long writes this hub
    const u64* row = keys + start[rim];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = 0; k < n; ++k) {
        const i64 v = (i64)(u32)row[k];
        sx += (double)vtx[3 * v], sy += (double)vtx[3 * v + 1], sz += (double)vtx[3 * v + 2];
    }
    const double d = (double)n;
    hubs[3 * h] = (float)(sx / d), hubs[3 * h + 1] = (float)(sy / d), hubs[3 * h + 2] = (float)(sz / d);
}
// the longer rims, one wave per rim: the shape of k_smooth_step_long
__global__ __launch_bounds__(BLK) void k_fill_hub_long(const float* __restrict__ vtx, const u64* __restrict__ keys,
                                                       const int* __restrict__ len, const int* __restrict__ start,
                                                       const i64* __restrict__ hub_off, const int32_t* __restrict__ long_rims,
                                                       i64 nlong, float* __restrict__ hubs) {
    const i64 w = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (w >= nlong) return;  // whole waves leave together
    const int rim = long_rims[w];
    const int n = len[rim];
    const u64* row = keys + start[rim];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = lane; k < n; k += 64) {
        const i64 v = (i64)(u32)row[k];
        sx += (double)vtx[3 * v], sy += (double)vtx[3 * v + 1], sz += (double)vtx[3 * v + 2];
    }
    for (int m = 32; m >= 1; m >>= 1) {
        sx += __shfl_xor(sx, m);
        sy += __shfl_xor(sy, m);
        sz += __shfl_xor(sz, m);
    }
    if (lane != 0) return;
    const i64 h = hub_off[rim];
    const double d = (double)n;
    hubs[3 * h] = (float)(sx / d), hubs[3 * h + 1] = (float)(sy / d), hubs[3 * h + 2] = (float)(sz / d);
}
// one thread per vertex of a filled rim, in key order: the triangle across the boundary edge that leaves it
__global__ void k_fill_emit(const u64* keys, i64 nrv, const int* len, const int* start, const int* succ, const i64* hub_off,
                            const i64* tri_off, i64 nv, int32_t* tri) {
    const i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nrv) return;
    const u64 k = keys[p];
    const int rim = (int)(k >> 32), a = (int)(u32)k;
    const i64 r = p - start[rim];
    if (len[rim] == 3) {  // no hub: (m, p, s) with p -> m -> s
        if (r != 0) return;
        const int s = succ[a], q = succ[s];
        int32_t* o = tri + 3 * tri_off[rim];
        o[0] = a, o[1] = q, o[2] = s;
        return;
    }
    int32_t* o = tri + 3 * (tri_off[rim] + r);
    o[0] = succ[a], o[1] = a, o[2] = (int32_t)(nv + hub_off[rim]);
}

MeshState& mstate(asr_hip_context* ctx) {
    if (!ctx->mesh_state) ctx->mesh_state = new MeshState();
    return *(MeshState*)ctx->mesh_state;
}
}  // namespace

void asr_mesh_release(asr_hip_context* ctx) {
    delete (MeshState*)ctx->mesh_state;
    ctx->mesh_state = nullptr;
}

int asr_mesh_contour_count(asr_hip_context* ctx, const float* values, i64 num_values, const i64* duals,
                           i64 num_duals, const float* positions, float threshold, i64* num_vertices,
                           i64* num_triangles) {
    ASR_TRY(count_begin(ctx));
    ContourState& st = mstate(ctx).contour;
    st = ContourState();
    *num_vertices = 0;
    *num_triangles = 0;
    if (num_duals <= 0 || num_values <= 0) return count_done(ctx, PendingOp::Contour);
    if (num_values >= (i64(1) << 31) || num_duals >= (i64(1) << 31))
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "contour: more than 2^31 voxels or dual cells");
    hipStream_t s = ctx->stream;
    SCRATCH_ALLOC(flag, i64, num_duals + 1);
    SCRATCH_ALLOC(npairs, i64, num_duals + 1);
    SCRATCH_ALLOC(voff, i64, num_duals + 1);
    SCRATCH_ALLOC(poff, i64, num_duals + 1);
    k_contour_active<<<grid_for(num_duals + 1, BLK), BLK, 0, s>>>(values, num_values, duals, num_duals, threshold,
                                                                   flag, npairs, ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, flag, voff, num_duals + 1));
    ASR_TRY(scan_counts(ctx, ctx->scratch, npairs, poff, num_duals + 1));
    i64 na = 0, np = 0;
    ASR_TRY(read_i64(ctx, voff + num_duals, &na));
    ASR_TRY(read_i64(ctx, poff + num_duals, &np));
    HostFlags host;
    ASR_TRY(read_flags(ctx, host));
    if (host[F_BAD_INDEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "contour: dual vertex index out of range");
    st.values = values;
    st.duals = duals;
    st.thr = threshold;
    st.num_active = na;
    if (na == 0) return count_done(ctx, PendingOp::Contour);
    SCRATCH_ALLOC(active, int32_t, na);
    SCRATCH_ALLOC(pairs, u64, np);
    SCRATCH_ALLOC(pairs_sorted, u64, np);
    SCRATCH_ALLOC(adj_rs, i64, num_values + 1);
    SCRATCH_ALLOC(adj, int32_t, np);
    SCRATCH_ALLOC(tri_cnt, i64, na * 3 + 1);
    SCRATCH_ALLOC(extra_cnt, i64, na * 3 + 1);
    SCRATCH_ALLOC(tri_off, i64, na * 3 + 1);
    SCRATCH_ALLOC(extra_off, i64, na * 3 + 1);
    // vertices: room for one fan centre per (dual, edge) is far too much; sized after the count
    SCRATCH_ALLOC(vtx0, float, na * 3);
    k_contour_vertices<<<grid_for(num_duals, BLK), BLK, 0, s>>>(values, duals, num_duals, positions, threshold,
                                                                voff, poff, active, vtx0, pairs);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(sort_keys(ctx, ctx->scratch, pairs, pairs_sorted, np, 32 + bits_for(num_values + 1)));
    k_adj_splits<<<grid_for(num_values + 1, BLK), BLK, 0, s>>>(pairs_sorted, np, num_values, adj_rs);
    ASR_CHECK_LAUNCH(ctx);
    k_adj_payload<<<grid_for(np, BLK), BLK, 0, s>>>(pairs_sorted, np, adj);
    ASR_CHECK_LAUNCH(ctx);
    k_contour_edges<false><<<grid_for(na * 3 + 1, BLK), BLK, 0, s>>>(values, duals, threshold, active, na, adj_rs,
                                                                     adj, tri_cnt, extra_cnt, nullptr, nullptr,
                                                                     nullptr, nullptr, ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, tri_cnt, tri_off, na * 3 + 1));
    ASR_TRY(scan_counts(ctx, ctx->scratch, extra_cnt, extra_off, na * 3 + 1));
    ASR_TRY(read_i64(ctx, tri_off + na * 3, &st.num_tri));
    ASR_TRY(read_i64(ctx, extra_off + na * 3, &st.num_extra));
    ASR_TRY(read_flags(ctx, host));
    if (host[F_DUAL_FAN])
        ASR_FAIL(ctx, ASR_HIP_ELOGIC, "contour: more than %d dual cells around one edge", ASR_USET_CAP);
    if (na + st.num_extra >= (i64(1) << 31) || st.num_tri >= (i64(1) << 31) / 3)
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "contour: mesh does not fit 32-bit indices");
    st.active = active;
    st.vtx = vtx0;
    st.adj_rs = adj_rs;
    st.adj = adj;
    st.tri_off = tri_off;
    st.extra_off = extra_off;
    *num_vertices = na + st.num_extra;
    *num_triangles = st.num_tri;
    return count_done(ctx, PendingOp::Contour);  // only a count that succeeded may be filled
}

int asr_mesh_contour_fill(asr_hip_context* ctx, float* vertices, int32_t* triangles) {
    if (!fill_begin(ctx, PendingOp::Contour))
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "contour_fill must follow the matching contour_count call");
    const ContourState& st = mstate(ctx).contour;
    const i64 na = st.num_active;
    if (na == 0) return ASR_HIP_OK;
    hipStream_t s = ctx->stream;
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(vertices, st.vtx, (size_t)na * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    k_contour_edges<true><<<grid_for(na * 3, BLK), BLK, 0, s>>>(st.values, st.duals, st.thr, st.active, na,
                                                                st.adj_rs, st.adj, nullptr, nullptr, st.tri_off,
                                                                st.extra_off, vertices, triangles, ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    HostFlags host;
    ASR_TRY(read_flags(ctx, host));
    if (host[F_DUAL_SORT]) ASR_FAIL(ctx, ASR_HIP_ELOGIC, "this should not happen: cannot sort duals (cpp/lib/contouring.cpp:366-370)");
    return ASR_HIP_OK;
}

int asr_mesh_components_count(asr_hip_context* ctx, const float* vertices, i64 nv, const int32_t* triangles,
                              i64 nt, i64 keep_n, i64 min_size, i64* nv_out, i64* nt_out) {
    ASR_TRY(count_begin(ctx));
    ComponentsState& st = mstate(ctx).components;
    st = ComponentsState();
    *nv_out = 0;
    *nt_out = 0;
    if (nv <= 0) return count_done(ctx, PendingOp::Components);
    if (nv >= (i64(1) << 31) || nt >= (i64(1) << 31) / 3)
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "components: mesh does not fit 32-bit indices");
    hipStream_t s = ctx->stream;
    SCRATCH_ALLOC(parent, int, nv);
    SCRATCH_ALLOC(is_root, i64, nv + 1);
    SCRATCH_ALLOC(label, i64, nv + 1);
    SCRATCH_ALLOC(comp, int32_t, nv);
    k_uf_init<<<grid_for(nv, BLK), BLK, 0, s>>>(parent, nv);
    ASR_CHECK_LAUNCH(ctx);
    if (nt > 0) {
        k_uf_link<<<grid_for(nt, BLK), BLK, 0, s>>>(triangles, nt, nv, parent, ctx->d_flags);
        ASR_CHECK_LAUNCH(ctx);
    }
    k_uf_roots<<<grid_for(nv + 1, BLK), BLK, 0, s>>>(parent, nv, is_root);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, is_root, label, nv + 1));
    i64 nc = 0;
    ASR_TRY(read_i64(ctx, label + nv, &nc));
    HostFlags host;
    ASR_TRY(read_flags(ctx, host));
    if (host[F_BAD_INDEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "components: triangle index out of range");
    SCRATCH_ALLOC(sizes, int, nc);
    SCRATCH_ALLOC(keys, u64, nc);
    SCRATCH_ALLOC(keys_sorted, u64, nc);
    SCRATCH_ALLOC(keep, uint8_t, nc);
    ASR_HIP_CHECK(ctx, hipMemsetAsync(sizes, 0, (size_t)nc * sizeof(int), s));
    k_comp_sizes<<<grid_for(nv, BLK), BLK, 0, s>>>(parent, nv, label, comp, sizes);
    ASR_CHECK_LAUNCH(ctx);
    k_comp_keys<<<grid_for(nc, BLK), BLK, 0, s>>>(sizes, nc, keys);
    ASR_CHECK_LAUNCH(ctx);
    {
        size_t tb = 0;
        ASR_HIP_CHECK(ctx, rocprim::radix_sort_keys_desc(nullptr, tb, keys, keys_sorted, (size_t)nc, 0, 64, s));
        void* tmp = ctx->scratch.alloc(tb ? tb : 256);
        if (!tmp) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        ASR_HIP_CHECK(ctx, rocprim::radix_sort_keys_desc(tmp, tb, keys, keys_sorted, (size_t)nc, 0, 64, s));
    }
    k_comp_keep<<<grid_for(nc, BLK), BLK, 0, s>>>(keys_sorted, nc, keep_n, min_size, keep);
    ASR_CHECK_LAUNCH(ctx);
    SCRATCH_ALLOC(vflag, i64, nv + 1);
    SCRATCH_ALLOC(voff, i64, nv + 1);
    SCRATCH_ALLOC(tflag, i64, nt + 1);
    SCRATCH_ALLOC(toff, i64, nt + 1);
    k_vertex_keep<<<grid_for(nv + 1, BLK), BLK, 0, s>>>(comp, keep, nv, vflag);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, vflag, voff, nv + 1));
    k_tri_keep<<<grid_for(nt + 1, BLK), BLK, 0, s>>>(triangles, nt, voff, tflag);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, tflag, toff, nt + 1));
    ASR_TRY(read_i64(ctx, voff + nv, &st.nv_out));
    ASR_TRY(read_i64(ctx, toff + nt, &st.nt_out));
    st.in_vtx = vertices;
    st.in_tri = triangles;
    st.nv = nv;
    st.nt = nt;
    st.v_off = voff;
    st.t_off = toff;
    *nv_out = st.nv_out;
    *nt_out = st.nt_out;
    return count_done(ctx, PendingOp::Components);
}

int asr_mesh_components_fill(asr_hip_context* ctx, float* vertices_out, int32_t* triangles_out) {
    if (!fill_begin(ctx, PendingOp::Components))
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "components_fill must follow the matching components_count call");
    const ComponentsState& st = mstate(ctx).components;
    hipStream_t s = ctx->stream;
    if (st.nv > 0 && st.nv_out > 0) {
        k_compact_vertices<<<grid_for(st.nv, BLK), BLK, 0, s>>>(st.in_vtx, st.nv, st.v_off, vertices_out);
        ASR_CHECK_LAUNCH(ctx);
    }
    if (st.nt > 0 && st.nt_out > 0) {
        k_compact_triangles<<<grid_for(st.nt, BLK), BLK, 0, s>>>(st.in_tri, st.nt, st.v_off, st.t_off,
                                                                 triangles_out);
        ASR_CHECK_LAUNCH(ctx);
    }
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(s));
    return ASR_HIP_OK;
}

int asr_mesh_simplify_count(asr_hip_context* ctx, const asr_octree_frame* frame, const float* vertices, i64 nv,
                            const int32_t* triangles, i64 nt, const int8_t* levels, int level, i64* nv_out, i64* nt_out) {
    ASR_TRY(count_begin(ctx));
    SimplifyState& st = mstate(ctx).simplify;
    st = SimplifyState();
    *nv_out = 0;
    *nt_out = 0;
    if (!levels && (level < 0 || level > ASR_MAX_LEVEL))
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_simplify: level %d is not in 0..%d", level, ASR_MAX_LEVEL);
    if (nv == 0 && nt == 0) return count_done(ctx, PendingOp::MeshSimplify);
    hipStream_t s = ctx->stream;
    const i64 nq = 3 * nt;
    if (nv == 0)  // every corner is out of range
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_simplify: triangle index out of range");
    SCRATCH_ALLOC(keys, u64, nv);
    SCRATCH_ALLOC(ids, int32_t, nv);
    SCRATCH_ALLOC(keys_s, u64, nv);
    SCRATCH_ALLOC(ids_s, int32_t, nv);
    SCRATCH_ALLOC(head, i64, nv + 1);
    SCRATCH_ALLOC(hoff, i64, nv + 1);
    SCRATCH_ALLOC(cluster, int32_t, nv);
    SCRATCH_ALLOC(ckey, u64, nv);
    SCRATCH_ALLOC(cstart, i64, nv + 1);
    k_simp_keys<<<grid_for(nv, BLK), BLK, 0, s>>>(*frame, vertices, nv, levels, level, keys, ids, ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(sort_pairs(ctx, ctx->scratch, keys, keys_s, ids, ids_s, nv, 64));
    k_simp_heads<<<grid_for(nv + 1, BLK), BLK, 0, s>>>(keys_s, nv, head);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, head, hoff, nv + 1));
    k_simp_clusters<<<grid_for(nv + 1, BLK), BLK, 0, s>>>(keys_s, ids_s, nv, hoff, cluster, ckey, cstart);
    ASR_CHECK_LAUNCH(ctx);
    u32 *ck = nullptr, *cv = nullptr, *ck_s = nullptr, *cv_s = nullptr;
    if (nt > 0) {
        ck = arena_alloc<u32>(ctx->scratch, (size_t)nq);
        cv = arena_alloc<u32>(ctx->scratch, (size_t)nq);
        ck_s = arena_alloc<u32>(ctx->scratch, (size_t)nq);
        cv_s = arena_alloc<u32>(ctx->scratch, (size_t)nq);
        if (!ck || !cv || !ck_s || !cv_s) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        k_simp_corner_keys<<<grid_for(nq, BLK), BLK, 0, s>>>(triangles, nq, nv, cluster, ck, cv, ctx->d_flags);
        ASR_CHECK_LAUNCH(ctx);
    }
    i64 nc = 0;
    HostFlags host;
    ASR_TRY(read_i64(ctx, hoff + nv, &nc));
    ASR_TRY(read_flags(ctx, host));
    // nothing below runs on a refused mesh: the kernels that follow index with the corners and shift by the levels
    if (host[F_BAD_LEVEL]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_simplify: a vertex level is not in 0..%d", ASR_MAX_LEVEL);
    if (host[F_OUTSIDE]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_simplify: vertex outside the frame (or not finite)");
    if (host[F_BAD_INDEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_simplify: triangle index out of range");
    st.nv = nv;
    if (nt == 0) return count_done(ctx, PendingOp::MeshSimplify);  // no triangle: no output vertex, vertex_map is all -1
    const int bits = bits_for(nc);
    ASR_TRY(sort_pairs(ctx, ctx->scratch, ck, ck_s, cv, cv_s, nq, bits));
    SCRATCH_ALLOC(kstart, i64, nc + 1);
    SCRATCH_ALLOC(cpos, float, nc * 3);
    k_simp_corner_starts<<<grid_for(nc + 1, BLK), BLK, 0, s>>>(ck_s, nq, nc, kstart);
    ASR_CHECK_LAUNCH(ctx);
    k_simp_solve<<<grid_for(nc * 64, BLK), BLK, 0, s>>>(*frame, vertices, triangles, ids_s, ckey, cstart, cv_s, kstart,
                                                        nc, cpos);
    ASR_CHECK_LAUNCH(ctx);
    // duplicates: the corner buffers are free again (same sizes: 3 nt u32 each)
    u32 *hi = ck, *tid = cv, *tid1 = cv_s, *hi_s = ck_s;
    SCRATCH_ALLOC(lomid, u64, nt);
    SCRATCH_ALLOC(lomid1, u64, nt);
    SCRATCH_ALLOC(lomid2, u64, nt);
    SCRATCH_ALLOC(tid2, u32, nt);
    SCRATCH_ALLOC(tflag, i64, nt + 1);
    SCRATCH_ALLOC(toff, i64, nt + 1);
    SCRATCH_ALLOC(cref, i64, nc + 1);
    SCRATCH_ALLOC(coff, i64, nc + 1);
    k_simp_triples<<<grid_for(nt, BLK), BLK, 0, s>>>(triangles, nt, cluster, bits, hi, lomid, tid);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(sort_pairs(ctx, ctx->scratch, hi, hi_s, tid, tid1, nt, bits));
    k_simp_gather_lomid<<<grid_for(nt, BLK), BLK, 0, s>>>(lomid, tid1, nt, lomid1);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(sort_pairs(ctx, ctx->scratch, lomid1, lomid2, tid1, tid2, nt, 2 * bits));
    k_simp_survivors<<<grid_for(nt + 1, BLK), BLK, 0, s>>>(tid2, lomid2, hi, nt, bits, tflag);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, tflag, toff, nt + 1));
    ASR_HIP_CHECK(ctx, hipMemsetAsync(cref, 0, (size_t)(nc + 1) * sizeof(i64), s));
    k_simp_mark<<<grid_for(nt, BLK), BLK, 0, s>>>(triangles, nt, toff, cluster, cref);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, cref, coff, nc + 1));
    i64 sizes[2] = {0, 0};
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(&sizes[0], coff + nc, sizeof(i64), hipMemcpyDeviceToHost, s));
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(&sizes[1], toff + nt, sizeof(i64), hipMemcpyDeviceToHost, s));
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(s));
    st.in_tri = triangles;
    st.nt = nt;
    st.nc = nc;
    st.cluster = cluster;
    st.cpos = cpos;
    st.c_off = coff;
    st.t_off = toff;
    st.nv_out = *nv_out = sizes[0];
    st.nt_out = *nt_out = sizes[1];
    return count_done(ctx, PendingOp::MeshSimplify);
}

int asr_mesh_simplify_fill(asr_hip_context* ctx, float* vertices_out, int32_t* triangles_out, int32_t* vertex_map) {
    if (!fill_begin(ctx, PendingOp::MeshSimplify))
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_simplify_fill must follow the matching mesh_simplify_count call");
    const SimplifyState& st = mstate(ctx).simplify;
    hipStream_t s = ctx->stream;
    if (st.nv_out > 0) {
        k_simp_out_vertices<<<grid_for(st.nc, BLK), BLK, 0, s>>>(st.cpos, st.nc, st.c_off, vertices_out);
        ASR_CHECK_LAUNCH(ctx);
    }
    if (st.nt_out > 0) {
        k_simp_out_triangles<<<grid_for(st.nt, BLK), BLK, 0, s>>>(st.in_tri, st.nt, st.t_off, st.cluster, st.c_off,
                                                                  triangles_out);
        ASR_CHECK_LAUNCH(ctx);
    }
    if (vertex_map && st.nv > 0) {
        k_simp_vertex_map<<<grid_for(st.nv, BLK), BLK, 0, s>>>(st.cluster, st.c_off, st.nv, vertex_map);
        ASR_CHECK_LAUNCH(ctx);
    }
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(s));
    return ASR_HIP_OK;
}

int asr_mesh_sample(asr_hip_context* ctx, const float* vertices, i64 nv, const int32_t* triangles, i64 nt, i64 num_samples,
                    u64 seed, float* points, float* normals, int32_t* tri) {
    ASR_TRY(ensure_flags(ctx));
    hipStream_t s = ctx->stream;
    double total = 0.0;
    double* prefix = nullptr;
    if (nt > 0) {  // the corner indices are checked whether or not samples are wanted
        ASR_TRY(fresh_flags(ctx));
        SCRATCH_ALLOC(area, double, nt);
        prefix = arena_alloc<double>(ctx->scratch, (size_t)nt);
        if (!prefix) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
        k_tri_areas<<<grid_for(nt, BLK), BLK, 0, s>>>(vertices, nv, triangles, nt, area, ctx->d_flags);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(scan_f64_inclusive(ctx, ctx->scratch, area, prefix, nt));
        ASR_HIP_CHECK(ctx, hipMemcpyAsync(&total, prefix + (nt - 1), sizeof(double), hipMemcpyDeviceToHost, s));
        HostFlags host;
        ASR_TRY(read_flags(ctx, host));
        if (host[F_BAD_INDEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_sample: triangle index out of range");
    }
    if (num_samples == 0) return ASR_HIP_OK;
    if (nt <= 0) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_sample: no triangles to sample");
    if (!(total > 0.0) || !std::isfinite(total))
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_sample: the mesh's area is %g", total);
    k_mesh_sample<<<grid_for(num_samples, BLK), BLK, 0, s>>>(vertices, triangles, nt, prefix, num_samples, seed, points,
                                                              normals, tri);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

namespace {
struct EdgeTable {
    i64 nq = 0;             // sides, an upper bound of the edges
    u64* keys = nullptr;    // sorted side keys [nq]
    i64* start = nullptr;   // [edges + 1] first side of every edge
    i64* count = nullptr;   // the number of edges, on the device
};
// sorts the sides of the triangles and finds the runs; nothing is read back (flags[F_BAD_INDEX]: a corner out of range)
int edge_table(asr_hip_context* ctx, const int32_t* triangles, i64 nt, i64 nv, ull* degenerate, EdgeTable& et) {
    hipStream_t s = ctx->stream;
    const i64 nq = 3 * nt;
    SCRATCH_ALLOC(keys, u64, nq + 1);
    SCRATCH_ALLOC(keys_s, u64, nq);
    i64* head = (i64*)keys;  // the unsorted keys are dead once they are sorted
    SCRATCH_ALLOC(eoff, i64, nq + 1);
    SCRATCH_ALLOC(estart, i64, nq + 1);
    SCRATCH_ALLOC(nvalid, i64, 1);
    if (nq > 0) {
        k_adj_edge_keys<<<grid_for(nq, BLK), BLK, 0, s>>>(triangles, nq, nv, keys, ctx->d_flags, degenerate);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(sort_keys(ctx, ctx->scratch, keys, keys_s, nq, 32 + bits_for(nv + 1)));
    }
    k_adj_edge_heads<<<grid_for(nq + 1, BLK), BLK, 0, s>>>(keys_s, nq, nv, head, nvalid);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, head, eoff, nq + 1));
    k_adj_edge_starts<<<grid_for(nq + 1, BLK), BLK, 0, s>>>(eoff, nq, nvalid, estart);
    ASR_CHECK_LAUNCH(ctx);
    et.nq = nq;
    et.keys = keys_s;
    et.start = estart;
    et.count = eoff + nq;
    return ASR_HIP_OK;
}
// the edge count and the flag block in one wait
int read_count_and_flags(asr_hip_context* ctx, const i64* count, i64* host_count, HostFlags& host_flags) {
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(host_count, count, sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
    return read_flags(ctx, host_flags);
}
}  // namespace

int asr_mesh_edges_count(asr_hip_context* ctx, const int32_t* triangles, i64 nt, i64 nv, i64* num_edges) {
    ASR_TRY(count_begin(ctx));
    EdgesState& st = mstate(ctx).edges;
    st = EdgesState();
    *num_edges = 0;
    if (nt == 0) return count_done(ctx, PendingOp::MeshEdges);
    EdgeTable et;
    ASR_TRY(edge_table(ctx, triangles, nt, nv, nullptr, et));
    i64 ne = 0;
    HostFlags host;
    ASR_TRY(read_count_and_flags(ctx, et.count, &ne, host));
    if (host[F_BAD_INDEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_edges: triangle index out of range");
    st.num_edges = *num_edges = ne;
    st.keys = et.keys;
    st.start = et.start;
    st.count = et.count;
    return count_done(ctx, PendingOp::MeshEdges);
}

int asr_mesh_edges_fill(asr_hip_context* ctx, int32_t* edges, int32_t* uses, int32_t* forward) {
    if (!fill_begin(ctx, PendingOp::MeshEdges))
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_edges_fill must follow the matching mesh_edges_count call");
    const EdgesState& st = mstate(ctx).edges;
    if (st.num_edges > 0 && (edges || uses || forward)) {
        k_adj_edge_out<<<grid_for(st.num_edges, BLK), BLK, 0, ctx->stream>>>(st.keys, st.start, st.count, st.num_edges,
                                                                             edges, uses, forward);
        ASR_CHECK_LAUNCH(ctx);
    }
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ASR_HIP_OK;
}

int asr_mesh_topology_report(asr_hip_context* ctx, const int32_t* triangles, i64 nt, i64 nv, asr_mesh_topology* out) {
    memset(out, 0, sizeof(*out));
    out->num_vertices = nv;
    if (nt == 0) return ASR_HIP_OK;
    ctx->scratch.reset();
    hipStream_t s = ctx->stream;
    ASR_TRY(fresh_flags(ctx));
    SCRATCH_ALLOC(cnt, ull, TOPO_COUNTERS);
    ASR_HIP_CHECK(ctx, hipMemsetAsync(cnt, 0, TOPO_COUNTERS * sizeof(ull), s));
    EdgeTable et;
    ASR_TRY(edge_table(ctx, triangles, nt, nv, &cnt[TOPO_DEGENERATE], et));
    // the number of edges stays on the device: the kernels below are launched for its upper bound, the sides
    const i64 cap = et.nq;
    SCRATCH_ALLOC(edges, int32_t, 2 * cap);
    SCRATCH_ALLOC(uses, int32_t, cap);
    SCRATCH_ALLOC(forward, int32_t, cap);
    k_adj_edge_out<<<grid_for(cap, BLK), BLK, 0, s>>>(et.keys, et.start, et.count, cap, edges, uses, forward);
    ASR_CHECK_LAUNCH(ctx);
    k_adj_topo_edges<<<grid_for(cap, BLK), BLK, 0, s>>>(uses, forward, et.count, cap, cnt);
    ASR_CHECK_LAUNCH(ctx);
    if (nv > 0) {  // (nv == 0: every corner is out of range, refused below)
        SCRATCH_ALLOC(parent_all, int, nv);
        SCRATCH_ALLOC(parent_bnd, int, nv);
        SCRATCH_ALLOC(marks, uint8_t, 2 * nv);
        ASR_HIP_CHECK(ctx, hipMemsetAsync(marks, 0, (size_t)(2 * nv), s));
        k_uf_init<<<grid_for(nv, BLK), BLK, 0, s>>>(parent_all, nv);
        ASR_CHECK_LAUNCH(ctx);
        k_uf_init<<<grid_for(nv, BLK), BLK, 0, s>>>(parent_bnd, nv);
        ASR_CHECK_LAUNCH(ctx);
        k_uf_link_edges<<<grid_for(cap, BLK), BLK, 0, s>>>(edges, uses, et.count, cap, 0, parent_all, marks);
        ASR_CHECK_LAUNCH(ctx);
        k_uf_link_edges<<<grid_for(cap, BLK), BLK, 0, s>>>(edges, uses, et.count, cap, 1, parent_bnd, marks + nv);
        ASR_CHECK_LAUNCH(ctx);
        k_adj_topo_vertices<<<grid_for(nv, BLK), BLK, 0, s>>>(parent_all, marks, parent_bnd, marks + nv, nv, cnt);
        ASR_CHECK_LAUNCH(ctx);
    }
    ull h[TOPO_COUNTERS];
    HostFlags host;
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, s));
    ASR_TRY(read_flags(ctx, host));
    if (host[F_BAD_INDEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_topology: triangle index out of range");
    out->degenerate_triangles = (i64)h[TOPO_DEGENERATE];
    out->triangles = nt - out->degenerate_triangles;
    out->edges = (i64)h[TOPO_EDGES];
    out->boundary_edges = (i64)h[TOPO_BOUNDARY];
    out->nonmanifold_edges = (i64)h[TOPO_NONMANIFOLD];
    out->inconsistent_edges = (i64)h[TOPO_INCONSISTENT];
    out->used_vertices = (i64)h[TOPO_USED];
    out->components = (i64)h[TOPO_COMPONENTS];
    out->boundary_loops = (i64)h[TOPO_LOOPS];
    out->euler = out->used_vertices - out->edges + out->triangles;
    return ASR_HIP_OK;
}

int asr_mesh_smooth(asr_hip_context* ctx, const float* vertices, i64 nv, const int32_t* triangles, i64 nt, int iterations,
                    double lambda, double mu, int boundary, float* vertices_out) {
    ctx->scratch.reset();
    ASR_TRY(fresh_flags(ctx));
    if (nv == 0) {
        if (nt > 0) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_smooth: triangle index out of range");
        return ASR_HIP_OK;
    }
    hipStream_t s = ctx->stream;
    EdgeTable et;
    ASR_TRY(edge_table(ctx, triangles, nt, nv, nullptr, et));
    i64 ne = 0;
    HostFlags host;
    ASR_TRY(read_count_and_flags(ctx, et.count, &ne, host));
    if (host[F_BAD_INDEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_smooth: triangle index out of range");
    // vertex -> neighbour rows: both directions of every edge, sorted; an entry is (neighbour << 1) | feature
    const i64 np = 2 * ne;
    SCRATCH_ALLOC(rs, i64, nv + 1);
    SCRATCH_ALLOC(adj, int32_t, np);
    SCRATCH_ALLOC(vfeat, uint8_t, nv);
    ASR_HIP_CHECK(ctx, hipMemsetAsync(vfeat, 0, (size_t)nv, s));
    if (ne > 0) {
        SCRATCH_ALLOC(edges, int32_t, 2 * ne);
        SCRATCH_ALLOC(uses, int32_t, ne);
        SCRATCH_ALLOC(pairs, u64, np);
        SCRATCH_ALLOC(pairs_s, u64, np);
        k_adj_edge_out<<<grid_for(ne, BLK), BLK, 0, s>>>(et.keys, et.start, et.count, ne, edges, uses, nullptr);
        ASR_CHECK_LAUNCH(ctx);
        k_adj_csr_pairs<<<grid_for(ne, BLK), BLK, 0, s>>>(edges, uses, ne, pairs, vfeat);
        ASR_CHECK_LAUNCH(ctx);
        ASR_TRY(sort_keys(ctx, ctx->scratch, pairs, pairs_s, np, 32 + bits_for(nv)));
        k_adj_splits<<<grid_for(nv + 1, BLK), BLK, 0, s>>>(pairs_s, np, nv, rs);
        ASR_CHECK_LAUNCH(ctx);
        k_adj_payload<<<grid_for(np, BLK), BLK, 0, s>>>(pairs_s, np, adj);
        ASR_CHECK_LAUNCH(ctx);
    } else {
        ASR_HIP_CHECK(ctx, hipMemsetAsync(rs, 0, (size_t)(nv + 1) * sizeof(i64), s));
    }
    // the rows a whole wave sums: at most np / (SMOOTH_CUT + 1) of them
    SCRATCH_ALLOC(lflag, i64, nv + 1);
    SCRATCH_ALLOC(loff, i64, nv + 1);
    SCRATCH_ALLOC(long_rows, int32_t, np / (SMOOTH_CUT + 1) + 1);
    k_smooth_long_flags<<<grid_for(nv + 1, BLK), BLK, 0, s>>>(rs, nv, lflag);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, lflag, loff, nv + 1));
    k_smooth_long_list<<<grid_for(nv, BLK), BLK, 0, s>>>(loff, nv, long_rows);
    ASR_CHECK_LAUNCH(ctx);
    double* pos[2];
    for (double*& p : pos) {
        p = arena_alloc<double>(ctx->scratch, (size_t)nv * 3);
        if (!p) ASR_FAIL(ctx, ASR_HIP_EHIP, "arena allocation failed");
    }
    ASR_TRY(fresh_flags(ctx));
    k_smooth_load<<<grid_for(nv, BLK), BLK, 0, s>>>(vertices, nv, pos[0], ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    i64 nlong = 0;
    ASR_TRY(read_count_and_flags(ctx, loff + nv, &nlong, host));
    if (host[F_BAD_VERTEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_smooth: a vertex is not finite");
    int cur = 0;
    for (int it = 0; it < iterations; ++it)
        for (int half = 0; half < (mu != 0.0 ? 2 : 1); ++half) {
            const double f = half ? mu : lambda;
            k_smooth_step<<<grid_for(nv, BLK), BLK, 0, s>>>(pos[cur], pos[cur ^ 1], nv, rs, adj, vfeat, boundary, f);
            ASR_CHECK_LAUNCH(ctx);
            if (nlong > 0) {
                k_smooth_step_long<<<grid_for(nlong * 64, BLK), BLK, 0, s>>>(pos[cur], pos[cur ^ 1], long_rows, nlong, rs,
                                                                         adj, vfeat, boundary, f);
                ASR_CHECK_LAUNCH(ctx);
            }
            cur ^= 1;
        }
    k_smooth_store<<<grid_for(nv, BLK), BLK, 0, s>>>(pos[cur], nv, vertices_out);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

int asr_mesh_fill_holes_count(asr_hip_context* ctx, const float* vertices, i64 nv, const int32_t* triangles, i64 nt,
                              int max_edges, i64* nv_out, i64* nt_out, asr_mesh_fill_report* report) {
    ASR_TRY(count_begin(ctx));
    FillHolesState& st = mstate(ctx).fill_holes;
    st = FillHolesState();
    memset(report, 0, sizeof(*report));
    *nv_out = nv;
    *nt_out = nt;
    st.in_vtx = vertices;
    st.in_tri = triangles;
    st.nv = st.nv_out = nv;
    st.nt = st.nt_out = nt;
    if (nt == 0) return count_done(ctx, PendingOp::MeshFillHoles);
    if (nv == 0)  // every corner is out of range
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_fill_holes: triangle index out of range");
    hipStream_t s = ctx->stream;
    SCRATCH_ALLOC(cnt, ull, FILL_COUNTERS);
    ASR_HIP_CHECK(ctx, hipMemsetAsync(cnt, 0, FILL_COUNTERS * sizeof(ull), s));
    EdgeTable et;
    ASR_TRY(edge_table(ctx, triangles, nt, nv, nullptr, et));
    // as in the topology report the number of edges stays on the device: launches for its upper bound, the sides
    const i64 cap = et.nq;
    SCRATCH_ALLOC(edges, int32_t, 2 * cap);
    SCRATCH_ALLOC(uses, int32_t, cap);
    SCRATCH_ALLOC(forward, int32_t, cap);
    SCRATCH_ALLOC(parent, int, nv);
    SCRATCH_ALLOC(ints, int, 6 * nv);  // out_deg, in_deg, len, bad, succ, start: zeroed together
    int *out_deg = ints, *in_deg = ints + nv, *len = ints + 2 * nv, *bad = ints + 3 * nv, *succ = ints + 4 * nv,
        *start = ints + 5 * nv;
    SCRATCH_ALLOC(root_of, int, nv);
    SCRATCH_ALLOC(marks, uint8_t, 2 * nv);  // on the boundary; rim id of a filled rim
    uint8_t *on_bnd = marks, *filled_rim = marks + nv;
    SCRATCH_ALLOC(hub_flag, i64, nv + 1);
    SCRATCH_ALLOC(tri_count, i64, nv + 1);
    SCRATCH_ALLOC(long_flag, i64, nv + 1);
    SCRATCH_ALLOC(hub_off, i64, nv + 1);
    SCRATCH_ALLOC(tri_off, i64, nv + 1);
    SCRATCH_ALLOC(long_off, i64, nv + 1);
    SCRATCH_ALLOC(keys, u64, nv);
    SCRATCH_ALLOC(keys_s, u64, nv);
    // a rim with a hub has at least 4 vertices, a long one more than FILL_CUT, and rims share no vertex
    SCRATCH_ALLOC(hub_rims, int32_t, nv / 4 + 1);
    SCRATCH_ALLOC(long_rims, int32_t, nv / (FILL_CUT + 1) + 1);
    ASR_HIP_CHECK(ctx, hipMemsetAsync(ints, 0, (size_t)(6 * nv) * sizeof(int), s));
    ASR_HIP_CHECK(ctx, hipMemsetAsync(marks, 0, (size_t)(2 * nv), s));
    k_adj_edge_out<<<grid_for(cap, BLK), BLK, 0, s>>>(et.keys, et.start, et.count, cap, edges, uses, forward);
    ASR_CHECK_LAUNCH(ctx);
    k_uf_init<<<grid_for(nv, BLK), BLK, 0, s>>>(parent, nv);
    ASR_CHECK_LAUNCH(ctx);
    k_uf_link_edges<<<grid_for(cap, BLK), BLK, 0, s>>>(edges, uses, et.count, cap, 1, parent, on_bnd);
    ASR_CHECK_LAUNCH(ctx);
    k_fill_degrees<<<grid_for(cap, BLK), BLK, 0, s>>>(edges, uses, forward, et.count, cap, out_deg, in_deg, succ);
    ASR_CHECK_LAUNCH(ctx);
    k_fill_rim_stats<<<grid_for(nv, BLK), BLK, 0, s>>>(parent, on_bnd, out_deg, in_deg, nv, root_of, len, bad);
    ASR_CHECK_LAUNCH(ctx);
    k_fill_select<<<grid_for(nv + 1, BLK), BLK, 0, s>>>(on_bnd, root_of, len, bad, nv, max_edges, filled_rim, hub_flag,
                                                        tri_count, long_flag, cnt);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(scan_counts(ctx, ctx->scratch, hub_flag, hub_off, nv + 1));
    ASR_TRY(scan_counts(ctx, ctx->scratch, tri_count, tri_off, nv + 1));
    ASR_TRY(scan_counts(ctx, ctx->scratch, long_flag, long_off, nv + 1));
    k_fill_keys<<<grid_for(nv, BLK), BLK, 0, s>>>(vertices, root_of, filled_rim, nv, keys, ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    ASR_TRY(sort_keys(ctx, ctx->scratch, keys, keys_s, nv, 32 + bits_for(nv + 1)));
    k_fill_starts<<<grid_for(nv, BLK), BLK, 0, s>>>(keys_s, nv, start);
    ASR_CHECK_LAUNCH(ctx);
    k_fill_lists<<<grid_for(nv, BLK), BLK, 0, s>>>(hub_off, long_off, nv, hub_rims, long_rims);
    ASR_CHECK_LAUNCH(ctx);
    // the one read-back: counters, sizes and flags
    ull h[FILL_COUNTERS];
    i64 sizes[3] = {0, 0, 0};
    HostFlags host;
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, s));
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(&sizes[0], hub_off + nv, sizeof(i64), hipMemcpyDeviceToHost, s));
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(&sizes[1], tri_off + nv, sizeof(i64), hipMemcpyDeviceToHost, s));
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(&sizes[2], long_off + nv, sizeof(i64), hipMemcpyDeviceToHost, s));
    ASR_TRY(read_flags(ctx, host));
    if (host[F_BAD_INDEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_fill_holes: triangle index out of range");
    if (host[F_BAD_VERTEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_fill_holes: a vertex of a filled rim is not finite");
    if (nv + sizes[0] >= (i64(1) << 31) || nt + sizes[1] >= (i64(1) << 31) / 3)
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_fill_holes: the filled mesh does not fit 32-bit indices");
    report->rims = (i64)h[FILL_RIMS];
    report->filled = (i64)h[FILL_FILLED];
    report->too_long = (i64)h[FILL_TOO_LONG];
    report->not_simple = (i64)h[FILL_NOT_SIMPLE];
    report->new_vertices = sizes[0];
    report->new_triangles = sizes[1];
    st.nv_out = *nv_out = nv + sizes[0];
    st.nt_out = *nt_out = nt + sizes[1];
    st.rim_vertices = (i64)h[FILL_RIM_VERTICES];
    st.num_long = sizes[2];
    st.keys = keys_s;
    st.len = len;
    st.succ = succ;
    st.start = start;
    st.hub_off = hub_off;
    st.tri_off = tri_off;
    st.hub_rims = hub_rims;
    st.long_rims = long_rims;
    return count_done(ctx, PendingOp::MeshFillHoles);
}

int asr_mesh_fill_holes_fill(asr_hip_context* ctx, float* vertices_out, int32_t* triangles_out) {
    if (!fill_begin(ctx, PendingOp::MeshFillHoles))
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "mesh_fill_holes_fill must follow the matching mesh_fill_holes_count call");
    const FillHolesState& st = mstate(ctx).fill_holes;
    hipStream_t s = ctx->stream;
    if (st.nv > 0)
        ASR_HIP_CHECK(ctx, hipMemcpyAsync(vertices_out, st.in_vtx, (size_t)st.nv * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (st.nt > 0)
        ASR_HIP_CHECK(ctx, hipMemcpyAsync(triangles_out, st.in_tri, (size_t)st.nt * 3 * sizeof(int32_t),
                                          hipMemcpyDeviceToDevice, s));
    const i64 nhubs = st.nv_out - st.nv;
    if (nhubs > 0) {
        float* hubs = vertices_out + 3 * st.nv;
        k_fill_hub<<<grid_for(nhubs, BLK), BLK, 0, s>>>(st.in_vtx, st.keys, st.len, st.start, st.hub_rims, nhubs, hubs);
        ASR_CHECK_LAUNCH(ctx);
        if (st.num_long > 0) {
            k_fill_hub_long<<<grid_for(st.num_long * 64, BLK), BLK, 0, s>>>(st.in_vtx, st.keys, st.len, st.start,
                                                                            st.hub_off, st.long_rims, st.num_long, hubs);
            ASR_CHECK_LAUNCH(ctx);
        }
    }
    if (st.nt_out > st.nt) {
        k_fill_emit<<<grid_for(st.rim_vertices, BLK), BLK, 0, s>>>(st.keys, st.rim_vertices, st.len, st.start, st.succ,
                                                                   st.hub_off, st.tri_off, st.nv, triangles_out + 3 * st.nt);
        ASR_CHECK_LAUNCH(ctx);
    }
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(s));
    return ASR_HIP_OK;
}
