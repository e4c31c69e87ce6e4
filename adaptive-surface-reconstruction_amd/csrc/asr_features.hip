// asr_features.hip -- global registration (contract: include/asr_hip.h; not in the reference):
//   point_fpfh        k_spfh: one wave per point, one lane per slot: the Darboux features of the pair in f64, the three bins,
//                     the 33 counts by ballots (no array indexed by a bin: nothing goes to scratch memory or LDS).
//                     k_fpfh: one wave per point, lane b < 33 owns bin b; the near slots are walked in slot order, a
//                     neighbour's SPFH row is one 132-byte read; the three sub-sums are taken over b ascending by shuffles.
//   feature_match     k_feature_match: brute force.  A tile of b in LDS (rows padded to 16 bytes, read as float4
//                     broadcasts), every thread keeps its own row of a in registers and the key bits(s) << 32 | j by min.
//                     The rows of b are split over blockIdx.y when a has few rows; the parts meet in a 64-bit atomicMin.
//   ransac_transform  k_ransac_gather (the pairs, contiguous), k_ransac_survivors (one thread per hypothesis: draws and
//                     tests; the survivors' numbers are compacted), k_ransac_score (one thread per survivor keeps its
//                     transform in registers and reads tiles of pairs from LDS as broadcasts: no reduction),
//                     k_ransac_best (64-bit atomicMax of score << 32 | ~h), k_ransac_result.
// Compiled with -ffp-contract=off: every expression rounds like its numpy restatement (tests/global_register_ref.py).
#include <cmath>
#include <cstring>

#include "asr_common.h"
#include "asr_prim.h"

namespace {
using namespace asr_prim;

constexpr int BLK = 256;
constexpr int BINS = ASR_FPFH_BINS;
constexpr int FDIM = ASR_FPFH_DIM;
__device__ constexpr double THETA[10][2] = ASR_FPFH_THETA_TABLE;

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}
struct Unit {
    double x, y, z;
    bool ok;
};
// n / sqrt(n . n) of normal i; ok: finite components and n . n > 0
__device__ __forceinline__ Unit unit_normal(const float* __restrict__ nrm, i64 i) {
    const float fx = nrm[3 * i], fy = nrm[3 * i + 1], fz = nrm[3 * i + 2];
    const double x = fx, y = fy, z = fz;
    const double nn = dot3(x, y, z, x, y, z);
    Unit u;
    u.ok = isfinite(fx) && isfinite(fy) && isfinite(fz) && nn > 0.0;
    const double len = sqrt(u.ok ? nn : 1.0);
    u.x = x / len, u.y = y / len, u.z = z / len;
    return u;
}
__device__ __forceinline__ int unit_bin(double f) {
    double b = floor((f + 1.0) * 5.5);
    b = b < 0.0 ? 0.0 : b;
    b = b > 10.0 ? 10.0 : b;
    return (int)b;
}
// what a slot of row i is: j in range and near (the slot counts for the FPFH sum), d = p_j - p_i and d2
struct Slot {
    i64 j;
    double dx, dy, dz, d2, dist;
    Unit uj;
    bool near, bad;
};
__device__ __forceinline__ Slot read_slot(const float* __restrict__ pts, const float* __restrict__ nrm, i64 n,
                                          const int32_t* __restrict__ index, i64 i, int k, int s, bool i_ok) {
    Slot t;
    t.j = 0, t.near = false, t.bad = false;
    t.dx = t.dy = t.dz = t.d2 = t.dist = 0.0;
    t.uj.x = t.uj.y = t.uj.z = 0.0, t.uj.ok = false;
    if (s >= k) return t;
    const i64 j = index[i * k + s];
    if (j == -1) return t;
    if (j < 0 || j >= n) {
        t.bad = true;
        return t;
    }
    t.j = j;
    if (j == i || !i_ok) return t;
    t.uj = unit_normal(nrm, j);
    if (!t.uj.ok) return t;
    t.dx = (double)pts[3 * j] - (double)pts[3 * i];
    t.dy = (double)pts[3 * j + 1] - (double)pts[3 * i + 1];
    t.dz = (double)pts[3 * j + 2] - (double)pts[3 * i + 2];
    t.d2 = dot3(t.dx, t.dy, t.dz, t.dx, t.dy, t.dz);
    t.dist = sqrt(t.d2);
    t.near = t.dist > 0.0 && t.dist < HUGE_VAL;  // (false for NaN)
    return t;
}

__global__ __launch_bounds__(BLK) void k_spfh(const float* __restrict__ pts, const float* __restrict__ nrm, i64 n,
                                              const int32_t* __restrict__ index, int k, float* __restrict__ spfh,
                                              uint8_t* __restrict__ ok_out, int* flags) {
    const int lane = threadIdx.x & 63;
    const i64 i = (i64)blockIdx.x * (BLK / 64) + (threadIdx.x >> 6);
    if (i >= n) return;  // (the whole wave)
    const Unit ui = unit_normal(nrm, i);
    const Slot t = read_slot(pts, nrm, n, index, i, k, lane, ui.ok);
    if (__ballot(t.bad) && lane == 0) atomicOr(&flags[F_BAD_INDEX], 1);  // the call fails; nothing bad was followed
    bool valid = false;
    int bt = 0, ba = 0, bp = 0;
    if (t.near) {
        const double a1 = dot3(ui.x, ui.y, ui.z, t.dx, t.dy, t.dz);
        const double a2 = dot3(t.uj.x, t.uj.y, t.uj.z, t.dx, t.dy, t.dz);
        const bool swap = fabs(a1) < fabs(a2);
        const double ux = swap ? t.uj.x : ui.x, uy = swap ? t.uj.y : ui.y, uz = swap ? t.uj.z : ui.z;
        const double tx = swap ? ui.x : t.uj.x, ty = swap ? ui.y : t.uj.y, tz = swap ? ui.z : t.uj.z;
        const double ex = swap ? -t.dx : t.dx, ey = swap ? -t.dy : t.dy, ez = swap ? -t.dz : t.dz;
        const double phi = (swap ? -a2 : a1) / t.dist;
        const double cx = ey * uz - ez * uy, cy = ez * ux - ex * uz, cz = ex * uy - ey * ux;
        const double cn = sqrt(dot3(cx, cy, cz, cx, cy, cz));
        if (cn > 0.0) {
            valid = true;
            const double vx = cx / cn, vy = cy / cn, vz = cz / cn;
            const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
            const double alpha = dot3(vx, vy, vz, tx, ty, tz);
            const double x = dot3(ux, uy, uz, tx, ty, tz);
            const double y = dot3(wx, wy, wz, tx, ty, tz);
            const bool upper = y >= 0.0;
#pragma unroll
            for (int b = 1; b < BINS; ++b) {
                const bool turned = (y * THETA[b - 1][0] - x * THETA[b - 1][1]) >= 0.0;
                bt += (b <= 5 ? (upper || turned) : (upper && turned)) ? 1 : 0;
            }
            ba = unit_bin(alpha);
            bp = unit_bin(phi);
        }
    }
    const int m = __popcll(__ballot(valid));
    int count = 0;  // of bin `lane`
#pragma unroll
    for (int b = 0; b < BINS; ++b) {
        const int ct = __popcll(__ballot(valid && bt == b));
        const int ca = __popcll(__ballot(valid && ba == b));
        const int cp = __popcll(__ballot(valid && bp == b));
        count = lane == b ? ct : lane == BINS + b ? ca : lane == 2 * BINS + b ? cp : count;
    }
    if (lane < FDIM) spfh[i * FDIM + lane] = m > 0 ? (float)((100.0 * (double)count) / (double)m) : 0.f;
    if (lane == 0 && ok_out) ok_out[i] = (ui.ok && m > 0) ? 1 : 0;
}

__global__ __launch_bounds__(BLK) void k_fpfh(const float* __restrict__ pts, const float* __restrict__ nrm, i64 n,
                                              const int32_t* __restrict__ index, int k, const float* __restrict__ spfh,
                                              float* __restrict__ fpfh) {
    const int lane = threadIdx.x & 63;
    const i64 i = (i64)blockIdx.x * (BLK / 64) + (threadIdx.x >> 6);
    if (i >= n) return;  // (the whole wave)
    const Unit ui = unit_normal(nrm, i);
    const Slot t = read_slot(pts, nrm, n, index, i, k, lane, ui.ok);
    const int bin = lane < FDIM ? lane : FDIM - 1;
    double acc = 0.0;
    for (u64 mask = __ballot(t.near); mask; mask &= mask - 1) {  // (the same in every lane) ascending slots
        const int s = __ffsll((long long)mask) - 1;
        const i64 j = __shfl((int)t.j, s);
        const double d2 = __shfl(t.d2, s);
        acc = acc + (double)spfh[j * FDIM + bin] / d2;
    }
    const int first = (bin / BINS) * BINS;
    double total = 0.0;
#pragma unroll
    for (int b = 0; b < BINS; ++b) total = total + __shfl(acc, first + b);
    const double scaled = total > 0.0 ? (100.0 * acc) / total : 0.0;
    if (lane < FDIM) fpfh[i * FDIM + lane] = ui.ok ? (float)(scaled + (double)spfh[i * FDIM + lane]) : 0.f;
}

// ------------------------------------------------------------------------------------------
// feature_match
// ------------------------------------------------------------------------------------------
constexpr int MATCH_TILE = ASR_FEATURE_MATCH_TILE;
__global__ void k_rows_finite(const float* __restrict__ rows, i64 n, int dim, uint8_t* __restrict__ ok) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    bool good = true;
    for (int c = 0; c < dim; ++c) good = good && isfinite(rows[r * dim + c]);
    ok[r] = good ? 1 : 0;
}
// MAXD: the row length the registers are laid out for; EXACT: dim == MAXD (else dim < MAXD at run time).  Rows of b that
// are not usable arrive in LDS as NaN rows: their s is NaN, whose key lies above that of every number.
template <int MAXD, bool EXACT>
__global__ __launch_bounds__(BLK) void k_feature_match(const float* __restrict__ a, i64 m, const float* __restrict__ b, i64 n,
                                                       int dim_rt, const uint8_t* __restrict__ b_ok, i64 rows_per_part,
                                                       u64* __restrict__ keys, int parts) {
    constexpr int STRIDE4 = (MAXD + 3) / 4;
    __shared__ float4 tile4[MATCH_TILE * STRIDE4];
    float* tile = reinterpret_cast<float*>(tile4);
    const int dim = EXACT ? MAXD : dim_rt;
    const i64 row = (i64)blockIdx.x * BLK + threadIdx.x;
    float ar[MAXD];
#pragma unroll
    for (int c = 0; c < MAXD; ++c) ar[c] = (row < m && c < dim) ? a[row * dim + c] : 0.f;
    u64 best = ~u64(0);
    const i64 j0 = (i64)blockIdx.y * rows_per_part;
    const i64 j1 = j0 + rows_per_part < n ? j0 + rows_per_part : n;
    for (i64 base = j0; base < j1; base += MATCH_TILE) {
        const int cnt = (int)(j1 - base < MATCH_TILE ? j1 - base : MATCH_TILE);
        __syncthreads();  // the tile of the round before has been read
        for (int e = threadIdx.x; e < cnt * dim; e += BLK) {
            const int r = e / dim, c = e - r * dim;
            tile[r * (STRIDE4 * 4) + c] = b_ok[base + r] ? b[(base + r) * dim + c] : __uint_as_float(0x7fc00000u);
        }
        __syncthreads();
        for (int r = 0; r < cnt; ++r) {
            const float4* row4 = tile4 + r * STRIDE4;
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < STRIDE4; ++q) {
                const float4 v = row4[q];
                if (4 * q < dim) {
                    const float t = ar[4 * q] - v.x;
                    s = s + t * t;
                }
                if (4 * q + 1 < MAXD && 4 * q + 1 < dim) {
                    const float t = ar[4 * q + 1 < MAXD ? 4 * q + 1 : 0] - v.y;
                    s = s + t * t;
                }
                if (4 * q + 2 < MAXD && 4 * q + 2 < dim) {
                    const float t = ar[4 * q + 2 < MAXD ? 4 * q + 2 : 0] - v.z;
                    s = s + t * t;
                }
                if (4 * q + 3 < MAXD && 4 * q + 3 < dim) {
                    const float t = ar[4 * q + 3 < MAXD ? 4 * q + 3 : 0] - v.w;
                    s = s + t * t;
                }
            }
            const u64 key = ((u64)__float_as_uint(s) << 32) | (u64)(u32)(base + r);
            best = key < best ? key : best;
        }
    }
    if (row >= m) return;
    if (parts > 1)
        atomicMin((unsigned long long*)&keys[row], (unsigned long long)best);
    else
        keys[row] = best;
}
__global__ void k_match_decode(const u64* __restrict__ keys, const float* __restrict__ a, i64 m, int dim,
                               int32_t* __restrict__ index_out, float* __restrict__ sq_out) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    bool good = true;
    for (int c = 0; c < dim; ++c) good = good && isfinite(a[r * dim + c]);
    const u64 key = keys[r];
    const float s = __uint_as_float((u32)(key >> 32));
    good = good && s == s;  // NaN: no usable row of b
    if (index_out) index_out[r] = good ? (int32_t)(u32)key : -1;
    if (sq_out) sq_out[r] = good ? s : __uint_as_float(0x7f800000u);
}

// ------------------------------------------------------------------------------------------
// ransac_transform
// ------------------------------------------------------------------------------------------
constexpr int PAIR_TILE = 256;
struct RansacDevice {
    u64 best;  // score << 32 | ~h
    int survivors;
    int bad;
    double transform[12];
};
// pair i: (source point, 1) and (target point, 1), or NaN points and 0 when a point is not finite or a row out of range
__global__ void k_ransac_gather(const float* __restrict__ src, i64 m, const float* __restrict__ tgt, i64 n,
                                const int32_t* __restrict__ corr, i64 c, float4* __restrict__ S, float4* __restrict__ T,
                                RansacDevice* res) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c) return;
    const i64 si = corr[2 * i], ti = corr[2 * i + 1];
    const float nan = __uint_as_float(0x7fc00000u);
    float4 s = make_float4(nan, nan, nan, 0.f), t = s;
    if (si < 0 || si >= m || ti < 0 || ti >= n) {
        atomicOr(&res->bad, 1);
    } else {
        const float sx = src[3 * si], sy = src[3 * si + 1], sz = src[3 * si + 2];
        const float tx = tgt[3 * ti], ty = tgt[3 * ti + 1], tz = tgt[3 * ti + 2];
        if (isfinite(sx) && isfinite(sy) && isfinite(sz) && isfinite(tx) && isfinite(ty) && isfinite(tz))
            s = make_float4(sx, sy, sz, 1.f), t = make_float4(tx, ty, tz, 1.f);
    }
    S[i] = s;
    T[i] = t;
}
__device__ __forceinline__ i64 ransac_draw(u64 seed, u64 h, u64 r, u64 c) {
    u64 z = seed + (3 * h + r + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (i64)(((z >> 32) * c) >> 32);
}
struct Frame {
    double e1x, e1y, e1z, e2x, e2y, e2z, e3x, e3y, e3z;
    bool good;
};
__device__ __forceinline__ Frame ransac_frame(float4 p0, float4 p1, float4 p2) {
    const double ax = (double)p1.x - (double)p0.x, ay = (double)p1.y - (double)p0.y, az = (double)p1.z - (double)p0.z;
    const double bx = (double)p2.x - (double)p0.x, by = (double)p2.y - (double)p0.y, bz = (double)p2.z - (double)p0.z;
    const double la = sqrt(dot3(ax, ay, az, ax, ay, az));
    Frame f;
    f.e1x = ax / la, f.e1y = ay / la, f.e1z = az / la;
    const double gx = f.e1y * bz - f.e1z * by, gy = f.e1z * bx - f.e1x * bz, gz = f.e1x * by - f.e1y * bx;
    const double lg = sqrt(dot3(gx, gy, gz, gx, gy, gz));
    f.e3x = gx / lg, f.e3y = gy / lg, f.e3z = gz / lg;
    f.e2x = f.e3y * f.e1z - f.e3z * f.e1y, f.e2y = f.e3z * f.e1x - f.e3x * f.e1z, f.e2z = f.e3x * f.e1y - f.e3y * f.e1x;
    f.good = la > 0.0 && lg > 0.0;
    return f;
}
__device__ __forceinline__ double edge_length(float4 p, float4 q) {
    const double x = (double)q.x - (double)p.x, y = (double)q.y - (double)p.y, z = (double)q.z - (double)p.z;
    return sqrt(dot3(x, y, z, x, y, z));
}
struct Rigid {
    double r00, r01, r02, t0, r10, r11, r12, t1, r20, r21, r22, t2;
};
// hypothesis h: false when it is rejected, else its transform
__device__ __forceinline__ bool ransac_hypothesis(const float4* __restrict__ S, const float4* __restrict__ T, i64 c, u64 seed,
                                                  i64 h, double ratio, Rigid& x) {
    const i64 d0 = ransac_draw(seed, (u64)h, 0, (u64)c), d1 = ransac_draw(seed, (u64)h, 1, (u64)c),
              d2 = ransac_draw(seed, (u64)h, 2, (u64)c);
    if (d0 == d1 || d0 == d2 || d1 == d2) return false;
    const float4 s0 = S[d0], s1 = S[d1], s2 = S[d2], t0 = T[d0], t1 = T[d1], t2 = T[d2];
    if (s0.w == 0.f || s1.w == 0.f || s2.w == 0.f) return false;
    double ls = edge_length(s0, s1), lt = edge_length(t0, t1);
    bool good = ls >= ratio * lt && lt >= ratio * ls;
    ls = edge_length(s0, s2), lt = edge_length(t0, t2);
    good = good && ls >= ratio * lt && lt >= ratio * ls;
    ls = edge_length(s1, s2), lt = edge_length(t1, t2);
    good = good && ls >= ratio * lt && lt >= ratio * ls;
    if (!good) return false;
    const Frame fs = ransac_frame(s0, s1, s2), ft = ransac_frame(t0, t1, t2);
    if (!fs.good || !ft.good) return false;
    x.r00 = (ft.e1x * fs.e1x + ft.e2x * fs.e2x) + ft.e3x * fs.e3x;
    x.r01 = (ft.e1x * fs.e1y + ft.e2x * fs.e2y) + ft.e3x * fs.e3y;
    x.r02 = (ft.e1x * fs.e1z + ft.e2x * fs.e2z) + ft.e3x * fs.e3z;
    x.r10 = (ft.e1y * fs.e1x + ft.e2y * fs.e2x) + ft.e3y * fs.e3x;
    x.r11 = (ft.e1y * fs.e1y + ft.e2y * fs.e2y) + ft.e3y * fs.e3y;
    x.r12 = (ft.e1y * fs.e1z + ft.e2y * fs.e2z) + ft.e3y * fs.e3z;
    x.r20 = (ft.e1z * fs.e1x + ft.e2z * fs.e2x) + ft.e3z * fs.e3x;
    x.r21 = (ft.e1z * fs.e1y + ft.e2z * fs.e2y) + ft.e3z * fs.e3y;
    x.r22 = (ft.e1z * fs.e1z + ft.e2z * fs.e2z) + ft.e3z * fs.e3z;
    const double sx = s0.x, sy = s0.y, sz = s0.z;
    x.t0 = (double)t0.x - ((x.r00 * sx + x.r01 * sy) + x.r02 * sz);
    x.t1 = (double)t0.y - ((x.r10 * sx + x.r11 * sy) + x.r12 * sz);
    x.t2 = (double)t0.z - ((x.r20 * sx + x.r21 * sy) + x.r22 * sz);
    return true;
}
// the numbers of the hypotheses that pass, in no particular order (every later step carries h along)
__global__ __launch_bounds__(BLK) void k_ransac_survivors(const float4* __restrict__ S, const float4* __restrict__ T, i64 c,
                                                          u64 seed, i64 num, double ratio, int32_t* __restrict__ list,
                                                          RansacDevice* res) {
    const i64 h = (i64)blockIdx.x * BLK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    Rigid x;
    const bool pass = h < num && ransac_hypothesis(S, T, c, seed, h, ratio, x);
    const u64 mask = __ballot(pass);
    if (!mask) return;  // (the whole wave)
    const int leader = __ffsll((long long)mask) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&res->survivors, __popcll(mask));
    base = __shfl(base, leader);
    if (pass) list[base + __popcll(mask & ((u64(1) << lane) - 1))] = (int32_t)h;
}
__global__ __launch_bounds__(BLK) void k_ransac_score(const float4* __restrict__ S, const float4* __restrict__ T, i64 c, u64 seed,
                                                      double ratio, const int32_t* __restrict__ list, int survivors,
                                                      float cap2, i64 pairs_per_part, int parts, int* __restrict__ counts) {
    __shared__ float4 s_src[PAIR_TILE];
    __shared__ float4 s_tgt[PAIR_TILE];
    const int e = blockIdx.x * BLK + threadIdx.x;
    Rigid x;
    // (a survivor passes again: the same function of the same inputs)
    const bool live = e < survivors && ransac_hypothesis(S, T, c, seed, list[e < survivors ? e : 0], ratio, x);
    if (!live) x.r00 = x.r01 = x.r02 = x.t0 = x.r10 = x.r11 = x.r12 = x.t1 = x.r20 = x.r21 = x.r22 = x.t2 = 0.0;
    int count = 0;
    const i64 c0 = (i64)blockIdx.y * pairs_per_part;
    const i64 c1 = c0 + pairs_per_part < c ? c0 + pairs_per_part : c;
    for (i64 base = c0; base < c1; base += PAIR_TILE) {
        const int cnt = (int)(c1 - base < PAIR_TILE ? c1 - base : PAIR_TILE);
        __syncthreads();  // the tile of the round before has been read
        if ((int)threadIdx.x < cnt) {
            s_src[threadIdx.x] = S[base + threadIdx.x];
            s_tgt[threadIdx.x] = T[base + threadIdx.x];
        }
        __syncthreads();
        for (int r = 0; r < cnt; ++r) {
            const float4 p = s_src[r], y = s_tgt[r];
            const double px = p.x, py = p.y, pz = p.z;
            const float qx = (float)(((x.r00 * px + x.r01 * py) + x.r02 * pz) + x.t0);
            const float qy = (float)(((x.r10 * px + x.r11 * py) + x.r12 * pz) + x.t1);
            const float qz = (float)(((x.r20 * px + x.r21 * py) + x.r22 * pz) + x.t2);
            const float dx = qx - y.x, dy = qy - y.y, dz = qz - y.z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            count += d2 <= cap2 ? 1 : 0;  // (false for the NaN of a pair that is not finite)
        }
    }
    if (!live) return;
    if (parts > 1)
        atomicAdd(&counts[e], count);
    else
        counts[e] = count;
}
__global__ void k_ransac_best(const int32_t* __restrict__ list, const int* __restrict__ counts, int survivors,
                              RansacDevice* res) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= survivors) return;
    const u64 key = ((u64)(u32)counts[e] << 32) | (u64)(~(u32)list[e]);
    atomicMax((unsigned long long*)&res->best, (unsigned long long)key);
}
__global__ void k_ransac_result(const float4* __restrict__ S, const float4* __restrict__ T, i64 c, u64 seed, double ratio,
                                RansacDevice* res) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Rigid x;
    const i64 h = (i64)(~(u32)res->best);
    if (!ransac_hypothesis(S, T, c, seed, h, ratio, x)) return;
    double* t = res->transform;
    t[0] = x.r00, t[1] = x.r01, t[2] = x.r02, t[3] = x.t0;
    t[4] = x.r10, t[5] = x.r11, t[6] = x.r12, t[7] = x.t1;
    t[8] = x.r20, t[9] = x.r21, t[10] = x.r22, t[11] = x.t2;
}

// parts of a loop of `tiles` tiles for `blocks` workgroups in x: enough of them to fill the device, never an empty one
void split_tiles(i64 tiles, i64 blocks, i64& tiles_per_part, int& parts) {
    i64 want = 512 / (blocks > 0 ? blocks : 1);
    if (want < 1) want = 1;
    if (want > tiles) want = tiles;
    tiles_per_part = (tiles + want - 1) / want;
    parts = (int)((tiles + tiles_per_part - 1) / tiles_per_part);
}
}  // namespace

// asr_hip_point_fpfh: two launches and one read-back (the index check); arguments validated by the caller
int asr_features_fpfh(asr_hip_context* ctx, const float* points, const float* normals, i64 n, const int32_t* index, int k,
                      float* fpfh_out, float* spfh_out, uint8_t* ok_out) {
    ctx->scratch.reset();
    if (n == 0) return ASR_HIP_OK;
    ASR_TRY(fresh_flags(ctx));
    float* spfh = spfh_out;
    if (!spfh) {
        SCRATCH_ALLOC(tmp, float, n * FDIM);
        spfh = tmp;
    }
    const unsigned grid = grid_for(n, BLK / 64);
    k_spfh<<<grid, BLK, 0, ctx->stream>>>(points, normals, n, index, k, spfh, ok_out, ctx->d_flags);
    ASR_CHECK_LAUNCH(ctx);
    k_fpfh<<<grid, BLK, 0, ctx->stream>>>(points, normals, n, index, k, spfh, fpfh_out);  // (follows no bad index either)
    ASR_CHECK_LAUNCH(ctx);
    HostFlags host;
    ASR_TRY(read_flags(ctx, host));
    if (host[F_BAD_INDEX]) ASR_FAIL(ctx, ASR_HIP_EINVAL, "point_fpfh: a neighbour index is neither -1 nor in [0, n)");
    return ASR_HIP_OK;
}

// asr_hip_feature_match; arguments validated by the caller
int asr_features_match(asr_hip_context* ctx, const float* a, i64 m, const float* b, i64 n, int dim, int32_t* index_out,
                       float* sqdist_out) {
    ctx->scratch.reset();
    if (m == 0 || (!index_out && !sqdist_out)) return ASR_HIP_OK;
    hipStream_t s = ctx->stream;
    SCRATCH_ALLOC(b_ok, uint8_t, n);
    SCRATCH_ALLOC(keys, u64, m);
    k_rows_finite<<<grid_for(n, BLK), BLK, 0, s>>>(b, n, dim, b_ok);
    ASR_CHECK_LAUNCH(ctx);
    const i64 blocks = (m + BLK - 1) / BLK, tiles = (n + MATCH_TILE - 1) / MATCH_TILE;
    i64 tiles_per_part;
    int parts;
    split_tiles(tiles, blocks, tiles_per_part, parts);
    if (parts > 1) ASR_HIP_CHECK(ctx, hipMemsetAsync(keys, 0xff, (size_t)m * sizeof(u64), s));
    const dim3 grid((unsigned)blocks, (unsigned)parts);
    const i64 rows = tiles_per_part * MATCH_TILE;
    if (dim == FDIM)
        k_feature_match<FDIM, true><<<grid, BLK, 0, s>>>(a, m, b, n, dim, b_ok, rows, keys, parts);
    else if (dim <= 16)
        k_feature_match<16, false><<<grid, BLK, 0, s>>>(a, m, b, n, dim, b_ok, rows, keys, parts);
    else
        k_feature_match<64, false><<<grid, BLK, 0, s>>>(a, m, b, n, dim, b_ok, rows, keys, parts);
    ASR_CHECK_LAUNCH(ctx);
    k_match_decode<<<grid_for(m, BLK), BLK, 0, s>>>(keys, a, m, dim, index_out, sqdist_out);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

// asr_hip_ransac_transform; arguments validated by the caller.  1: no hypothesis passed (the error text stays empty)
int asr_features_ransac(asr_hip_context* ctx, const float* source, i64 m, const float* target, i64 n, const int32_t* corr,
                        i64 c, const asr_ransac_params* params, double transform_out[12], asr_ransac_report* report) {
    ctx->scratch.reset();
    report->evaluated = 0, report->best_hypothesis = -1, report->inliers = 0;
    hipStream_t s = ctx->stream;
    const i64 num = params->num_hypotheses;
    SCRATCH_ALLOC(res, RansacDevice, 1);
    SCRATCH_ALLOC(S, float4, c);
    SCRATCH_ALLOC(T, float4, c);
    SCRATCH_ALLOC(list, int32_t, num);
    ASR_HIP_CHECK(ctx, hipMemsetAsync(res, 0, sizeof(RansacDevice), s));
    k_ransac_gather<<<grid_for(c, BLK), BLK, 0, s>>>(source, m, target, n, corr, c, S, T, res);
    ASR_CHECK_LAUNCH(ctx);
    k_ransac_survivors<<<grid_for(num, BLK), BLK, 0, s>>>(S, T, c, params->seed, num, params->edge_ratio, list, res);
    ASR_CHECK_LAUNCH(ctx);
    RansacDevice host;
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(&host, res, sizeof(host), hipMemcpyDeviceToHost, s));
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(s));
    if (host.bad) ASR_FAIL(ctx, ASR_HIP_EINVAL, "ransac_transform: a correspondence names a row outside its cloud");
    if (host.survivors < 0 || host.survivors > num) ASR_FAIL(ctx, ASR_HIP_ELOGIC, "ransac_transform: survivor count");
    if (host.survivors == 0) return 1;
    const int survivors = host.survivors;
    SCRATCH_ALLOC(counts, int, survivors);
    const i64 blocks = (survivors + BLK - 1) / BLK, tiles = (c + PAIR_TILE - 1) / PAIR_TILE;
    i64 tiles_per_part;
    int parts;
    split_tiles(tiles, blocks, tiles_per_part, parts);
    if (parts > 1) ASR_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, (size_t)survivors * sizeof(int), s));
    const float cap2 = params->max_distance * params->max_distance;
    k_ransac_score<<<dim3((unsigned)blocks, (unsigned)parts), BLK, 0, s>>>(S, T, c, params->seed, params->edge_ratio, list,
                                                                          survivors, cap2, tiles_per_part * PAIR_TILE, parts,
                                                                          counts);
    ASR_CHECK_LAUNCH(ctx);
    k_ransac_best<<<grid_for(survivors, BLK), BLK, 0, s>>>(list, counts, survivors, res);
    ASR_CHECK_LAUNCH(ctx);
    k_ransac_result<<<1, 64, 0, s>>>(S, T, c, params->seed, params->edge_ratio, res);
    ASR_CHECK_LAUNCH(ctx);
    ASR_HIP_CHECK(ctx, hipMemcpyAsync(&host, res, sizeof(host), hipMemcpyDeviceToHost, s));
    ASR_HIP_CHECK(ctx, hipStreamSynchronize(s));
    report->evaluated = survivors;
    report->best_hypothesis = (i64)(~(u32)host.best);
    report->inliers = (i64)(host.best >> 32);
    for (int i = 0; i < 12; ++i) transform_out[i] = host.transform[i];
    return ASR_HIP_OK;
}
