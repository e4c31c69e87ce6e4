// asr_query.hip -- the implicit field at arbitrary points (UNet5.decode / decode_with_gradient,
// models/v0/net_definitions_torch.py:655-686, at shifts other than zero):
//   leaf location: point -> row of the grid-0 leaf that contains it (Octree::ComputeCoord, cpp/lib/octree.h:49-66)
//   decoder at shifts: [s | code] -> h1 -> ReLU -> h2 -> ReLU -> 2, optionally with d value[:,0] / d s
//   whole-path query: location, code gather and decoder in one pass over the queries
// Compiled with -ffp-contract=off (GEOM_FLAGS) so that the location rounds exactly like asr_hip_point_keys; the
// decoder's matrix-core chain is explicit builtins and does not depend on contraction.
#include "asr_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int QDEC_MAX = 64;  // generic widths: the forward decoder's limit (asr_conv.hip DEC_MAX)

struct QueryArgs {
    // decoder: w1 [h1, 3+c], b1 [h1], w2 [h2, h1], b2 [h2], w3 [2, h2]
    const float* code;
    int c, h1, h2;
    const float *w1, *b1, *w2, *b2, *w3;
    i64 m;
    // decode_mlp_at: code row per query (null: the query's index) and its shift [m, 3]
    const int32_t* rows;
    const float* shifts;
    // implicit_query: the leaf set (sorted keys, centres, sizes) and the positions [m, 3]
    asr_octree_frame frame;
    const u64* keys;
    i64 nleaves;
    const float* centers;
    const float* sizes;
    const float* pos;
    // per row: values[:, 0] *= vsize[row] (null: no sdf scale), grad /= gsize[row] (null: none)
    const float* vsize;
    const float* gsize;
    float* values;    // [m, 2]
    float* grad;      // [m, 3] or null
    int32_t* rows_out;  // [m] or null
};

__device__ inline i64 lower_bound_u64(const u64* __restrict__ keys, i64 lo, i64 hi, u64 k) {
    while (lo < hi) {
        const i64 mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Level runs of a sorted leaf set into run[0 .. 22]: the leaves of level l are rows [run[l], run[l+1]), because every
// level-l key lies in [8^l, 8^(l+1)).  Every thread of the block takes part (one __syncthreads).  On an unsorted
// input the runs are wrong but every index stays inside [0, n].
__device__ inline void level_runs(const u64* __restrict__ keys, i64 n, i64* run) {
    const int t = threadIdx.x;
    if (t <= ASR_MAX_LEVEL) run[t] = lower_bound_u64(keys, 0, n, u64(1) << (3 * t));
    if (t == ASR_MAX_LEVEL + 1) run[t] = n;
    __syncthreads();
}

// row of the leaf that contains the point, or -1: walks the levels from the coarsest to the finest and stops at the
// first level whose run holds the point's key of that level (binary search in the run)
__device__ inline int32_t locate(const asr_octree_frame& f, const u64* __restrict__ keys, const i64* run, float px,
                                 float py, float pz) {
    int x, y, z;
    if (!frame_coord21_checked(f, px, py, pz, x, y, z)) return -1;
    for (int l = 0; l <= ASR_MAX_LEVEL; ++l) {
        const i64 lo = run[l], hi = run[l + 1];
        if (lo >= hi) continue;
        const int s = ASR_MAX_LEVEL - l;
        const u64 k = asr_coord_key(x >> s, y >> s, z >> s, l);
        const i64 i = lower_bound_u64(keys, lo, hi, k);
        if (i < hi && keys[i] == k) return (int32_t)i;
    }
    return -1;
}

__global__ __launch_bounds__(256) void k_leaf_locate(asr_octree_frame f, const u64* __restrict__ keys, i64 n,
                                                     const float* __restrict__ pos, i64 m, int32_t* __restrict__ rows) {
    __shared__ i64 s_run[ASR_MAX_LEVEL + 2];
    level_runs(keys, n, s_run);
    for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < m; q += (i64)gridDim.x * blockDim.x)
        rows[q] = locate(f, keys, s_run, pos[3 * q], pos[3 * q + 1], pos[3 * q + 2]);
}

// one query's row and shift: located (LOCATE) or given
template <bool LOCATE>
__device__ inline int32_t query_row(const QueryArgs& a, const i64* run, i64 q, float& sx, float& sy, float& sz) {
    sx = sy = sz = 0.f;
    if (LOCATE) {
        const float px = a.pos[3 * q], py = a.pos[3 * q + 1], pz = a.pos[3 * q + 2];
        const int32_t row = locate(a.frame, a.keys, run, px, py, pz);
        if (a.rows_out) a.rows_out[q] = row;
        if (row >= 0) {  // s = (p - centre) / size: exactly 0 at a centre
            const float size = a.sizes[row];
            sx = (px - a.centers[3 * (i64)row]) / size;
            sy = (py - a.centers[3 * (i64)row + 1]) / size;
            sz = (pz - a.centers[3 * (i64)row + 2]) / size;
        }
        return row;
    }
    const int32_t row = a.rows ? a.rows[q] : (int32_t)q;
    sx = a.shifts[3 * q];
    sy = a.shifts[3 * q + 1];
    sz = a.shifts[3 * q + 2];
    return row;
}

// Generic widths (c, h1, h2 <= 64): thread per query, weights staged in LDS (k_decode with the shift columns kept) and
// the backward pass of decode_with_gradient: z3 = w3[0] * [f2 > 0], z2 = (z3 . W2) * [f1 > 0], grad = z2 . W1[:, :3].
template <bool LOCATE>
__global__ __launch_bounds__(256) void k_decode_at(QueryArgs a) {
    const int c = a.c, h1 = a.h1, h2 = a.h2, c3 = 3 + a.c;
    extern __shared__ float s_w[];
    __shared__ i64 s_run[ASR_MAX_LEVEL + 2];
    float* sw1 = s_w;             // [h1][3+c]
    float* sb1 = sw1 + h1 * c3;   // [h1]
    float* sw2 = sb1 + h1;        // [h2][h1]
    float* sb2 = sw2 + h2 * h1;   // [h2]
    float* sw3 = sb2 + h2;        // [2][h2]
    for (int i = threadIdx.x; i < h1 * c3; i += blockDim.x) sw1[i] = a.w1[i];
    for (int i = threadIdx.x; i < h1; i += blockDim.x) sb1[i] = a.b1[i];
    for (int i = threadIdx.x; i < h2 * h1; i += blockDim.x) sw2[i] = a.w2[i];
    for (int i = threadIdx.x; i < h2; i += blockDim.x) sb2[i] = a.b2[i];
    for (int i = threadIdx.x; i < 2 * h2; i += blockDim.x) sw3[i] = a.w3[i];
    if (LOCATE)
        level_runs(a.keys, a.nleaves, s_run);
    else
        __syncthreads();
    const float qnan = __int_as_float(0x7fc00000);
    for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < a.m; q += (i64)gridDim.x * blockDim.x) {
        float sx, sy, sz;
        const int32_t row = query_row<LOCATE>(a, s_run, q, sx, sy, sz);
        if (row < 0) {
            a.values[2 * q] = a.values[2 * q + 1] = qnan;
            if (a.grad) a.grad[3 * q] = a.grad[3 * q + 1] = a.grad[3 * q + 2] = qnan;
            continue;
        }
        const float* x = a.code + (i64)row * c;
        float f1[QDEC_MAX], z2[QDEC_MAX];
        for (int j = 0; j < h1; ++j) {
            const float* w = sw1 + j * c3;
            float s = 0.f;
            for (int k = 0; k < c; ++k) s += x[k] * w[3 + k];
            s += sb1[j] + (w[0] * sx + w[1] * sy + w[2] * sz);
            f1[j] = fmaxf(s, 0.f);
            z2[j] = 0.f;
        }
        float o0 = 0.f, o1 = 0.f;
        for (int j = 0; j < h2; ++j) {
            float s = 0.f;
            for (int k = 0; k < h1; ++k) s += f1[k] * sw2[j * h1 + k];
            s += sb2[j];
            s = fmaxf(s, 0.f);
            o0 += s * sw3[j];
            o1 += s * sw3[h2 + j];
            if (a.grad && s > 0.f)
                for (int k = 0; k < h1; ++k) z2[k] += sw3[j] * sw2[j * h1 + k];
        }
        if (a.vsize) o0 *= a.vsize[row];
        a.values[2 * q] = o0;
        a.values[2 * q + 1] = o1;
        if (a.grad) {
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
            for (int k = 0; k < h1; ++k) {
                const float z = f1[k] > 0.f ? z2[k] : 0.f;
                g0 += z * sw1[k * c3];
                g1 += z * sw1[k * c3 + 1];
                g2 += z * sw1[k * c3 + 2];
            }
            if (a.gsize) {
                const float size = a.gsize[row];
                g0 /= size;
                g1 /= size;
                g2 /= size;
            }
            a.grad[3 * q] = g0;
            a.grad[3 * q + 1] = g1;
            a.grad[3 * q + 2] = g2;
        }
    }
}

// The released widths (c = h1 = h2 = 32) on the f32 matrix cores, after k_decode_mfma (asr_conv.hip): same B
// fragments, same k order (MFMA step s of k-lane kk contracts k = 8 kk + s), same accumulators.  The three shift
// products are folded into the first layer's bias where the forward adds bias1, so that at shift 0 every operation is
// the forward's and the values are its bits.  A wave takes 64 queries at a time: one lane per query finds the row and
// the shift (LDS), then four groups of 16 run through the layers with their code rows loaded up front.  The gradient is
// two more tiles: z2 = (w3[0] * [f2 > 0]) . W2, then (z2 * [f1 > 0]) . W1[:, :3] (three real columns); [f1 > 0] stays
// as 8 bits per lane, [f2 > 0] is the sign of the A fragment the third layer consumes.
template <bool LOCATE, bool GRAD>
__global__ __launch_bounds__(256) void k_decode_at_mfma(QueryArgs a) {
    constexpr int C = 32, LD = 36;
    __shared__ __attribute__((aligned(16))) float s_t[4][16][LD];
    __shared__ float s_q[4][64][4];  // per wave and query: shift x, y, z, row (int bits)
    __shared__ i64 s_run[ASR_MAX_LEVEL + 2];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = lane & 15, kk = lane >> 4;
    const float* __restrict__ w1 = a.w1;
    const float* __restrict__ w2 = a.w2;
    const float* __restrict__ w3 = a.w3;
    float B1[8][2], B2[8][2], B3[8], bias1[2], bias2[2], W1s[2][3];
    float G2[8][2], W30[8], G1[8];  // gradient: W2 as [k][col], w3[0], W1[:, :3] as [k][d]
#pragma unroll
    for (int s = 0; s < 8; ++s) {
#pragma unroll
        for (int T = 0; T < 2; ++T) {
            B1[s][T] = w1[(i64)(16 * T + n) * (3 + C) + 3 + 8 * kk + s];
            B2[s][T] = w2[(i64)(16 * T + n) * C + 8 * kk + s];
            if (GRAD) G2[s][T] = w2[(i64)(8 * kk + s) * C + 16 * T + n];
        }
        B3[s] = n < 2 ? w3[n * C + 8 * kk + s] : 0.f;
        if (GRAD) {
            W30[s] = w3[8 * kk + s];
            G1[s] = n < 3 ? w1[(i64)(8 * kk + s) * (3 + C) + n] : 0.f;
        }
    }
#pragma unroll
    for (int T = 0; T < 2; ++T) {
        bias1[T] = a.b1[16 * T + n];
        bias2[T] = a.b2[16 * T + n];
#pragma unroll
        for (int d = 0; d < 3; ++d) W1s[T][d] = w1[(i64)(16 * T + n) * (3 + C) + d];
    }
    if (LOCATE) level_runs(a.keys, a.nleaves, s_run);
    const float qnan = __int_as_float(0x7fc00000);
    const i64 chunks = (a.m + 63) / 64;
    float (*st)[LD] = s_t[wave];
    float (*sq)[4] = s_q[wave];
    for (i64 ch = (i64)blockIdx.x * 4 + wave; ch < chunks; ch += (i64)gridDim.x * 4) {
        // ---- rows and shifts of the chunk's 64 queries, one lane each ----
        {
            const i64 q = ch * 64 + lane;
            float sx = 0.f, sy = 0.f, sz = 0.f;
            int32_t row = -1;
            if (q < a.m) row = query_row<LOCATE>(a, s_run, q, sx, sy, sz);
            __builtin_amdgcn_wave_barrier();
            sq[lane][0] = sx;
            sq[lane][1] = sy;
            sq[lane][2] = sz;
            sq[lane][3] = __int_as_float(row);
            __builtin_amdgcn_wave_barrier();
        }
        // ---- code rows of the four groups, all in flight ----
        float4 cd[4][2];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int32_t row = __float_as_int(sq[16 * g + n][3]);
            cd[g][0] = cd[g][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row >= 0) {
                cd[g][0] = *reinterpret_cast<const float4*>(a.code + (i64)row * C + 8 * kk);
                cd[g][1] = *reinterpret_cast<const float4*>(a.code + (i64)row * C + 8 * kk + 4);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (ch * 64 + 16 * g >= a.m) break;
            float x[8];
            x[0] = cd[g][0].x; x[1] = cd[g][0].y; x[2] = cd[g][0].z; x[3] = cd[g][0].w;
            x[4] = cd[g][1].x; x[5] = cd[g][1].y; x[6] = cd[g][1].z; x[7] = cd[g][1].w;
            // first-layer bias of voxel 4 kk + i, column 16 T + n: b1 + W1[:, :3] . s
            float bb1[4][2];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* sh = sq[16 * g + 4 * kk + i];
                const float sx = sh[0], sy = sh[1], sz = sh[2];
#pragma unroll
                for (int T = 0; T < 2; ++T) bb1[i][T] = bias1[T] + (W1s[T][0] * sx + W1s[T][1] * sy + W1s[T][2] * sz);
            }
            unsigned m1 = 0;  // bit 4 T + i: f1[voxel 4 kk + i][column 16 T + n] > 0
#pragma unroll
            for (int layer = 0; layer < 2; ++layer) {
                f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[s], layer == 0 ? B1[s][0] : B2[s][0], a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[s], layer == 0 ? B1[s][1] : B2[s][1], a1, 0, 0, 0);
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v0 = fmaxf(a0[i] + (layer == 0 ? bb1[i][0] : bias2[0]), 0.f);
                    const float v1 = fmaxf(a1[i] + (layer == 0 ? bb1[i][1] : bias2[1]), 0.f);
                    if (layer == 0) m1 |= (v0 > 0.f ? 1u << i : 0u) | (v1 > 0.f ? 16u << i : 0u);
                    st[4 * kk + i][n] = v0;
                    st[4 * kk + i][16 + n] = v1;
                }
                __builtin_amdgcn_wave_barrier();
                const float4 t0 = *reinterpret_cast<const float4*>(&st[n][8 * kk]);
                const float4 t1 = *reinterpret_cast<const float4*>(&st[n][8 * kk + 4]);
                x[0] = t0.x; x[1] = t0.y; x[2] = t0.z; x[3] = t0.w;
                x[4] = t1.x; x[5] = t1.y; x[6] = t1.z; x[7] = t1.w;
            }
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 8; ++s) o = __builtin_amdgcn_mfma_f32_16x16x4f32(x[s], B3[s], o, 0, 0, 0);
            if (n < 2) {  // o[i] = out[voxel 4 kk + i][n]
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int v = 16 * g + 4 * kk + i;
                    const i64 q = ch * 64 + v;
                    if (q < a.m) {
                        const int32_t row = __float_as_int(sq[v][3]);
                        float val = o[i];
                        if (row < 0)
                            val = qnan;
                        else if (n == 0 && a.vsize)
                            val = o[i] * a.vsize[row];
                        a.values[2 * q + n] = val;
                    }
                }
            }
            if (GRAD) {
                // z2[voxel][column of h1] = sum_k z3[voxel][k] W2[k][column], z3 = w3[0] where f2 > 0 (A layout: x)
                f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const float za = x[s] > 0.f ? W30[s] : 0.f;
                    z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(za, G2[s][0], z0, 0, 0, 0);
                    z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(za, G2[s][1], z1, 0, 0, 0);
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    st[4 * kk + i][n] = (m1 >> i & 1u) ? z0[i] : 0.f;
                    st[4 * kk + i][16 + n] = (m1 >> (4 + i) & 1u) ? z1[i] : 0.f;
                }
                __builtin_amdgcn_wave_barrier();
                const float4 t0 = *reinterpret_cast<const float4*>(&st[n][8 * kk]);
                const float4 t1 = *reinterpret_cast<const float4*>(&st[n][8 * kk + 4]);
                const float y[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
                f32x4 gz = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 8; ++s) gz = __builtin_amdgcn_mfma_f32_16x16x4f32(y[s], G1[s], gz, 0, 0, 0);
                if (n < 3) {  // gz[i] = d value[voxel 4 kk + i][0] / d shift[n]
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int v = 16 * g + 4 * kk + i;
                        const i64 q = ch * 64 + v;
                        if (q < a.m) {
                            const int32_t row = __float_as_int(sq[v][3]);
                            float gv = gz[i];
                            if (row < 0)
                                gv = qnan;
                            else if (a.gsize)
                                gv = gv / a.gsize[row];
                            a.grad[3 * q + n] = gv;
                        }
                    }
                }
            }
        }
    }
}

template <bool LOCATE>
int launch_decode_at(asr_hip_context* ctx, const QueryArgs& a) {
    if (a.m <= 0) return ASR_HIP_OK;
    if (a.c > QDEC_MAX || a.h1 > QDEC_MAX || a.h2 > QDEC_MAX || a.c < 1 || a.h1 < 1 || a.h2 < 1)
        ASR_FAIL(ctx, ASR_HIP_EINVAL, "decode_mlp_at: layer widths must be 1..64");
    if (a.m >= (i64(1) << 31)) ASR_FAIL(ctx, ASR_HIP_EINVAL, "decode_mlp_at: more than 2^31 - 1 queries in one call");
    if (a.c == 32 && a.h1 == 32 && a.h2 == 32 && ((uintptr_t)a.code % 16 == 0)) {
        const unsigned blocks = (unsigned)std::min<i64>((a.m + 255) / 256, 2048);
        if (a.grad)
            k_decode_at_mfma<LOCATE, true><<<blocks, 256, 0, ctx->stream>>>(a);
        else
            k_decode_at_mfma<LOCATE, false><<<blocks, 256, 0, ctx->stream>>>(a);
    } else {
        const size_t lds = sizeof(float) * (size_t)(a.h1 * (3 + a.c) + a.h1 + a.h2 * a.h1 + a.h2 + 2 * a.h2);
        const unsigned blocks = (unsigned)std::min<i64>(grid_for(a.m, 256), 4096);
        k_decode_at<LOCATE><<<blocks, 256, lds, ctx->stream>>>(a);
    }
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

}  // namespace

int asr_query_leaf_locate(asr_hip_context* ctx, const asr_octree_frame* frame, const u64* keys, i64 n, const float* pos,
                          i64 m, int32_t* rows) {
    if (m <= 0) return ASR_HIP_OK;
    if (n < 0 || n >= (i64(1) << 31)) ASR_FAIL(ctx, ASR_HIP_EINVAL, "leaf_locate: num_leaves must be 0 .. 2^31 - 1");
    const unsigned blocks = (unsigned)std::min<i64>(grid_for(m, 256), 8192);
    k_leaf_locate<<<blocks, 256, 0, ctx->stream>>>(*frame, keys, n, pos, m, rows);
    ASR_CHECK_LAUNCH(ctx);
    return ASR_HIP_OK;
}

int asr_query_decode_at(asr_hip_context* ctx, const float* code, int c, const int32_t* rows, const float* shifts, i64 m,
                        const float* w1, const float* b1, int h1, const float* w2, const float* b2, int h2,
                        const float* w3, const float* sizes, float* values, float* grad) {
    QueryArgs a = {};
    a.code = code;
    a.c = c;
    a.h1 = h1;
    a.h2 = h2;
    a.w1 = w1;
    a.b1 = b1;
    a.w2 = w2;
    a.b2 = b2;
    a.w3 = w3;
    a.m = m;
    a.rows = rows;
    a.shifts = shifts;
    a.vsize = sizes;
    a.values = values;
    a.grad = grad;
    return launch_decode_at<false>(ctx, a);
}

int asr_query_implicit(asr_hip_context* ctx, const asr_octree_frame* frame, const u64* keys, const float* centers,
                       const float* sizes, i64 num_leaves, const float* code, int c, const float* w1, const float* b1,
                       int h1, const float* w2, const float* b2, int h2, const float* w3, int scale_sdf,
                       const float* pos, i64 m, float* values, float* grad, int32_t* rows_out) {
    if (num_leaves >= (i64(1) << 31)) ASR_FAIL(ctx, ASR_HIP_EINVAL, "implicit_query: more than 2^31 - 1 leaves");
    QueryArgs a = {};
    a.code = code;
    a.c = c;
    a.h1 = h1;
    a.h2 = h2;
    a.w1 = w1;
    a.b1 = b1;
    a.w2 = w2;
    a.b2 = b2;
    a.w3 = w3;
    a.m = m;
    a.frame = *frame;
    a.keys = keys;
    a.nleaves = num_leaves;
    a.centers = centers;
    a.sizes = sizes;
    a.pos = pos;
    // values[:, 0] *= size with scale_sdf (asr.cpp:334-336); d values[:, 0] / d p = z1 / size without it, z1 with it
    a.vsize = scale_sdf ? sizes : nullptr;
    a.gsize = scale_sdf ? nullptr : sizes;
    a.values = values;
    a.grad = grad;
    a.rows_out = rows_out;
    return launch_decode_at<true>(ctx, a);
}
