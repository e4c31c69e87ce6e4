/*
 * asr_hip.h -- C ABI of the MI355X (gfx950) implementation of the adaptive-surface-
 * reconstruction hot path: oriented points -> signed/unsigned implicit values on the
 * adaptive octree grid.
 *
 * Conventions
 *   - every pointer documented as "dev" is a device (HBM) pointer, everything else is host
 *   - all kernels are enqueued on the context's hipStream_t; functions that return a
 *     data-dependent size synchronise that stream before returning
 *   - int return value: 0 = ok, otherwise an ASR_HIP_E* code; asr_hip_last_error() gives text
 *   - no ownership transfer: the caller allocates every output after the *_count call
 *   - dtypes follow the reference tensors (cpp/lib/asr.cpp:179-312): indices int32, kernel
 *     indices uint8, row splits int64, keys uint64, features float32
 *
 * Count / fill pairs
 *   Eight operators come as X_count, which does the work, reports the output sizes and parks device arrays in the
 *   context's scratch arena, and X_fill, which writes the outputs from them: asr_hip_multi_radius_search, _dual_cells
 *   (both count forms), _contour, _components, _mesh_simplify, _mesh_edges, _mesh_fill_holes and _points_merge.
 *   A context holds ONE pending count.  X_fill completes the most recent successful _count on that context, which must
 *   be X's own, and does so once.  It is refused -- ASR_HIP_EINVAL "... must follow the matching ... call", on the host,
 *   nothing is launched -- when no count is pending, when the last count was another operator's or failed (a count that
 *   begins voids the pending one, whatever becomes of it), and when any call that RECYCLES THE SCRATCH ARENA ran on the
 *   context in between: the parked arrays then belong to that call.  Such calls are every _count of these pairs, both
 *   calls of the grid_neighbors and grid_coarsen pairs, the octree builds and the asr_hip_implicit_* entry points, and
 *   every single-call operator that needs device temporaries (the searches: knn_*, radius_neighbor_count,
 *   nearest_point, point_attributes_at, icp_step, register_points; row_groups, invert_neighbors_list, sparse_conv_plan_create,
 *   continuous_conv_f32; mesh_sample, mesh_topology, mesh_smooth; normals_orient; point_fpfh, feature_match,
 *   ransac_transform).  Take every call that enqueues work
 *   on the context for one of them; the calls that only read or set host state (last_error, options, set_stream, ...)
 *   never are.  The input arrays of X_count must stay alive and unchanged until X_fill returns: fill reads them again.
 *
 * The reference has no C ABI (the ASR_API_EXTERN_C macros of cpp/lib/asr_config.h:18-28 are
 * unused); each entry point cites the reference interface it stands in for.
 */
#ifndef ASR_HIP_H
#define ASR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASR_HIP_OK 0
#define ASR_HIP_EINVAL 1   /* bad argument (shape / null / unsupported size)            */
#define ASR_HIP_EHIP 2     /* a HIP runtime call failed                                 */
#define ASR_HIP_ENODEV 3   /* no gfx950 device / extension not usable                   */
#define ASR_HIP_ELOGIC 4   /* internal invariant violated (e.g. hash table overflow)    */
#define ASR_HIP_EWEIGHT 5  /* weight table incomplete / wrong shape                     */
#define ASR_HIP_EPEER 6    /* sharded forward: ANOTHER rank failed; every rank returns  */

#define ASR_MAX_LEVEL 21      /* cpp/lib/octreebase.h:42                                  */
#define ASR_NUM_GRIDS 5       /* cpp/lib/asr.cpp:156, models/v0/net_definitions_torch.py:403 */

typedef struct asr_hip_context asr_hip_context;

/* Octree frame: per-level voxel sizes and the integer offset of the root cube.
 * Replaces asr::Octree::Octree (cpp/lib/octree.cpp:20-42); plain host POD, passed by value
 * into kernels. */
typedef struct asr_octree_frame {
    float voxel_size[ASR_MAX_LEVEL + 1];
    float inv_voxel_size[ASR_MAX_LEVEL + 1];
    int32_t offset[3];
    float bb_min[3];
    float bb_max[3];
} asr_octree_frame;

/* ---- context ---------------------------------------------------------------------- */
/* stream: a hipStream_t (NULL = the null stream). The context owns a device arena that is
 * reused across calls. */
int asr_hip_context_create(asr_hip_context** ctx, void* stream);
void asr_hip_context_destroy(asr_hip_context* ctx);
/* Moves the context to another stream of its device.  The context's arenas and counters are shared by all streams it
 * visits, so the move orders the new stream behind everything the context enqueued on the previous one (one event: recorded
 * there, awaited here); the previous stream must therefore still exist when the stream is changed.  Setting the stream
 * the context already has does nothing.  A failing HIP call leaves its text in asr_hip_last_error(). */
void asr_hip_context_set_stream(asr_hip_context* ctx, void* stream);
const char* asr_hip_last_error(const asr_hip_context* ctx);
const char* asr_hip_version(void); /* asr::GetVersionStr, cpp/lib/asr.hpp:29 */
/* sizeof() of an ABI struct by name ("asr_octree_frame", "asr_sparse_conv_args", "asr_weight",
 * "asr_implicit_params", "asr_implicit_sizes"); 0 for unknown names. Lets FFI bindings verify
 * their struct layouts. */
size_t asr_hip_struct_size(const char* name);
/* bytes currently reserved by the arena */
size_t asr_hip_context_reserved_bytes(const asr_hip_context* ctx);
/* HIP device the context is bound to (the device current when it was created); every entry point
 * selects it on the calling thread.  -1 for a null context. */
int asr_hip_context_device(const asr_hip_context* ctx);
/* The whole-path driver keeps packed 16-bit copies of the weight tensors it was given (keyed by the tensors'
 * device pointers and shapes).  Call this after the contents of a weight tensor changed in place -- or when a new
 * table may reuse the addresses of an old one -- so that the copies are made again by the next forward. */
int asr_hip_context_weights_changed(asr_hip_context* ctx);
/* Per-context tunables (no process-wide state).  Names: "sconv_min_blocks" (2816) and
 * "sconv_wide_min" (2048): launch-size thresholds that pick the sparse-conv tile shape;
 * "row_segment" (524288), "row_lpt" (1): MFMA row regrouping; "overlap" (1): aggregation search on a
 * second stream; "build_search" (1): 0 makes asr_hip_implicit_build stop
 * after the grid hierarchy (a rank of a sharded run searches only the rows it owns).  Results never depend
 * on the tuning options: none of them skips work.
 * "search_half" (1): the aggregation search of asr_hip_implicit_build covers a voxel's ball with 4^3 half-size
 * cells for the rows with many candidates (2: for every voxel, 0: 3^3 full-size cells throughout).  get_option also answers the read-only "last_search_margin_pairs": pairs the last
 * such search found in the rounding margin of the half-size cells.
 * Read-only "table_regrows": the number of times a hash table of the geometry half (octree closure and key growth, voxel
 * key maps of the neighbour lists, the cell tables of the searches -- the early table of the overlapped
 * build that is dropped included) overflowed and was rebuilt four times the size, since the context was created; the
 * auxiliary search context is summed in.  Cumulative: take differences around a call.  Lattice-aligned clouds cause it
 * (many keys share the low 6 bits that choose the slot inside a table's 64-slot buckets); a grown cell table stays grown
 * for the later searches of the context.  It is no entry of asr_hip_option_info. */
int asr_hip_context_set_option(asr_hip_context* ctx, const char* name, int64_t value);
int asr_hip_context_get_option(asr_hip_context* ctx, const char* name, int64_t* value);
/* The table of tunables: name and built-in default of option `index` (0, 1, ... until ASR_HIP_EINVAL).  A context's defaults can
 * be seeded from the environment (ASR_<NAME>) when it is created; bench.py prints every option that differs from its built-in
 * default into the line's `config` (the reference has no tunables: cpp/lib/asr.hpp:27-101). */
int asr_hip_option_info(int index, const char** name, int64_t* default_value);

/* ---- print callbacks: asr::SetPrintCallbackFunction (cpp/lib/asr.hpp:25-34, asr.cpp:34-47) ------------- */
/* Process-wide like the reference's (a static table of four callbacks).  Levels: cpp/lib/asr.hpp:27.  The whole-path
 * entry points announce their stages at ASR_HIP_INFO with the reference's texts (cpp/lib/asr.cpp:117,144,264,
 * 314-323): "grid building\n", "aggregate\n", "network aggregate\n", "network unet\n", "network decode\n"
 * ("preprocessing\n" comes from the host side that runs the pre-filter).  Without a callback nothing is printed. */
#define ASR_HIP_DEBUG 0
#define ASR_HIP_INFO 1
#define ASR_HIP_WARN 2
#define ASR_HIP_ERROR 3
typedef void (*asr_hip_print_callback)(const char* msg, void* user);
/* installs `callback` (NULL: removes) for each of levels[0..num_levels); ASR_HIP_EINVAL for a level outside
 * DEBUG..ERROR ("invalid verbosity level", asr.cpp:42-44) -- nothing is changed in that case */
int asr_hip_set_print_callback(asr_hip_print_callback callback, void* user, const int* levels, int num_levels);
/* asr::Print (cpp/lib/utils.h:26): hands msg to the callback of `level`, if one is installed */
void asr_hip_print(const char* msg, int level);

/* ---- a3: octree frame (cpp/lib/octree.cpp:20-42), host only --------------------------- */
int asr_octree_frame_init(asr_octree_frame* frame, const float bb_min[3], const float bb_max[3]);

/* ---- a1/a2/a3: per-point location codes (cpp/lib/octree.h:42-68, octreebase.h:59-65) --- */
/* keys_out[i] = key of point i at the level chosen from radius_scale*radii[i] (clamped to
 * max_depth); 0 for points outside [bb_min,bb_max] or with an invalid coordinate. */
int asr_hip_point_keys(asr_hip_context* ctx, const asr_octree_frame* frame,
                       const float* points_dev, const float* radii_dev, int64_t n,
                       float radius_scale, int max_depth, uint64_t* keys_out_dev);

/* ---- a4: octree construction (asr::CreateOctreeFromPoints, cpp/lib/octree.cpp:230-280;
 *      pybind create_octree, cpp/pybind/module.cpp:144-161) ----------------------------- */
/* Builds the balanced node set inside the context and reports its sizes (grow_steps = 0, the value of the
 * reconstruction path, cpp/lib/asr.cpp:151-153). */
int asr_hip_octree_build(asr_hip_context* ctx, const asr_octree_frame* frame,
                         const float* points_dev, const float* radii_dev, int64_t n,
                         float radius_scale, int max_depth, int64_t* num_nodes,
                         int64_t* num_leaves);
/* the same with Octree::Grow (cpp/lib/octree.cpp:44-108) applied `grow_steps` times to the point keys before the
 * closure, as create_octree(..., grow_steps, ...) of the pybind module does (cpp/pybind/module.cpp:144-161).  The
 * candidate test of an iteration (:87) is evaluated against the key set at the start of the iteration; the reference
 * walks its hash map sequentially, which only matters for grow_steps >= 2 on trees that mix levels. */
int asr_hip_octree_build_grow(asr_hip_context* ctx, const asr_octree_frame* frame,
                              const float* points_dev, const float* radii_dev, int64_t n,
                              float radius_scale, int grow_steps, int max_depth, int64_t* num_nodes,
                              int64_t* num_leaves);
/* An octree in parts, for builds that are spread over several processes: the node set is the closure (all siblings,
 * all ancestors; cpp/lib/octree.cpp:110-150) of the keys of `points` AND of `extra_keys` (node keys of other builds),
 * then 2:1 balanced (:152-206) unless balance == 0.  Closure commutes with union, so every rank can close the keys of its
 * share of the points (balance = 0), the ranks exchange their node lists, and each rank closes and balances the union
 * (n = 0, extra_keys = all lists): the tree of the whole cloud, bit for bit. */
int asr_hip_octree_build_parts(asr_hip_context* ctx, const asr_octree_frame* frame, const float* points_dev,
                               const float* radii_dev, int64_t n, float radius_scale, int max_depth,
                               const uint64_t* extra_keys_dev, int64_t num_extra, int balance,
                               int64_t* num_nodes, int64_t* num_leaves);
/* copies the sorted node keys / sorted leaf keys (tree.leaves) of the last build */
int asr_hip_octree_get(asr_hip_context* ctx, uint64_t* nodes_out_dev, uint64_t* leaves_out_dev);

/* ---- dual cells ("next" row D.1): asr::CreateDualVertexIndices (cpp/lib/grid.cpp:316-459) ------ */
/* For the octree of the last asr_hip_octree_build / asr_hip_implicit_build of this context.
 * count returns the number of dual cells D; fill writes [D,8] leaf indices (leaf order x corner
 * order), the `dual_vertex_indices` consumed by CreateTriangleMesh (cpp/lib/asr.cpp:154,340).  A count / fill pair
 * ("Count / fill pairs" at the top of this file). */
int asr_hip_dual_cells_count(asr_hip_context* ctx, int64_t* num_cells);
/* the same for ANY octree given by its sorted node / leaf keys (asr_hip_octree_get): the pybind Octree handle
 * (cpp/pybind/module.cpp:230-235) stays usable however many trees were built since. */
int asr_hip_dual_cells_count_for(asr_hip_context* ctx, const uint64_t* nodes_dev, int64_t num_nodes,
                                 const uint64_t* leaves_dev, int64_t num_leaves, int64_t* num_cells);
int asr_hip_dual_cells_fill(asr_hip_context* ctx, int64_t* dual_vertex_indices_out_dev);

/* ---- dual contouring ("next" row D.2): asr::CreateTriangleMesh (cpp/lib/contouring.cpp:29-460) ---- */
/* values [V,2] (signed, unsigned), dual_vertex_indices [D,8] int64, node_positions [V,3]; all
 * device pointers.  A count / fill pair ("Count / fill pairs" at the top): count returns the mesh sizes, fill
 * writes vertices f32[M,3] (one per active dual cell in dual order, then the fan centres in
 * emission order) and triangles i32[T,3] in the reference's serial emission order, including the
 * corner order it derives from libstdc++'s unordered_set iteration (see csrc/asr_uset.h).
 * count checks on the device, before any load through them, that every dual vertex index lies in
 * [0, num_values): ASR_HIP_EINVAL "contour: dual vertex index out of range" otherwise.  More than 29 active
 * cells around one crossing edge (no face-balanced octree has more than 8) is ASR_HIP_ELOGIC from count; cells
 * around an edge that cannot be ordered are the reference's "cannot sort duals", ASR_HIP_ELOGIC from fill. */
int asr_hip_contour_count(asr_hip_context* ctx, const float* values_dev, int64_t num_values,
                          const int64_t* dual_vertex_indices_dev, int64_t num_duals,
                          const float* node_positions_dev, float value_threshold,
                          int64_t* num_vertices, int64_t* num_triangles);
int asr_hip_contour_fill(asr_hip_context* ctx, float* vertices_out_dev, int32_t* triangles_out_dev);

/* ---- component filter ("next" row D.3): asr::RemoveConnectedComponents
 * (cpp/lib/postprocess.cpp:141-176).  Keeps the keep_n largest components (size in vertices,
 * ties -> the component found later first, like std::greater on (size, label)) that have at least
 * min_size vertices; compacts vertices and re-indexes triangles, order preserving.  A count / fill pair ("Count /
 * fill pairs" at the top). */
int asr_hip_components_count(asr_hip_context* ctx, const float* vertices_dev, int64_t num_vertices,
                             const int32_t* triangles_dev, int64_t num_triangles, int64_t keep_n,
                             int64_t min_size, int64_t* num_vertices_out, int64_t* num_triangles_out);
int asr_hip_components_fill(asr_hip_context* ctx, float* vertices_out_dev, int32_t* triangles_out_dev);

/* Host-only: asr::ComputeInlierFromDensity (cpp/lib/preprocess.cpp:41-62) on the neighbour counts of
 * asr_hip_radius_neighbor_count (host array).  Reproduces the reference literally, including that
 * it compares the counts AFTER std::partial_sort has permuted them in place (:53-60), so inlier[i]
 * is not a function of point i's own count (quirk B.11 in DESIGN.md). */
int asr_density_inlier(const int64_t* counts_host, int64_t n, double density_percentile_threshold,
                       uint8_t* inlier_out_host);

/* Host-only helper (no GPU): iteration order of a libstdc++ std::unordered_set<size_t> filled with
 * xs[0..n) in that order, n <= 29 -- the rule the contouring kernel replays (csrc/asr_uset.h). */
int asr_hip_unordered_set_order(const uint32_t* xs, int n, uint32_t* out);

/* ---- a5: CreateLeafNeighborInformation (cpp/lib/grid.cpp:43-175) ---------------------- */
/* keys: sorted unique voxel keys. count: fills row_splits[V+1] and returns the pair count;
 * fill: writes the CSR entries in ascending kernel-slot order.
 * Both build the voxel key map.  The context notes the enlargement the map of the last count call needed ("table_regrows"
 * above) with the keys' address and number; the next fill call on the same context with that address and number starts at
 * that size, not at the smallest, and clears the note.  A fill call without such a note grows its map by itself; the
 * results never depend on it.  The same holds for the row-list pair below. */
int asr_hip_grid_neighbors_count(asr_hip_context* ctx, const uint64_t* keys_dev, int64_t v,
                                 int64_t* row_splits_out_dev, int64_t* num_pairs);
int asr_hip_grid_neighbors_fill(asr_hip_context* ctx, const uint64_t* keys_dev, int64_t v,
                                const int64_t* row_splits_dev, int32_t* index_out_dev,
                                uint8_t* kernel_index_out_dev);

/* The same for a list of rows (ascending voxel indices, int32): row_splits keeps its full length V + 1 with empty
 * rows for the voxels that are not listed, index / kernel_index hold the listed rows' entries only.  A rank of the
 * one-scan sharding builds the lists of the voxels it owns. */
int asr_hip_grid_neighbors_rows_count(asr_hip_context* ctx, const uint64_t* keys_dev, int64_t v,
                                      const int32_t* rows_dev, int64_t num_rows, int64_t* row_splits_out_dev,
                                      int64_t* num_pairs);
int asr_hip_grid_neighbors_rows_fill(asr_hip_context* ctx, const uint64_t* keys_dev, int64_t v,
                                     const int32_t* rows_dev, int64_t num_rows, const int64_t* row_splits_dev,
                                     int32_t* index_out_dev, uint8_t* kernel_index_out_dev);

/* ---- a6: CombineSiblings (cpp/lib/grid.cpp:177-243) ----------------------------------- */
/* keys: sorted unique voxel keys. count: returns the coarse voxel count; fill: v_out must be that count
 * (ASR_HIP_EINVAL otherwise). */
int asr_hip_grid_coarsen_count(asr_hip_context* ctx, const uint64_t* keys_dev, int64_t v,
                               int64_t* v_out);
int asr_hip_grid_coarsen_fill(asr_hip_context* ctx, const uint64_t* keys_dev, int64_t v,
                              uint64_t* out_keys_dev, int64_t v_out, int32_t* up_index_out_dev,
                              uint8_t* up_kernel_index_out_dev, int64_t* up_row_splits_out_dev);

/* ---- a7: InitGridVoxelInfo (cpp/lib/grid.cpp:251-268) --------------------------------- */
int asr_hip_voxel_info(asr_hip_context* ctx, const asr_octree_frame* frame,
                       const uint64_t* keys_dev, int64_t v, float* centers_out_dev,
                       float* sizes_out_dev);

/* ---- a8: ComputeAggregationNeighborsAndScaleCompatibility (cpp/lib/nsearch.cpp:107-162) - */
/* Members of row q: points with ((dx*dx+dy*dy)+dz*dz) < size[q]^2, ordered by (distance,
 * index); dist = squared distance; compat = (min(size, 2 r)/max(size, 2 r))^2.  A count / fill pair ("Count / fill
 * pairs" at the top); fill must name the n and v of its count. */
int asr_hip_multi_radius_search_count(asr_hip_context* ctx, const asr_octree_frame* frame,
                                      const float* points_dev, int64_t n,
                                      const float* centers_dev, const float* sizes_dev,
                                      int64_t v, int64_t* row_splits_out_dev,
                                      int64_t* num_pairs);
int asr_hip_multi_radius_search_fill(asr_hip_context* ctx, const float* points_dev,
                                     const float* radii_dev, int64_t n,
                                     const float* centers_dev, const float* sizes_dev,
                                     int64_t v, const int64_t* row_splits_dev,
                                     int32_t* index_out_dev, float* dist_out_dev,
                                     float* compat_out_dev);

/* ---- pre-filter ("next" row D.4): asr::KDTree (cpp/lib/nsearch.cpp:23-105) -------------------- */
/* The frame only defines the acceleration grid; any box that contains the points works.
 * radii_out[i] = distance to the k-th nearest neighbour, the point itself included (:30-51).
 * If inlier_out is given, radii_in is required: inlier iff fewer than outlier_threshold of the k
 * nearest neighbours have radius < radius_fraction * radii_in[i] (:54-86). */
int asr_hip_knn_radius(asr_hip_context* ctx, const asr_octree_frame* frame, const float* points_dev,
                       int64_t n, int k, const float* radii_in_dev, float radius_fraction,
                       int outlier_threshold, float* radii_out_dev, uint8_t* inlier_out_dev);
/* counts_out[i] = number of points with squared distance < radii[i]^2 (:88-105) */
int asr_hip_radius_neighbor_count(asr_hip_context* ctx, const asr_octree_frame* frame,
                                  const float* points_dev, const float* radii_dev, int64_t n,
                                  int64_t* counts_out_dev);

/* ---- a10: open3d::continuous_conv as used by CConvAggregationBlock
 *      (models/v0/net_definitions_torch.py:53-70,107-116): kernel 4x4x4, align_corners,
 *      linear, ball_to_cube_radial, per-output extent, per-neighbour importance ------------ */
/* filters [4,4,4,cin,cout]; out = conv (+bias if bias_dev) (relu if relu). */
int asr_hip_continuous_conv_f32(asr_hip_context* ctx, const float* filters_dev,
                                const float* out_positions_dev, const float* extents_dev,
                                const float* inp_positions_dev, const float* inp_features_dev,
                                const int32_t* neighbors_index_dev,
                                const float* neighbors_importance_dev,
                                const int64_t* neighbors_row_splits_dev, int64_t num_out,
                                int cin, int cout, int normalize, const float* bias_dev,
                                int relu, float* out_dev);
/* Backward support ("next" row f4): per-output interpolation matrices basis_out [num_out, 4*4*4*cin] (filter cell
 * major, un-normalised: sum_p importance_p * trilinear_weight(cell, p) * feature_p[c]) and importance sums norm_out
 * [num_out]; the filter gradient is dW = basis^T (g / norm).  cin must be 4. */
int asr_hip_continuous_conv_basis_f32(asr_hip_context* ctx, const float* out_positions_dev, const float* extents_dev,
                                      const float* inp_positions_dev, const float* inp_features_dev,
                                      const int32_t* neighbors_index_dev, const float* neighbors_importance_dev,
                                      const int64_t* neighbors_row_splits_dev, int64_t num_out, int cin,
                                      float* basis_out_dev, float* norm_out_dev);
/* neighbors_importance = compat * clamp((1-d)^3,0,1) (models/common_torch.py:21-22,
 * net_definitions_torch.py:107) */
int asr_hip_aggregation_importance(asr_hip_context* ctx, const float* compat_dev,
                                   const float* dist_dev, int64_t num_pairs, float* out_dev);

/* ---- a12: SpecialSparseConv.forward / open3d::sparse_conv
 *      (models/common_torch.py:95-148) ------------------------------------------------- */
typedef struct asr_sparse_conv_args {
    const float* filters;              /* dev [K, cin, cout] row-major                       */
    const float* inp_features;         /* dev, row i at inp_features + i*inp_ld              */
    int64_t inp_ld;                    /* row stride in floats (>= cin)                      */
    const float* inp_importance;       /* dev [num_inp] or NULL: neighbour importance =
                                          inp_importance[neighbors_index] (:124-126)         */
    const float* neighbors_importance; /* dev [P] or NULL: per-pair importance as taken by
                                          open3d::sparse_conv; wins over inp_importance      */
    const int32_t* neighbors_index;    /* dev [P]                                            */
    const uint8_t* neighbors_kernel_index; /* dev [P]                                        */
    const int64_t* neighbors_row_splits;   /* dev [num_out+1]                                */
    int64_t num_out;
    int64_t num_inp;
    int kernel_size;                   /* 55 or 9                                            */
    int cin, cout;
    int normalize;                     /* divide by the importance sum (if != 0)             */
    const float* bias;                 /* dev [cout] or NULL (:144-145)                      */
    int relu;                          /* (:146)                                             */
    const float* residual;             /* dev or NULL: added after the activation
                                          (net_definitions_torch.py:633)                     */
    int64_t residual_ld;
    float* out;                        /* dev, row i at out + i*out_ld                       */
    int64_t out_ld;
    float* out_importance;             /* dev [num_out] or NULL: sum of neighbour importance
                                          (reduce_subarrays_sum, :127-128)                   */
    int algo;                          /* 0 = auto, 1 = scalar reference kernel, 2 = MFMA    */
    const int32_t* row_perm;           /* dev [num_out] or NULL: order in which the MFMA kernel
                                          tiles the output rows (asr_hip_row_groups); results
                                          do not depend on it                                */
    /* optional second filter bank, same gather, same launch (SparseConvBlock conv1a + conv1b,
     * models/v0/net_definitions_torch.py:262-281): output columns [cout, cout + cout_b).  With
     * filters_b != NULL the importance arrays, `normalize` and `out_importance` belong to bank b
     * only and bank a is the plain convolution.  MFMA path: cout % 16 == 8, cout_b == 8. */
    const float* filters_b;            /* dev [K, cin, cout_b] or NULL                       */
    const float* bias_b;               /* dev [cout_b] or NULL                               */
    int cout_b;
    /* 0 = chosen from the problem size.  Otherwise the MFMA kernel instance is forced: column tile
     * width force_nt * 16 (1, 2, 4, 8, 16) and force_waves * 16 rows per block (4 or 8) -- lets a
     * small input run the instances that large inputs select (parity tests). */
    int force_nt;
    int force_waves;
    /* 16-bit entry points only: row-group plan of this neighbour list (asr_hip_sparse_conv_plan_create), or NULL
     * to have a temporary one built for the call.  A plan is tied to (neighbour arrays, row_perm, num_out). */
    const struct asr_hip_conv_plan* plan;
    /* ASR_CONV16_F16X2 only: largest |element| of inp_features as f32 bits (device scalar), or NULL to have it
     * computed by one pass over the input. */
    const uint32_t* inp_absmax;
    /* 16-bit entry points: device scalar that receives max(its value, f32 bits of the largest |element| written to
     * `out`) -- the inp_absmax of the convolutions that read `out`; the caller zeroes it.  NULL: not kept. */
    uint32_t* out_absmax;
} asr_sparse_conv_args;
/* The call is asynchronous and does not inspect the list.  With algo 0 or 2 (the MFMA kernel keeps one neighbour per
 * (row, slot)) a row may name every kernel slot at most once (true for all lists of the reference's grids,
 * cpp/lib/grid.cpp:99-170, 229-240); a row that names a slot twice gets one of the two neighbours, unspecified which,
 * and both importances in its sum.  algo = 1 (the scalar kernel) takes any list and sums repeated slots.  Both kernels
 * skip an entry whose slot is >= kernel_size, its importance included. */
int asr_hip_sparse_conv_f32(asr_hip_context* ctx, const asr_sparse_conv_args* args);
/* Launch statistics of the MFMA sparse conv since the last reset: text "NT,KC,IMP,WAVES,DUAL:count;..."
 * (template instance k_sconv_mfma<NT,KC,IMP,WAVES,DUAL> -> number of launches), NUL terminated.  The 16-bit
 * kernels count as "NT,KC,IMP,WAVES,DUAL,MODE,PLAN" (PLAN 1: k_sconv_plan16, 0: k_sconv_mfma16). */
int asr_hip_sparse_conv_variant_counts(asr_hip_context* ctx, char* buf, size_t cap, int reset);

/* ---- a12 on the 16-bit matrix cores (v_mfma_f32_16x16x32_{f16,bf16}) --------------------------------
 * ASR_CONV16_F16 (BASELINE config C5, "fp16 features"): activations in HBM are f16, weights are rounded to
 *   f16 once, products accumulate in f32.  In args, inp_features / residual / out point to f16 data (out: f32
 *   when out_is_f16 == 0), leading dimensions count elements; importance, bias and out_importance stay f32.
 * ASR_CONV16_BF16X3: f32 activations and weights; every operand is split exactly into three bf16 terms and
 *   the product is evaluated with six bf16 MFMAs, f32 accumulate -- fp32-class results (error of the dropped
 *   terms < 2^-23 per product) at 2.7x the f32 matrix peak.  args as for asr_hip_sparse_conv_f32.
 * ASR_CONV16_F16X2: f32 activations and weights, fp32-class results from HALF the MFMAs of bf16x3: each tensor is
 *   scaled by a power of two (its largest magnitude to [2^14, 2^15): exact, no f16 overflow or underflow worth
 *   speaking of) and split into two f16 terms, a*b = a0*b0 + a1*b0 + a0*b1 (three f16 MFMAs, f32 accumulate).
 *   Error per product < 2^-21 for elements within 2^-17 of their tensor's maximum, < 2^-38 of the product of the
 *   maxima otherwise.  The activations' scale comes from args->inp_absmax, which the producing convolution keeps
 *   through args->out_absmax (asr_hip_absmax_f32 for other producers).  args as for asr_hip_sparse_conv_f32.
 * ASR_CONV16_BF16X3_2ACC: bf16x3 with a second accumulator -- the same operands, packed filters (byte for byte) and six
 *   products, but only the leading product a0*b0 goes to the running sum; the five small ones go to a second f32
 *   accumulator that is added once, before the epilogue (importance-weighted tiles keep the one chain of bf16x3).
 *   The running sum is rounded once per step instead of six times: on the full-width network at 1 M points the rms
 *   error is about 1/3 of the exact-f32 kernel's, with no bias (bf16x3: slightly above it, biased negative), for
 *   3.5 % more U-Net time than bf16x3 at 10 M points (32 more registers on the 128-column tiles: two blocks per CU
 *   instead of three).  args as for asr_hip_sparse_conv_f32.
 * All take the filters re-packed by asr_hip_sparse_conv_pack (16-bit, [plane][K][cin panel][cout padded to
 * 16][panel depth] in the kernels' LDS order; bank b appended as columns); args->filters / filters_b are
 * ignored, cout_b > 0 selects the two-bank form.  cin and the row strides must be multiples of 8 (f16) / 4 (f32) elements.
 * A row may name every kernel slot at most once (true for all lists of the reference's grids, cpp/lib/grid.cpp:99-170,
 * 229-240); a list that does not is refused with ASR_HIP_EINVAL when its plan is built. */
#define ASR_CONV16_F16 1
#define ASR_CONV16_BF16X3 2
#define ASR_CONV16_F16X2 3
#define ASR_CONV16_BF16X3_2ACC 4
size_t asr_hip_sparse_conv_packed_bytes(int mode, int kernel_size, int cin, int cout, int cout_b);
int asr_hip_sparse_conv_pack(asr_hip_context* ctx, int mode, const float* filters_dev, const float* filters_b_dev,
                             int kernel_size, int cin, int cout, int cout_b, void* packed_out_dev);
int asr_hip_sparse_conv_f16(asr_hip_context* ctx, const asr_sparse_conv_args* args, const void* packed_dev,
                            int out_is_f16);
int asr_hip_sparse_conv_bf16x3(asr_hip_context* ctx, const asr_sparse_conv_args* args, const void* packed_dev);
int asr_hip_sparse_conv_f16x2(asr_hip_context* ctx, const asr_sparse_conv_args* args, const void* packed_dev);
int asr_hip_sparse_conv_bf16x3_2acc(asr_hip_context* ctx, const asr_sparse_conv_args* args, const void* packed_dev);
/* f32 bits of the largest |element| of a [rows, cols] matrix with row stride ld (floats) into *out_dev */
int asr_hip_absmax_f32(asr_hip_context* ctx, const float* x_dev, int64_t rows, int cols, int64_t ld, uint32_t* out_dev);
/* Row-group plan: the neighbour list re-laid in the order the 16-bit kernels stream it -- per 16 consecutive
 * rows (row_perm order) the set of kernel slots in use and, slot by slot, the 16 neighbour indices.  Built once
 * per list and reused by every convolution over it (the U-Net runs ~10 per grid level); the kernels then need no
 * neighbour table in LDS and do no CSR parsing.  The plan owns its device memory; the arrays it was built from
 * must keep their contents while it is in use.  Per-pair importance (neighbors_importance) and neighbour-count
 * normalisation are served by the table-driven kernel, which ignores the plan. */
typedef struct asr_hip_conv_plan asr_hip_conv_plan;
int asr_hip_sparse_conv_plan_create(asr_hip_context* ctx, const int32_t* neighbors_index_dev,
                                    const uint8_t* neighbors_kernel_index_dev, const int64_t* neighbors_row_splits_dev,
                                    const int32_t* row_perm_dev, int64_t num_out, int kernel_size,
                                    asr_hip_conv_plan** plan_out);
void asr_hip_sparse_conv_plan_destroy(asr_hip_conv_plan* plan);
/* With context option "plan_arena" = 1 the plans created afterwards take their memory from an arena of the context
 * instead of owning it (no device allocation per plan); this call invalidates ALL of them at once and recycles the
 * memory (hosts that rebuild every plan per geometry, e.g. the one-scan sharding). */
int asr_hip_context_plan_arena_reset(asr_hip_context* ctx);
/* bytes of device memory a plan holds */
size_t asr_hip_sparse_conv_plan_bytes(const asr_hip_conv_plan* plan);
/* f32 <-> f16 conversion of an activation buffer (n elements) */
int asr_hip_convert_f16(asr_hip_context* ctx, const void* in_dev, int64_t n, void* out_dev, int to_f16);

/* MFMA tiling order for asr_hip_sparse_conv_f32: reorders the rows of a CSR inside segments of
 * `segment_rows` consecutive rows (0 = default) by their set of kernel slots, so that 16-row MFMA
 * tiles see few distinct slots. perm_out_dev [num_rows] goes into asr_sparse_conv_args.row_perm.
 * The order: rows stably by (row / segment_rows, slot mask, row), the mask being the OR of 1 << slot over the
 * row (an empty row: 0); then, with option row_lpt and more than 128 rows, the 128-row chunks of that order
 * stably by (128 c / segment_rows) * 128 + 127 - cost, cost = slots in the union of the chunk's first 64 rows
 * + the same for its second 64 rows, 0 for the partial last chunk.  Always a permutation; for segment_rows a
 * multiple of 128 every row stays inside its segment (tests/list_ops_ref.py).
 * The list goes through the routine that orders the 13 lists of a build, as a batch of one list sorted on the whole
 * mask, whatever option row_ranked says: any segment_rows (below 16: 16) and any num_rows below 2^31 - 127; with
 * row_lpt, EINVAL for 2^24 segments and more (the chunk key is 31 bits). */
int asr_hip_row_groups(asr_hip_context* ctx, const uint8_t* kernel_index_dev,
                       const int64_t* row_splits_dev, int64_t num_rows, int64_t segment_rows,
                       int32_t* perm_out_dev);

/* ---- a11: open3d::invert_neighbors_list (net_definitions_torch.py:22-36,548-559) -------- */
int asr_hip_invert_neighbors_list(asr_hip_context* ctx, int64_t num_points,
                                  const int32_t* inp_index_dev,
                                  const int64_t* inp_row_splits_dev, int64_t num_rows,
                                  const uint8_t* inp_attributes_dev, int32_t* out_index_dev,
                                  int64_t* out_row_splits_dev, uint8_t* out_attributes_dev);

/* ---- open3d::reduce_subarrays_sum (models/common_torch.py:127) -------------------------- */
/* gather_index may be NULL; otherwise out[i] = sum values[gather_index[p]] */
int asr_hip_reduce_subarrays_sum(asr_hip_context* ctx, const float* values_dev,
                                 const int32_t* gather_index_dev,
                                 const int64_t* row_splits_dev, int64_t num_rows,
                                 float* out_dev);

/* ---- a14: UNet5.decode with zero shifts + sdf scale
 *      (net_definitions_torch.py:655-666, cpp/lib/asr.cpp:324-336) ------------------------ */
/* w1 [h1, 3+c], b1 [h1], w2 [h2,h1], b2 [h2], w3 [2,h2] (torch Linear layout);
 * sizes may be NULL (no sdf scale). out [v,2].  c, h1, h2 in 1..64, else ASR_HIP_EINVAL. */
int asr_hip_decode_mlp(asr_hip_context* ctx, const float* code_dev, int64_t v, int c,
                       const float* w1_dev, const float* b1_dev, int h1, const float* w2_dev,
                       const float* b2_dev, int h2, const float* w3_dev,
                       const float* sizes_dev, float* out_dev);

/* ---- the implicit field at arbitrary points: UNet5.decode / decode_with_gradient at shifts
 *      (net_definitions_torch.py:655-686) ------------------------------------------------------- */
/* Row of the leaf that contains each position: leaf_keys_dev [num_leaves] sorted ascending, a leaf set that tiles the
 * root cube (grid 0 of a build, the leaves of asr_hip_octree_get).  The frame's key convention (asr_hip_point_keys):
 * c = floor(p * inv_voxel_size[21]) + offset per axis; a position is inside when all three c lie in [0, 2^21), and its
 * row is that of the leaf whose key is the key of (c >> (21 - l), l) at that leaf's level l.  Non-finite positions and
 * positions outside the cube get -1.  Memory-safe on any input; every row lies in [-1, num_leaves). */
int asr_hip_leaf_locate(asr_hip_context* ctx, const asr_octree_frame* frame, const uint64_t* leaf_keys_dev,
                        int64_t num_leaves, const float* positions_dev, int64_t m, int32_t* rows_out_dev);
/* decode at given shifts: values_out[i] = decode(shifts[i], code[rows[i]]) for the layer order
 * [s | code] -> h1 -> ReLU -> h2 -> ReLU -> 2 (weights as asr_hip_decode_mlp).  rows_dev NULL: row i; a row < 0 gives
 * NaN.  shifts_dev [m,3], any values.  sizes_dev (NULL: none): values_out[i,0] *= sizes[row].  grad_out_dev [m,3]
 * (NULL: not computed): decode_with_gradient's z1[:, :3] = d decode[:,0] / d shift (unscaled). */
int asr_hip_decode_mlp_at(asr_hip_context* ctx, const float* code_dev, int c, const int32_t* rows_dev,
                          const float* shifts_dev, int64_t m, const float* w1_dev, const float* b1_dev, int h1,
                          const float* w2_dev, const float* b2_dev, int h2, const float* w3_dev, const float* sizes_dev,
                          float* values_out_dev, float* grad_out_dev);
/* ---- per-point attributes (colour, intensity, a label probability) blended at arbitrary positions ------------------ */
/* For row j with position x and scale s = sizes[j], and k = 0, 1, ..., max_widen with R = s 2^k: the members are the points
 * with d = ((dx*dx+dy*dy)+dz*dz) < R*R (the predicate of asr_hip_multi_radius_search), each with the weight
 *     w = (min(R, 2 r)/max(R, 2 r))^2 * clamp((1 - d/R^2)^3, 0, 1)
 * -- that search's scale compatibility for size R times the window of asr_hip_aggregation_importance on d/R^2 (radii_dev
 * as given to the forward, before point_radius_scale).  With W_k = sum w, the row is sum(w a)/W_k of the first k whose
 * W_k >= min_weight (> 0); weight_out[j] = that W_k, widen_out[j] = k.  Rows without such a k, non-finite positions,
 * positions outside the frame's root cube and sizes that are not finite and > 0 get `fill`, weight 0 and widen -1.
 * A convex combination of the members' attributes, clamped per channel to the range of the members with w > 0 (rounding
 * never takes it out of their hull; a constant comes back exactly); non-finite attributes propagate.  The same inputs give
 * the same bits.
 * attributes_dev [n,c] with 1 <= c <= ASR_MAX_ATTRIBUTE_CHANNELS, out_dev [m,c]; weight_out_dev [m] and widen_out_dev [m]
 * may be NULL; n = 0 and m = 0 are valid; max_widen 0..126.  For mesh vertices, sizes are the voxel sizes of the grid-0
 * rows asr_hip_leaf_locate / asr_hip_implicit_query return.  One fused kernel on the context's stream, nothing sized by
 * the number of pairs; scratch (context arena): the search's point index plus 4 c' n bytes (c' = c rounded up to a power
 * of two).  The index build reads its per-level cell counts back, the blend itself is not waited for. */
#define ASR_MAX_ATTRIBUTE_CHANNELS 16
int asr_hip_point_attributes_at(asr_hip_context* ctx, const asr_octree_frame* frame, const float* points_dev,
                                const float* radii_dev, int64_t n, const float* attributes_dev, int c,
                                const float* positions_dev, const float* sizes_dev, int64_t m, int max_widen,
                                float min_weight, float fill, float* out_dev, float* weight_out_dev,
                                int8_t* widen_out_dev);
/* ---- comparing two surfaces: nearest point of another set, points sampled on a mesh (not in the reference) --------- */
/* index_out[j] = the i that minimises d2(i, j), sqdist_out[j] = that minimum, with
 *     d2(i, j) = ((px-qx)^2 + (py-qy)^2) + (pz-qz)^2 in f32 (the predicate arithmetic of asr_hip_multi_radius_search).
 * Exact: the result of a brute-force search over all n points with that formula; ties go to the smallest point index.
 * 1 <= n < 2^31 and 0 <= m < 2^31, else ASR_HIP_EINVAL; either output pointer may be NULL.  The frame only defines the
 * acceleration grid (as for asr_hip_knn_radius): queries may lie anywhere, outside the frame too, and still get the
 * exact answer (more slowly, the further from the points they are).  A query with a non-finite coordinate gets index -1
 * and distance +inf; non-finite POINTS are ASR_HIP_EINVAL.  Plain stores, no float atomics: the same inputs give the
 * same bits.  The index build reads its cell counts back; the search itself is not waited for. */
int asr_hip_nearest_point(asr_hip_context* ctx, const asr_octree_frame* frame, const float* points_dev, int64_t n,
                          const float* queries_dev, int64_t m, int32_t* index_out_dev, float* sqdist_out_dev);
/* num_samples points on a triangle mesh, area weighted, stratified and deterministic.  Triangle areas are f64 from the f32
 * corners, P their prefix sums, A the total.  Sample s takes u = (s + r0) A / S, the first triangle t with P[t] > u
 * (triangles without area are never chosen), the barycentric coordinates b1 = sqrt(r1) (1 - r2), b2 = sqrt(r1) r2 and the
 * point v0 + b1 (v1 - v0) + b2 (v2 - v0) in f32 without contraction (a triangle in a coordinate plane yields points
 * exactly in that plane).  r0, r1, r2 in [0, 1) are a counter-based hash of (seed, s, stream): no state,
 * the same bits for the same arguments.  normals_out_dev [S,3] (may be NULL): the unit normal of the sample's triangle,
 * (v1 - v0) x (v2 - v0) normalised; triangle_out_dev [S] (may be NULL): its index.
 * ASR_HIP_EINVAL: a corner index outside [0, num_vertices); num_samples > 0 with no triangles or with A == 0 (or not
 * finite).  num_samples == 0 is valid.  Reads the total area back before the sampling kernel is enqueued. */
int asr_hip_mesh_sample(asr_hip_context* ctx, const float* vertices_dev, int64_t num_vertices,
                        const int32_t* triangles_dev, int64_t num_triangles, int64_t num_samples, uint64_t seed,
                        float* points_out_dev, float* normals_out_dev, int32_t* triangle_out_dev);
/* ---- mesh simplification: octree vertex clustering with quadric placement (not in the reference).
 * Merges all vertices that share a cell of the frame's octree and places the merged vertex on the planes of the
 * triangles around it.  Count / fill pair like asr_hip_components_*; the contract, which tests/mesh_simplify_ref.py
 * restates in numpy:
 *   Cell of vertex i: its level is l_i = levels_dev[i], or `level` when levels_dev is NULL, and must lie in
 *     0..ASR_MAX_LEVEL (else ASR_HIP_EINVAL).  With c21 = floor(p * inv_voxel_size[21]) + offset per axis (f32, as in
 *     asr_hip_leaf_locate) the cell is c21 >> (21 - l_i) and its key the location code of (cell, l_i).  A vertex that
 *     is not finite or lies outside the root cube is ASR_HIP_EINVAL ("vertex outside the frame"), a triangle corner
 *     outside [0, num_vertices) is ASR_HIP_EINVAL ("out of range").
 *   Clusters: the distinct keys.  Cells of different levels are different clusters, even when one contains the other.
 *   Triangles: every corner is replaced by its cluster; a triangle with two equal corners is dropped; among the
 *     triangles with the same SET of three clusters (any orientation) the one with the smallest input index survives,
 *     with its own corner order; survivors keep the input order.
 *   Output vertices: the clusters that a surviving triangle references, in ascending key order.  vertex_map[i] is the
 *     output index of vertex i's cluster, -1 when no surviving triangle references it.
 *   Position of a cluster: a cluster of exactly one input vertex copies that vertex's bits.  All others, in f64: with
 *     s = 21 - l the cell centre is c = (((cell << s) - offset) + 0.5 * 2^s) * (double)voxel_size[21], the cell size
 *     h = voxel_size[l], and all coordinates are taken relative to c.  Every corner (t, j) of every INPUT triangle
 *     whose corner vertex lies in the cluster (triangles that collapse later too) contributes, with
 *     N = (p1 - p0) x (p2 - p0) of triangle t and only if |N| > 0:  A += N N^T / (2|N|),  b += -(N . p0) N / (2|N|).
 *     m is the plain mean of the cluster's vertices.  If tr A > 0: eps = 1e-3 tr(A) / 3 and x solves
 *     (A + eps I) x = -b + eps m; otherwise x = m.  x is clamped per axis to [-h/2, h/2]; the output is (float)(c + x).
 *   Determinism: no floating-point atomics; the corners of a cluster are summed in a fixed order and shape, so the
 *     same inputs give the same bits on every run.
 * num_vertices == 0 or num_triangles == 0 is valid and gives an empty result (the vertices are still checked).
 * Sizes < 2^31 vertices and < 2^31 / 3 triangles.  _count reads the cluster count and the error flags back once and
 * the two output sizes once; a count / fill pair ("Count / fill pairs" at the top).  vertex_map_out_dev [num_vertices]
 * may be NULL.
 * Clustering can create non-manifold edges and vertices (two sheets closer than a cell merge); the result is not
 * filtered -- running asr_hip_components_* afterwards is the caller's choice. */
int asr_hip_mesh_simplify_count(asr_hip_context* ctx, const asr_octree_frame* frame, const float* vertices_dev,
                                int64_t num_vertices, const int32_t* triangles_dev, int64_t num_triangles,
                                const int8_t* levels_dev, int level, int64_t* num_vertices_out,
                                int64_t* num_triangles_out);
int asr_hip_mesh_simplify_fill(asr_hip_context* ctx, float* vertices_out_dev, int32_t* triangles_out_dev,
                               int32_t* vertex_map_out_dev);
/* ---- mesh adjacency: edge table, topology report, Taubin smoothing (not in the reference).
 * The contract, which tests/mesh_adjacency_ref.py restates in numpy.  Shared by the three entry points:
 *   A triangle with two equal corner indices is DEGENERATE: it contributes no edges and is counted.  A corner outside
 *     [0, num_vertices) is ASR_HIP_EINVAL ("out of range").  Sizes < 2^31 vertices and < 2^31 / 3 triangles.
 *   Each of the sides (c0,c1), (c1,c2), (c2,c0) of a non-degenerate triangle is one USE of the undirected edge
 *     (lo, hi) = (min, max) of its ends; the use is FORWARD when it runs lo -> hi.
 *   EDGES are the distinct (lo, hi) pairs in ascending (lo, hi) order; per edge `uses` is the number of its uses and
 *     `forward` the number of forward ones.  An edge is BOUNDARY when uses == 1, NON-MANIFOLD when uses >= 3,
 *     INCONSISTENT when uses == 2 and forward != 1 (its two triangles disagree about the orientation), and a FEATURE
 *     edge when uses != 2.  A FEATURE VERTEX is an end of a feature edge.
 *
 * The edge table.  A count / fill pair ("Count / fill pairs" at the top): _count reads the number of edges and the
 * error flag back once.  edges_out_dev [E,2] = (lo, hi), uses_out_dev [E], forward_out_dev [E]; any of them may be NULL.
 * num_triangles == 0 gives E == 0.  Integers only: the same inputs give the same bits. */
int asr_hip_mesh_edges_count(asr_hip_context* ctx, const int32_t* triangles_dev, int64_t num_triangles,
                             int64_t num_vertices, int64_t* num_edges_out);
int asr_hip_mesh_edges_fill(asr_hip_context* ctx, int32_t* edges_out_dev, int32_t* uses_out_dev,
                            int32_t* forward_out_dev);
/* The topology report: every count comes from a device reduction, all are read back once.
 *   used_vertices       vertices referenced by a non-degenerate triangle
 *   triangles           non-degenerate triangles;  degenerate_triangles: the others
 *   edges, boundary_edges, nonmanifold_edges, inconsistent_edges: as defined above
 *   components          connected components of the used vertices under the edges
 *   boundary_loops      connected components of the graph formed by the boundary edges alone.  This is the number of
 *                       rims (holes and outer borders) when no vertex has more than two boundary edges; rims that touch
 *                       in a vertex count as one.
 *   euler               used_vertices - edges + triangles
 * A mesh is watertight when it has triangles and no boundary, non-manifold or inconsistent edge; its genus is then
 * (2 components - euler) / 2.  NOT detected: non-manifold VERTICES (several triangle fans that meet in one vertex
 * without sharing an edge); such a mesh can pass as edge manifold here. */
typedef struct asr_mesh_topology {
    int64_t num_vertices, used_vertices, triangles, degenerate_triangles, edges, boundary_edges, nonmanifold_edges,
        inconsistent_edges, components, boundary_loops, euler;
} asr_mesh_topology;
int asr_hip_mesh_topology(asr_hip_context* ctx, const int32_t* triangles_dev, int64_t num_triangles,
                          int64_t num_vertices, asr_mesh_topology* out);
/* Laplacian / Taubin smoothing.  N(i) is the set of distinct vertices that share an edge with vertex i, restricted by
 * `boundary`:
 *   0 free    every vertex uses all of its edge neighbours
 *   1 pinned  feature vertices do not move; the others use all neighbours
 *   2 along   a feature vertex uses only the far ends of its own feature edges (open rims and non-manifold seams are
 *             smoothed as curves and do not shrink into the surface); the others use all neighbours
 * A vertex with an empty N(i) does not move.  One step with factor f is, for all vertices at once and reading only
 * the previous positions,  p'_i = p_i + f (mean_{j in N(i)} p_j - p_i);  one iteration is a `lambda` step followed by
 * a `mu` step, mu == 0 means plain Laplacian smoothing (no second step).  Taubin's filter does not shrink the surface
 * when mu < -lambda (a little more negative than -lambda); the defaults everywhere are lambda = 0.5, mu = -0.53.
 * Positions are f64 between the steps; the neighbour sum (ascending neighbour index for rows of up to 128 entries; longer
 * rows as 64 interleaved partial sums added pairwise), the mean and the update are f64 without contraction, the output
 * is rounded to f32 once at the end.  A vertex that never moves gets its input bits; iterations == 0 copies the input.
 * No float atomics, every row is summed in a fixed order and shape: the same inputs give the same bits on every run.
 * vertices_out_dev [num_vertices,3] may equal vertices_dev.
 * ASR_HIP_EINVAL: iterations outside 0..1000, lambda not in (0, 1], mu not finite or > 0, boundary outside 0..2, a
 * vertex that is not finite (one check pass before any step, its flag read back once), a corner out of range.
 * Reads back the number of edges and, with the flags, the number of rows longer than 128 entries. */
int asr_hip_mesh_smooth(asr_hip_context* ctx, const float* vertices_dev, int64_t num_vertices,
                        const int32_t* triangles_dev, int64_t num_triangles, int iterations, double lambda, double mu,
                        int boundary, float* vertices_out_dev);
/* ---- hole filling: centroid fans over small boundary rims (not in the reference).
 * The contract, which tests/mesh_fill_ref.py restates in numpy; degenerate triangles, uses, forward and boundary edges
 * (uses == 1) are those of the mesh adjacency section above.
 *   The one use of a boundary edge runs a -> b inside its triangle: a is the edge's TAIL and b its HEAD (forward == 1
 *     means lo -> hi, otherwise hi -> lo).
 *   A RIM is a connected component of the graph of the boundary edges alone (what boundary_loops counts).  Its id is
 *     its smallest vertex index and its length n the number of its boundary edges.
 *   A rim is SIMPLE when each of its vertices is the tail of exactly one and the head of exactly one of its boundary
 *     edges: it is then one consistently directed cycle of n >= 3 vertices.  Rims that touch in a vertex, rims through
 *     a vertex with three or more boundary edges and rims whose triangles disagree about the orientation are not
 *     simple and are left alone.
 *   A rim is FILLED when it is simple and n <= max_edges.  max_edges must lie in 3..2^20 (else ASR_HIP_EINVAL): the
 *     outer border of an open scan is a rim too, and the cap is what keeps it open.
 *   Output vertices: the input vertices first, bits unchanged (unused ones stay), then one HUB per filled rim with
 *     n >= 4 in ascending rim id.  The hub is the mean of the rim's vertices: an f64 sum of the f32 coordinates in
 *     ascending vertex index (rims of up to 128 vertices sequentially; longer rims as the 64 interleaved partial sums,
 *     lane l taking the entries l, l + 64, ..., added pairwise xor 32, 16, ... 1, of asr_hip_mesh_smooth), divided by
 *     n in f64 without contraction and rounded once to f32.  No float atomics.
 *   Output triangles: all input triangles first, unchanged and in order (degenerate ones stay), then the new ones
 *     ordered by rim id and inside a rim by ascending tail a.  A rim with n >= 4 gets one triangle (b, a, hub) per
 *     boundary edge a -> b: it crosses the edge the other way, so the edge becomes a consistent 2-use edge.  A rim
 *     with n == 3 gets no hub and the one triangle (m, p, s): m is the rim id, p -> m and m -> s its boundary edges.
 *     (A mesh of a single triangle so becomes a two-sided pillow.)
 *   Report: rims (== boundary_loops of asr_hip_mesh_topology), filled, too_long (simple, n > max_edges), not_simple
 *     (whatever its length), new_vertices (hubs), new_triangles.  Every filled rim raises the Euler characteristic by
 *     exactly 1; an edge-manifold, oriented mesh with simple rims only and max_edges >= its longest rim comes out
 *     watertight.
 * A count / fill pair ("Count / fill pairs" at the top): _count reads the report, the sizes and the error flags back
 * once; _fill also copies the input arrays (the outputs must not overlap the inputs).
 * ASR_HIP_EINVAL: a corner out of range ("out of range"); a vertex ON A FILLED RIM that is not finite -- no other
 * vertex is read; a result that no longer fits the sizes above.  num_triangles == 0, or no boundary at all, copies the
 * input and gives a zero report.  The same inputs give the same bits on every run. */
typedef struct asr_mesh_fill_report {
    int64_t rims, filled, too_long, not_simple, new_vertices, new_triangles;
} asr_mesh_fill_report;
int asr_hip_mesh_fill_holes_count(asr_hip_context* ctx, const float* vertices_dev, int64_t num_vertices,
                                  const int32_t* triangles_dev, int64_t num_triangles, int64_t max_edges,
                                  int64_t* num_vertices_out, int64_t* num_triangles_out, asr_mesh_fill_report* report);
int asr_hip_mesh_fill_holes_fill(asr_hip_context* ctx, float* vertices_out_dev, int32_t* triangles_out_dev);
/* ---- point merge: one point per occupied octree cell (not in the reference).
 * Reduces a cloud before the reconstruction: all points that share a cell of the frame's octree become one point, the
 * mean of its members.  A count / fill pair ("Count / fill pairs" at the top); the contract, which tests/points_merge_ref.py
 * restates in numpy:
 *   Inputs: points_dev [n,3]; optional (NULL: absent) normals_dev [n,3], radii_dev [n] and attributes_dev [n,c] with
 *     1 <= c <= ASR_MAX_ATTRIBUTE_CHANNELS (c is ignored without attributes).  0 <= n < 2^31; n == 0 is valid and gives
 *     an empty result.
 *   Cell of point i: exactly the cell of asr_hip_mesh_simplify_*.  Its level is l_i = levels_dev[i], or `level` when
 *     levels_dev is NULL, and must lie in 0..ASR_MAX_LEVEL (else ASR_HIP_EINVAL); with c21 = floor(p *
 *     inv_voxel_size[21]) + offset per axis in f32 the cell is c21 >> (21 - l_i) and its key the location code of
 *     (cell, l_i).  A point that is not finite or lies outside the root cube is DROPPED, not an error (scanner output
 *     holds NaNs): it belongs to no cluster, its map entry is -1 and the report counts it.
 *   Side bit (split_sides = 1 only; needs normals, else ASR_HIP_EINVAL): r is the normal of the member of the cell with
 *     the smallest input index.  Member i has side 1 when (nx*rx + ny*ry) + nz*rz < 0, evaluated in f32 without
 *     contraction, otherwise side 0 (a NaN product gives side 0).  The two faces of a thin wall that share a cell so
 *     stay apart.  Without split_sides every side is 0.
 *   Clusters: the distinct (key, side) pairs, in ascending key order and side 0 before side 1.  Cells of different
 *     levels are different clusters, even when one contains the other.
 *   Per cluster, its members taken in ascending input index: counts_out_dev = their number (int32); position, radius
 *     and every attribute channel = the mean, summed in f64, divided by the count in f64 and rounded once to f32;
 *     normal = the f64 sum of the members' normals as given, divided by its f64 length sqrt((sx*sx + sy*sy) + sz*sz)
 *     -- when that length is 0 or not finite, the normal of the cluster's first member, bit for bit.  A cluster of
 *     exactly one member copies all of that member's bits.  Non-finite radii, normals and attributes propagate into
 *     their cluster; only positions decide dropping.
 *   Summation: a cluster of at most ASR_MERGE_LONG_CLUSTER members is one sequential f64 chain in ascending input
 *     index.  A longer one is summed by a workgroup of 256 threads: thread t adds the members t, t + 256, ... of the
 *     sorted member list in order, the 64 partial sums of each wave are added pairwise (xor 32, 16, ... 1), and the four
 *     wave sums as (w0 + w1) + (w2 + w3).  No floating-point atomics: the same inputs give the same bits on every run.
 *   Accuracy: an output value is the f32 rounding of a value within members * 2^-53 * max|x| of the exact mean, so it
 *     differs from the correctly rounded mean by at most 1 f32 ulp for clusters of up to 2^20 members whose mean is not
 *     cancelled (|mean| of the order of max|x|); the same holds for the normal when |sum n| >= 1e-3 sum |n|.
 *   A merged position is NOT guaranteed to fall back into its own cell: the f32 cell arithmetic is not convex to the
 *     last bit.  It lies in the cell's box within 2^-22 * max|corner| per axis.
 *   cluster_out_dev [n] (int32): the output index of each point's cluster, -1 for a dropped point.
 *   Report: clusters, dropped points, members of the largest cluster, cells that were split into two sides.
 * _count enqueues the key pass, one stable radix sort of (key, index) -- its last bit taken from `level`, all 64 bits
 * with levels_dev --, the side partition and the cluster scan, and reads the cluster count, the error flags and the
 * report back once; _fill runs the reduction.  Every output pointer of _fill, and report, may be NULL; an output whose
 * input was not given is not written. */
#define ASR_MERGE_LONG_CLUSTER 128
typedef struct asr_points_merge_report {
    int64_t clusters, dropped, largest_cluster, split_cells;
} asr_points_merge_report;
int asr_hip_points_merge_count(asr_hip_context* ctx, const asr_octree_frame* frame, const float* points_dev, int64_t n,
                               const float* normals_dev, const float* radii_dev, const float* attributes_dev, int c,
                               const int8_t* levels_dev, int level, int split_sides, int64_t* num_clusters_out,
                               asr_points_merge_report* report);
int asr_hip_points_merge_fill(asr_hip_context* ctx, float* points_out_dev, float* normals_out_dev, float* radii_out_dev,
                              float* attributes_out_dev, int32_t* counts_out_dev, int32_t* cluster_out_dev);

/* ---- oriented normals for clouds without them (not in the reference) ---------------------------------- */
/* Exact k-nearest-neighbour lists.  With d2(i, j) = ((px-qx)^2 + (py-qy)^2) + (pz-qz)^2 in f32 without contraction (the
 * arithmetic of asr_hip_nearest_point), row i of index_out_dev (int32 [n,k]) and sqdist_out_dev (f32 [n,k]) holds the k
 * smallest pairs (d2(i, j), j) in lexicographic order, ascending: the point itself is included, ties in distance go to the
 * smaller index -- the result of a brute-force search, for duplicated points and lattices too.  1 <= k <= 64 and
 * 1 <= n < 2^31, else ASR_HIP_EINVAL; rows of a cloud with n < k are padded with index -1 and distance +inf.  Non-finite
 * points are ASR_HIP_EINVAL.  The frame only defines the acceleration grid and must contain the points, as for
 * asr_hip_knn_radius.  Either output may be NULL.  Plain stores: the same inputs give the same bits.  The index build
 * reads its cell counts back; the search itself is not waited for. */
int asr_hip_knn_index(asr_hip_context* ctx, const asr_octree_frame* frame, const float* points_dev, int64_t n, int k,
                      int32_t* index_out_dev, float* sqdist_out_dev);
/* PCA normals over given lists (from asr_hip_knn_index or hand-made): index_dev int32 [n,k], 3 <= k <= 64; entries equal
 * to -1 are skipped, any other entry outside [0, n) is ASR_HIP_EINVAL (checked on the device).  Per point, all in f64 from
 * the f32 coordinates, in slot order (the same bits on every run): the mean of the m valid neighbours, then the six
 * centred sums divided by m (two passes); the symmetric 3 x 3 is diagonalised by cyclic Jacobi sweeps until its
 * off-diagonal elements are exactly zero.  eigenvalues_out_dev (f32 [n,3], may be NULL): the eigenvalues ascending,
 * negative rounding residues clamped to 0.  normals_out_dev (f32 [n,3]): the unit eigenvector of the smallest, rounded to
 * f32 and signed so that its component of largest magnitude is positive (ties: the lowest axis) -- a function of the list
 * alone.  ok_out_dev (u8 [n], may be NULL): 0, with the normal (0,0,0), when m < 3 or l1 <= 1e-10 l2 (coincident or
 * collinear neighbours, l2 == 0 included), else 1.  One launch, one read-back (the index check). */
int asr_hip_point_normals(asr_hip_context* ctx, const float* points_dev, int64_t n, const int32_t* index_dev, int k,
                          float* normals_out_dev, float* eigenvalues_out_dev, uint8_t* ok_out_dev);
/* Consistent signs.  report = {components, flipped, skipped, rounds}.  Points with a zero normal are skipped: never
 * flipped, members of no component, counted in `skipped`.  normals_out_dev (f32 [n,3]) may be normals_dev; flips_out_dev
 * (u8 [n], 1 = negated) may be NULL.
 * num_viewpoints 1 or n (viewpoints_dev f32 [1,3] or [n,3]): flip iff (nx (vx-px) + ny (vy-py)) + nz (vz-pz) < 0 in f32
 *   without contraction; index_dev may be NULL; components and rounds are 0.
 * num_viewpoints 0: Hoppe's propagation over the minimum spanning forest of the k-NN graph.
 *   Edges: every directed slot e = i k + s with j = index[i,s], j != i, j >= 0 and both normals non-zero, read as the
 *     undirected edge {i, j}; entries outside [0, n) other than -1 are ASR_HIP_EINVAL.  Weight w = max(0, 1 - |dot|) with
 *     dot = (nx_i nx_j + ny_i ny_j) + nz_i nz_j in f32 without contraction (bitwise symmetric); key = bits(w) << 32 | e,
 *     which needs n k < 2^32 (else ASR_HIP_EINVAL).  The keys are distinct, so the minimum spanning forest under them is
 *     unique.  A forest edge asks for opposite flips of its ends iff dot < 0; that fixes every sign relative to its tree.
 *   Each tree's sign: its member with the largest z (ties: the smallest index; -0 == +0) gets n_z >= 0; n_z == 0 there
 *     leaves the tree as propagated.
 *   Built by Boruvka rounds over a signed union-find (64-bit atomicMin per root, of a mutual pair the smaller root stays),
 *   flattened without read-write races: the result does not depend on scheduling.  One read-back per round; rounds = the
 *   rounds that hooked a root, at most ceil(log2 n) + 1. */
int asr_hip_normals_orient(asr_hip_context* ctx, const float* points_dev, const float* normals_dev, int64_t n,
                           const int32_t* index_dev, int k, const float* viewpoints_dev, int64_t num_viewpoints,
                           float* normals_out_dev, uint8_t* flips_out_dev, int64_t report[4]);

/* ---- rigid registration of two scans: point-to-plane / point-to-point ICP (not in the reference) ------ */
/* Sums of one linearised step.  ata: the upper triangle of the 6 x 6 normal matrix, row by row ((0,0) (0,1) .. (0,5)
 * (1,1) .. (5,5)); atb: its right-hand side; unknowns xi = (omega, v): a small rotation about `origin` and a translation.
 * mode: 1 = point-to-plane, 0 = point-to-point (three rows per pair); set by asr_hip_icp_step, read by _update. */
typedef struct asr_icp_sums {
    double ata[21];
    double atb[6];
    double sq_residual; /* sum of r^2 over all rows                     */
    double sq_distance; /* sum of |q - y|^2 over all pairs              */
    int64_t pairs;
    int32_t mode;
    int32_t reserved;
} asr_icp_sums;
typedef struct asr_icp_params {
    float max_distance;           /* the cap on a pair's distance: finite, > 0                        */
    int max_iterations;           /* 1..1000                                                          */
    double rotation_tolerance;    /* stop when |omega| <= this (radians) ...                          */
    double translation_tolerance; /* ... and |v| <= this; both >= 0                                   */
} asr_icp_params;
typedef struct asr_icp_report {
    int iterations; /* steps evaluated                                                                */
    int converged;  /* the last update was within both tolerances                                     */
    int degenerate; /* the last step's normal equations had no unique solution; the transform is that
                       of the step before                                                             */
    int64_t pairs;  /* of the LAST evaluated step, like rmse = sqrt(sq_distance / pairs) (0 without
                       pairs) and fitness = pairs / m (0 for m = 0)                                   */
    double rmse;
    double fitness;
} asr_icp_report;
/* One ICP step: pairs every source point with its nearest target point within max_distance and accumulates the normal
 * equations of the linearised alignment.  target_dev f32 [n,3], target_normals_dev f32 [n,3] or NULL (point-to-point),
 * source_dev f32 [m,3]; transform: 12 doubles, the rows (R | t) of a 3 x 4; origin: 3 doubles.  The frame has the role it
 * has for asr_hip_nearest_point: it only defines the acceleration grid of the TARGET.  Per source point p:
 *   q   = (float)(((R00 (double)px + R01 (double)py) + R02 (double)pz) + t0), qy and qz alike: f64, uncontracted, rounded once;
 *   y   = the target point that minimises d2 = ((dx dx + dy dy) + dz dz) in f32 (asr_hip_nearest_point's arithmetic) among
 *         those with d2 <= cap2 = max_distance * max_distance (f32); ties go to the smallest index: the result of a brute-
 *         force search with that restriction;
 *   no pair (index -1) when p or q is not finite, when no target point is within the cap, or, with normals, when the normal
 *         of y has a non-finite component or is (0,0,0);
 *   terms, f64 from the f32 values: u = q - o, v = y - o, n = the normal of y as given (not normalised),
 *         a = (u x n, n), r = (nx (ux-vx) + ny (uy-vy)) + nz (uz-vz); a pair adds a a^T to ata, a r to atb, r^2 to sq_residual
 *         and ((ux-vx)^2 + (uy-vy)^2) + (uz-vz)^2 to sq_distance.  Point-to-point: the three rows n = e_0, e_1, e_2 of a pair
 *         are added up in that order first (r_k = u_k - v_k; sq_residual == sq_distance).
 * The sums are added in a fixed order (queries in the Morton order of q, a fixed run per wave, partials folded in index
 * order; no float atomics): the same bits on every run and on a fresh context.  index_out_dev (int32 [m]) may be NULL.
 * ASR_HIP_EINVAL: sizes and non-finite target points as for asr_hip_nearest_point; max_distance not finite or <= 0; a non-
 * finite transform or origin.  m = 0 is valid and gives zero sums.  The index build reads its cell counts back, the sums
 * are the one read-back of the step itself. */
int asr_hip_icp_step(asr_hip_context* ctx, const asr_octree_frame* frame, const float* target_dev, int64_t n,
                     const float* target_normals_dev, const float* source_dev, int64_t m, const double transform[12],
                     const double origin[3], float max_distance, asr_icp_sums* sums_out, int32_t* index_out_dev);
/* Host only, no context: solves A xi = -b (A, b: ata, atb) by Cholesky in f64 and applies xi = (omega, v):
 *     R <- Rw R,   t <- Rw (t - o) + v + o,   Rw = I + sin|w|/|w| [w]x + (1 - cos|w|)/|w|^2 [w]x^2   (I for |w| < 1e-300).
 * xi_out (6 doubles) may be NULL.  Returns 0, or 1 = degenerate, with transform_inout untouched and xi_out zero: fewer
 * than 6 (mode 1) or 3 (mode 0) pairs, a non-finite sum, or a pivot <= 2^-52 trace(A); -1 for a NULL argument. */
int asr_hip_icp_update(const asr_icp_sums* sums, const double origin[3], double transform_inout[12], double xi_out[6]);
/* The ICP loop: the target's point index is built once; each iteration is asr_hip_icp_step at the current transform, its
 * read-back, asr_hip_icp_update and the stop test -- converged when |omega| <= rotation_tolerance and |v| <=
 * translation_tolerance after the update was applied, degenerate when the update says so -- at most max_iterations times.
 * origin[a] = (double)(2^20 - frame.offset[a]) * (double)frame.voxel_size[21], the centre of the frame's root cube.
 * The queries are sorted again in every iteration: the result is a pure function of the arguments.  ASR_HIP_EINVAL as for
 * asr_hip_icp_step, for max_iterations outside 1..1000 and tolerances that are negative or NaN. */
int asr_hip_register_points(asr_hip_context* ctx, const asr_octree_frame* frame, const float* target_dev, int64_t n,
                            const float* target_normals_dev, const float* source_dev, int64_t m,
                            const asr_icp_params* params, double transform_inout[12], asr_icp_report* report);

/* ---- global registration: FPFH descriptors, nearest descriptors, RANSAC (not in the reference) -------- */
/* The borders of the theta bins: (cos beta_b, sin beta_b), beta_b = -pi + 2 pi b / 11, b = 1..10, as f64 literals.  The
 * numpy restatement (tests/global_register_ref.py) carries the same literals. */
#define ASR_FPFH_BINS 11
#define ASR_FPFH_DIM 33
#define ASR_FPFH_THETA_TABLE                               \
    {                                                      \
        {-0.84125353283118109, -0.54064081745559778},      \
        {-0.41541501300188632, -0.90963199535451844},      \
        {0.14231483827328512, -0.98982144188093268},       \
        {0.6548607339452851, -0.75574957435425827},        \
        {0.95949297361449748, -0.2817325568414295},        \
        {0.95949297361449748, 0.2817325568414295},         \
        {0.6548607339452851, 0.75574957435425827},         \
        {0.14231483827328512, 0.98982144188093268},        \
        {-0.41541501300188616, 0.90963199535451855},       \
        {-0.84125353283118132, 0.54064081745559744},       \
    }
/* Fast point feature histograms over given lists.  points_dev, normals_dev f32 [n,3]; index_dev int32 [n,k], 3 <= k <= 64,
 * from asr_hip_knn_index or hand-made: entries equal to -1 are skipped, any other entry outside [0, n) is ASR_HIP_EINVAL
 * (checked on the device).  fpfh_out_dev f32 [n,33]; spfh_out_dev f32 [n,33] and ok_out_dev u8 [n] may be NULL.
 * All arithmetic is f64 from the f32 inputs, uncontracted, only + - * / sqrt; a sum of three products is (a + b) + c.
 *   Normals: nn = (nx nx + ny ny) + nz nz; a normal is USABLE when its components are finite and nn > 0, and is then used
 *     as n / sqrt(nn).  A point without a usable normal has ok = 0 and zero rows and is no neighbour of anyone.
 *   Pair (i, slot s), j = index[i,s]: d = p_j - p_i, d2 = (dx dx + dy dy) + dz dz, dist = sqrt(d2).  The pair is NEAR when
 *     j is neither -1 nor i, both normals are usable and 0 < dist < +inf.  a1 = n_i . d, a2 = n_j . d.  Darboux frame as in
 *     PCL: if |a1| < |a2|: u = n_j, n_t = n_i, d <- -d, phi = -a2 / dist; otherwise u = n_i, n_t = n_j, phi = a1 / dist.
 *     c = d x u (cx = dy uz - dz uy, ...), |c| = sqrt(c . c); the pair is VALID when it is near and |c| > 0.  v = c / |c|,
 *     w = u x v, alpha = v . n_t, x = u . n_t, y = w . n_t.
 *   Bins, 11 per feature, in the order theta | alpha | phi.  alpha and phi: clamp(floor((f + 1) * 5.5), 0, 10).  theta,
 *     the bin of atan2(y, x), without a transcendental function: with (cos_b, sin_b) of ASR_FPFH_THETA_TABLE and
 *     y'_b = y cos_b - x sin_b, ge_b = (y >= 0) || (y'_b >= 0) for b <= 5 and (y >= 0) && (y'_b >= 0) for b >= 6;
 *     bin = the number of b in 1..10 with ge_b.
 *   SPFH: spfh[i][b] = (float)((100.0 * count_b) / m) over the m valid pairs of row i; m = 0 gives zeros and ok = 0.
 *   FPFH (Open3D's form): acc[b] = sum over the NEAR slots of row i, in slot order, of (double)spfh[j][b] / d2.  Each of
 *     the three sub-histograms: total = its acc added over b ascending, scaled[b] = (100.0 * acc[b]) / total, or 0 when the
 *     total is 0.  fpfh[i][b] = (float)(scaled[b] + (double)spfh[i][b]).
 * Plain stores, no atomics on values: the same bits on every run.  Two launches and one read-back (the index check);
 * when spfh_out_dev is NULL the SPFH rows live in the context's scratch arena, which the call recycles either way. */
int asr_hip_point_fpfh(asr_hip_context* ctx, const float* points_dev, const float* normals_dev, int64_t n,
                       const int32_t* index_dev, int k, float* fpfh_out_dev, float* spfh_out_dev, uint8_t* ok_out_dev);
/* The exact nearest row of b_dev (f32 [n,dim]) for every row of a_dev (f32 [m,dim]); 1 <= dim <= 64, 1 <= n < 2^31,
 * 0 <= m < 2^31.  Per pair of rows, in f32 without contraction: s = 0; for c ascending: t = a_c - b_c; s = s + t * t.
 * The result is the smallest pair (s, j): ties go to the smaller j, as in a brute-force search.  A row of a with a
 * non-finite entry gets index -1 and distance +inf; a row of b with one is never chosen; without any usable row of b every
 * result is -1 / +inf.  index_out_dev int32 [m], sqdist_out_dev f32 [m]; either may be NULL.  The rows of b may be split
 * over workgroups, whose partial results meet in a 64-bit atomicMin of bits(s) << 32 | j: the result does not depend on
 * the order.  Recycles the scratch arena; not waited for. */
int asr_hip_feature_match(asr_hip_context* ctx, const float* a_dev, int64_t m, const float* b_dev, int64_t n, int dim,
                          int32_t* index_out_dev, float* sqdist_out_dev);
typedef struct asr_ransac_params {
    float max_distance;     /* an inlier's cap: finite, > 0                                   */
    int32_t reserved;
    double edge_ratio;      /* 0 < r <= 1: both edge lengths of a triple within that ratio     */
    int64_t num_hypotheses; /* 1 <= H <= 2^24                                                  */
    uint64_t seed;
} asr_ransac_params;
typedef struct asr_ransac_report {
    int64_t evaluated;       /* hypotheses that passed the tests and were scored               */
    int64_t best_hypothesis; /* -1 when none passed                                            */
    int64_t inliers;         /* of the best one                                                */
} asr_ransac_report;
/* RANSAC over given correspondences: hypotheses from triples, each scored over all correspondences.  source_dev f32 [m,3],
 * target_dev f32 [n,3], corr_dev int32 [c,2] of (source row, target row), 3 <= c < 2^31; a row outside its cloud is
 * ASR_HIP_EINVAL (checked on the device).  A correspondence with a non-finite point is never an inlier, and a triple with
 * one is rejected.
 *   Hypothesis h = 0 .. H-1, draw r = 0, 1, 2 (splitmix64, u64 wrap-around):
 *     z = seed + (3h + r + 1) * 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31;  draw = ((z >> 32) * c) >> 32.
 *   Rejected when two draws coincide, when for one of the edges (0,1), (0,2), (1,2) the f64 lengths ls (source) and lt
 *     (target), sqrt((dx dx + dy dy) + dz dz), fail ls >= r lt or lt >= r ls, or when a frame is degenerate.
 *   Frame of three points, f64: e1 = (p1 - p0) / |p1 - p0|, g = e1 x (p2 - p0), e3 = g / |g|, e2 = e3 x e1; degenerate
 *     unless both norms are > 0.  R[a][b] = (Ft[a][0] Fs[b][0] + Ft[a][1] Fs[b][1]) + Ft[a][2] Fs[b][2] with the columns
 *     e1, e2, e3; t[a] = t0[a] - ((R[a][0] s0x + R[a][1] s0y) + R[a][2] s0z), anchored at the first pair.
 *   Score: the number of correspondences whose source point, moved as asr_hip_icp_step moves it (f64, rounded once to
 *     f32), has d2 = ((dx dx + dy dy) + dz dz) <= cap2 = max_distance * max_distance to its partner, both in f32.
 *   The winner is the largest score, ties go to the smallest h (a 64-bit atomicMax of score << 32 | ~h): integers only,
 *     no summation order enters.
 * transform_out: 12 doubles, the rows of (R | t).  Returns 0; or 1 = no hypothesis passed, with transform_out untouched
 * and the report {0, -1, 0} -- the code ASR_HIP_EINVAL has too, told apart by asr_hip_last_error(), which is then empty.
 * ASR_HIP_EINVAL: sizes, a NULL argument, max_distance not finite or <= 0, edge_ratio outside (0, 1], H outside 1..2^24.
 * Recycles the scratch arena.  Two read-backs: the number of survivors, which shapes the scoring launch, and the result. */
int asr_hip_ransac_transform(asr_hip_context* ctx, const float* source_dev, int64_t m, const float* target_dev, int64_t n,
                             const int32_t* corr_dev, int64_t c, const asr_ransac_params* params, double transform_out[12],
                             asr_ransac_report* report);
/* (asr_hip_implicit_query, the whole-path query on the last forward, is declared after asr_hip_implicit_stage_ms) */

/* ---- whole path: the section of asr::ReconstructSurface between the pre-filter and the
 *      contouring (cpp/lib/asr.cpp:143-336) ---------------------------------------------- */
typedef struct asr_weight {
    const char* name;   /* state_dict name of UNet5, e.g. "sparseconv_encblock0.conv1a.kernel" */
    const float* data;  /* dev                                                                */
    int32_t ndim;
    int64_t shape[5];
} asr_weight;

typedef struct asr_implicit_params {
    float point_radius_scale; /* asr.hpp:55, default 1                                      */
    int octree_max_depth;     /* asr.hpp:63, default 21                                     */
    float bb_min[3];          /* bounding box handed to CreateOctreeFromPoints              */
    float bb_max[3];
    int scale_sdf;            /* 1: values[:,0] *= voxel_size (asr.cpp:334-336)             */
    int precision;            /* arithmetic of the 53 sparse convs: 0 = exact f32 MFMA (default),
                                 ASR_CONV16_F16 = f16 activations + weights (config C5),
                                 ASR_CONV16_BF16X3 = fp32-class result on the bf16 matrix cores (six MFMAs per
                                 product), ASR_CONV16_F16X2 = fp32-class result on the f16 matrix cores
                                 (three MFMAs per product, per-tensor power-of-two scaling),
                                 ASR_CONV16_BF16X3_2ACC = bf16x3 with a second accumulator for the
                                 small products (below the exact f32 kernel's error)                    */
} asr_implicit_params;

/* sizes of the structures built by the last asr_hip_implicit_* call */
typedef struct asr_implicit_sizes {
    int64_t num_points;
    int64_t num_nodes;
    int64_t num_voxels[ASR_NUM_GRIDS];
    int64_t num_pairs[ASR_NUM_GRIDS];
    int64_t num_agg_pairs;
} asr_implicit_sizes;

/* geometry half: octree, 5 grids, aggregation neighbours. Results stay in the context. */
int asr_hip_implicit_build(asr_hip_context* ctx, const float* points_dev,
                           const float* radii_dev, int64_t n,
                           const asr_implicit_params* params, asr_implicit_sizes* sizes);
/* network half: aggregate + unet + decode on the structures of the last build.
 * values_out_dev [num_voxels[0], 2]. */
int asr_hip_implicit_network(asr_hip_context* ctx, const float* points_dev,
                             const float* normals_dev, int64_t n, const asr_weight* weights,
                             int num_weights, const asr_implicit_params* params,
                             float* values_out_dev);
/* first stage of the network half alone (UNet5.aggregate, net_definitions_torch.py:640-653): "feats1" [V0, C] and the
 * per-pair "importance" of the last build, readable with asr_hip_implicit_get.  For hosts that run the U-Net themselves
 * (the one-scan sharding: every rank aggregates the whole cloud, then convolves the rows it owns). */
int asr_hip_implicit_aggregate(asr_hip_context* ctx, const float* points_dev, const float* normals_dev, int64_t n,
                               const asr_weight* weights, int num_weights, const asr_implicit_params* params);
/* both halves; values live in the context afterwards (asr_hip_implicit_get "values") */
int asr_hip_implicit_forward(asr_hip_context* ctx, const float* points_dev,
                             const float* normals_dev, const float* radii_dev, int64_t n,
                             const asr_weight* weights, int num_weights,
                             const asr_implicit_params* params, asr_implicit_sizes* sizes);
/* ---- one scan over several GPUs, inside the library (round 4; SURVEY 8(e), BASELINE config C4) ----------------------
 * The reference has no multi-device path (cpp/lib/asr.cpp:161-163 creates CPU tensors); what defines the halo is the
 * stencil of its operators: one face ring per 55-slot convolution on the same / child / parent level
 * (cpp/lib/grid.cpp:99-170) and parent <-> children for the transitions (cpp/lib/grid.cpp:206-242).
 *
 * asr_hip_implicit_forward_sharded: every rank holds the whole cloud.  Option "shard_geometry" (default -1 = 1 whenever
 * world > 1): 1 = octree, voxel keys and the one-entry-per-voxel up / down lists of the whole cloud on every rank (the
 * integer work ownership is derived from), 55-slot neighbour lists, row-group plans, aggregation search and continuous
 * conv for the voxels the rank owns only; 0 = geometry + aggregation of the whole cloud on every rank (replicated).
 * After a forward with per-rank geometry the context holds a PARTIAL build ("neighbors_*", "aggregation_*" of
 * asr_hip_implicit_get list the owned rows, sizes.num_pairs / num_agg_pairs are the rank's): asr_hip_implicit_network
 * and asr_hip_implicit_aggregate refuse it (ASR_HIP_EINVAL) until the next asr_hip_implicit_build.
 * The 53 sparse convolutions and the decoder run on the rows the rank OWNS (grid-0 voxels
 * cut into `world` contiguous ranges of their level-21 Morton order with equal pair counts, a coarser voxel belongs to
 * the owner of its first child), with one point-to-point exchange of the boundary rows of the input buffer (+ the
 * importance of those rows) before each convolution -- grouped with the MAX all-reduce of the f16x2 running maximum of that
 * buffer --, and an all-gather of the owned values at the end.  Per row the same kernel, plan-group arithmetic and summation order as on one GPU:
 * the values equal asr_hip_implicit_forward's bit for bit.
 *
 * Transport: a table of two collective primitives on DEVICE buffers, enqueued on (or synchronised with) `stream`.
 * asr_hip_shard_comm_rccl_* provides it over RCCL (librccl.so is loaded at run time); tests plug in a host-staged one.
 */
typedef struct asr_shard_comm {
    void* user;
    int rank, world;
    /* grouped point-to-point exchange: message i goes to / comes from peer[i]; all of one call may proceed
     * concurrently (ncclGroupStart .. ncclGroupEnd).  Buffers are device memory.  0 = ok. */
    int (*exchange)(void* user, int nsend, const int* send_peer, const void* const* send_buf, const size_t* send_bytes,
                    int nrecv, const int* recv_peer, void* const* recv_buf, const size_t* recv_bytes, void* stream);
    /* in-place MAX over the ranks of n uint32 values (f16x2 running maxima: non-negative f32 bit patterns) */
    int (*allreduce_max_u32)(void* user, uint32_t* buf_dev, size_t n, void* stream);
    /* optional (NULL: the two calls above, one after the other): both in ONE group -- the maximum of a convolution's
     * input tensor and the halo of that tensor are needed at the same moment, before the convolution starts */
    int (*exchange_and_max)(void* user, int nsend, const int* send_peer, const void* const* send_buf,
                            const size_t* send_bytes, int nrecv, const int* recv_peer, void* const* recv_buf,
                            const size_t* recv_bytes, uint32_t* max_buf_dev, size_t max_n, void* stream);
} asr_shard_comm;

/* RCCL transport.  unique_id_out / unique_id: the 128 bytes of ncclUniqueId (rank 0 creates, the host broadcasts). */
int asr_hip_shard_comm_rccl_unique_id(asr_hip_context* ctx, void* unique_id_out);
int asr_hip_shard_comm_rccl_create(asr_hip_context* ctx, const void* unique_id, int rank, int world,
                                   asr_shard_comm** comm_out);
void asr_hip_shard_comm_rccl_destroy(asr_shard_comm* comm);

typedef struct asr_shard_stats {
    int64_t owned_rows[ASR_NUM_GRIDS];
    int64_t halo_rows_recv[ASR_NUM_GRIDS]; /* 55-slot lists: rows received per application of the level's stencil */
    int64_t bytes_sent, bytes_received;    /* halo exchanges + stitch of the last forward                       */
    int64_t exchanges;                     /* grouped exchanges of the last forward                              */
    double exchange_seconds;               /* option "shard_timing": wall time of the exchanges, each bracketed by stream
                                              synchronisations (instrumented runs only; 0 otherwise)             */
} asr_shard_stats;

/* values_out_dev [num_voxels[0], 2] complete on every rank (NULL: stays in the context, "values") */
int asr_hip_implicit_forward_sharded(asr_hip_context* ctx, const asr_shard_comm* comm, const float* points_dev,
                                     const float* normals_dev, const float* radii_dev, int64_t n,
                                     const asr_weight* weights, int num_weights, const asr_implicit_params* params,
                                     asr_implicit_sizes* sizes, float* values_out_dev, asr_shard_stats* stats);
/* copies one of the arrays of the last build/forward into dst_dev (device to device).
 * name: "values", "feats1", "importance", "code",
 *       "voxel_keys<i>", "voxel_centers<i>", "voxel_sizes<i>", "neighbors_index<i>",
 *       "neighbors_kernel_index<i>", "neighbors_row_splits<i>", "up_neighbors_index<i>",
 *       "up_neighbors_kernel_index<i>", "up_neighbors_row_splits<i>",
 *       "aggregation_neighbors_index", "aggregation_neighbors_dist",
 *       "aggregation_row_splits", "aggregation_scale_compat", "nodes",
 *       "down_neighbors_{index,kernel_index,row_splits}<i>" (inverted up lists, rows = grid i+1),
 *       "tiling<i>", "tiling_up<i>", "tiling_down<i>" (int32 MFMA tiling orders of the three CSRs)
 * (the input_dict keys of cpp/lib/asr.cpp:159-312). nbytes returns the byte size; dst_dev may
 * be NULL to query only. */
int asr_hip_implicit_get(asr_hip_context* ctx, const char* name, void* dst_dev,
                         size_t* nbytes);
/* per-stage times (ms, hip events) of the last forward: [0] octree, [1] grids, [2] aggregation
 * search, [3] continuous conv, [4] unet, [5] decode, [6] geometry wall (octree start .. search
 * joined), [7] network wall.  With option "overlap" (default) the search runs on a second stream
 * concurrently with the grids: [2] is measured on that stream and [0]+[1]+[2] exceeds [6]. */
int asr_hip_implicit_stage_ms(asr_hip_context* ctx, float out_ms[8]);
/* The field of the last forward at positions_dev [m,3]: row = asr_hip_leaf_locate on grid 0 of that forward's frame,
 * s = (p - centre[row]) / size[row], values_out [m,2] = decode(s, code[row]) with values[:,0] *= size[row] when that
 * forward had scale_sdf; grad_out [m,3] (NULL: not computed) = d values[:,0] / d p inside the leaf (ReLU derivative 0
 * at 0).  Outside positions: NaN values and gradient, row -1.  rows_out [m] (NULL: not written).  The decoder weights
 * are looked up by name as in the forward.  Asynchronous on the context's stream; no device memory beyond the
 * caller's buffers.  At the centres of grid 0 the values are the forward's bits (released widths).  ASR_HIP_EINVAL
 * before a forward, after a build alone, after a failed forward and after a forward sharded over several ranks;
 * m = 0 is a no-op. */
int asr_hip_implicit_query(asr_hip_context* ctx, const float* positions_dev, int64_t m, const asr_weight* weights,
                           int num_weights, float* values_out_dev, float* grad_out_dev, int32_t* rows_out_dev);

#ifdef __cplusplus
}
#endif
#endif /* ASR_HIP_H */
