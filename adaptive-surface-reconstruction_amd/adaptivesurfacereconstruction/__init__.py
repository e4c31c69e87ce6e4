"""`adaptivesurfacereconstruction` drop-in for the hot-path part of the reference's pybind module
(cpp/pybind/module.cpp:279-491, re-exported by python/adaptivesurfacereconstruction/__init__.py).

Same function names, keyword defaults, numpy in / numpy out, ValueError for shape errors and
RuntimeError from the library.  Everything runs on the MI355X through libasr_hip.so (no CPU
fallback), including the "next" rows of SURVEY section 8: pre-filter, dual cells, contouring and
component filter.
"""
import numpy as np
import torch

from asr_hip import _lib, ops as _ops
from asr_hip._lib import AsrHipError  # noqa: F401

__version__ = _lib.load().asr_hip_version().decode() if True else None


def get_version_str():
    """cpp/pybind/module.cpp:284-286"""
    return __version__


def set_print_callback_function(print_callback, levels=(0, 1, 2, 3)):
    """asr::SetPrintCallbackFunction (cpp/lib/asr.hpp:29-34; C++ API of the reference, not in its pybind module):
    stage banners and messages of the library go to `print_callback(str)`"""
    _lib.set_print_callback_function(print_callback, levels)


def _f32(a, name, shape_msg, ndim, last=None):
    a = np.ascontiguousarray(a, dtype=np.float32)  # forcecast, module.cpp:59-61
    if a.ndim != ndim or (last is not None and a.shape[-1] != last):
        raise ValueError("%s must have shape %s" % (name, shape_msg))
    return a


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def get_third_party_notices():
    """cpp/pybind/module.cpp:287-289.  The reference returns the licence texts of the libraries linked into its
    binary (Eigen, libcuckoo, nanoflann, TBB, Open3D, PyTorch); none of those is linked into libasr_hip.so."""
    return ("libasr_hip.so links the ROCm runtime (HIP) and uses the header-only rocPRIM (MIT licence, "
            "Copyright (c) Advanced Micro Devices, Inc.).  PyTorch (BSD-3-Clause) provides device memory and "
            "torch.distributed on the host side.  No code of the reference implementation or of its "
            "third-party dependencies is included.")


class Octree:
    """Opaque handle returned by create_octree (module.cpp:282): owns the sorted node and leaf keys (GPU
    tensors) and the octree frame, so it stays valid however many trees are built afterwards."""

    def __init__(self, frame, nodes, leaves):
        self.frame = frame
        self.nodes = nodes
        self.leaves = leaves

    def __repr__(self):
        return "<Octree nodes=%d leaves=%d>" % (self.nodes.shape[0], self.leaves.shape[0])


def create_octree(points, radii, bb_min, bb_max, radius_scale=1.0, grow_steps=0, max_depth=21):
    """module.cpp:144-161,372-400 -> asr::CreateOctreeFromPoints (cpp/lib/octree.cpp:230-280)"""
    points = _f32(points, "points", "[N,3]", 2, 3)
    radii = _f32(radii, "radii", "[N]", 1)
    if radii.shape[0] != points.shape[0]:
        raise ValueError("radii must have shape [N]")
    if grow_steps < 0:
        raise ValueError("grow_steps must be >= 0")
    frame = _lib.frame_init(np.asarray(bb_min, np.float32), np.asarray(bb_max, np.float32))
    dev = torch.device("cuda")
    nodes, leaves = _ops.octree_build(frame, torch.from_numpy(points).to(dev),
                                      torch.from_numpy(radii).to(dev), radius_scale, max_depth, int(grow_steps))
    return Octree(frame, nodes, leaves)


def create_grids_from_octree(tree, num_levels, voxel_info_all_levels=False):
    """module.cpp:163-228,402-441 -> asr::CreateGridsFromOctree (cpp/lib/grid.cpp:245-314).
    Empty arrays are omitted from the dicts like in the reference."""
    result = []
    keys = tree.leaves
    for i in range(num_levels):
        d = {}
        up = None
        if i + 1 < num_levels:
            nxt, up_idx, up_kidx, up_rs = _ops.grid_coarsen(keys)
            up = (up_idx, up_kidx, up_rs)
        if i == 0 or voxel_info_all_levels:
            centers, sizes = _ops.voxel_info(tree.frame, keys)
            if keys.numel():
                d["voxel_keys"] = _u64(keys)
                d["voxel_centers"] = centers.cpu().numpy()
                d["voxel_sizes"] = sizes.cpu().numpy()
        idx, kidx, rs = _ops.grid_neighbors(keys)
        if idx.numel():
            d["neighbors_index"] = idx.cpu().numpy()
            d["neighbors_kernel_index"] = kidx.cpu().numpy()
        d["neighbors_row_splits"] = rs.cpu().numpy()
        if up is not None and up[0].numel():
            d["up_neighbors_index"] = up[0].cpu().numpy()
            d["up_neighbors_kernel_index"] = up[1].cpu().numpy()
            d["up_neighbors_row_splits"] = up[2].cpu().numpy()
        result.append(d)
        if up is not None:
            keys = nxt
    return result


def compute_aggregation_neighbors(tree, points, radii, voxel_centers, voxel_sizes):
    """asr::ComputeAggregationNeighborsAndScaleCompatibility (cpp/lib/nsearch.cpp:107-162); the
    reference keeps this internal to ReconstructSurface, models/v0/datareader.py:776-795 does the
    same with open3d.core.nns."""
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    idx, dist, rs, compat = _ops.multi_radius_search(tree.frame, t(points), t(radii),
                                                     t(voxel_centers), t(voxel_sizes))
    return {"aggregation_neighbors_index": idx.cpu().numpy(),
            "aggregation_neighbors_dist": dist.cpu().numpy(),
            "aggregation_row_splits": rs.cpu().numpy(),
            "aggregation_scale_compat": compat.cpu().numpy()}


def create_dual_vertex_indices(tree):
    """module.cpp:230-235,443-453 -> asr::CreateDualVertexIndices (cpp/lib/grid.cpp:450-459):
    uint64 [D,8] indices into the leaves, for any live tree (models/v0/datareader.py:224-243 keeps several)."""
    return _ops.dual_cells(tree.leaves.device, nodes=tree.nodes, leaves=tree.leaves).cpu().numpy().astype(np.uint64)


def create_triangle_mesh(values, dual_vertex_indices, node_positions, contouring_value_threshold=1.0):
    """asr::CreateTriangleMesh (cpp/lib/contouring.cpp:29-460), internal to ReconstructSurface in the
    reference (cpp/lib/asr.cpp:340-342): values [V,2], dual_vertex_indices [D,8], node_positions
    [V,3] -> {'vertices': f32[M,3], 'triangles': i32[T,3]}"""
    dev = torch.device("cuda")
    values = _f32(values, "values", "[V,2]", 2, 2)
    pos = _f32(node_positions, "node_positions", "[V,3]", 2, 3)
    duals = np.ascontiguousarray(dual_vertex_indices)
    if duals.ndim != 2 or duals.shape[1] != 8:
        raise ValueError("dual_vertex_indices must have shape [D,8]")
    duals = duals.astype(np.int64, copy=False) if duals.dtype != np.uint64 else duals.view(np.int64)
    if duals.size and (duals.min() < 0 or duals.max() >= values.shape[0]):
        raise ValueError("dual_vertex_indices out of range")
    v, t = _ops.contour(torch.from_numpy(values).to(dev), torch.from_numpy(duals).to(dev),
                        torch.from_numpy(pos).to(dev), contouring_value_threshold)
    return {"vertices": v.cpu().numpy(), "triangles": t.cpu().numpy()}


def _load_weights(weights):
    """state dict of the network (names of UNet5.state_dict()).  The reference loads the TorchScript
    file <resource dir>/model.pt (cpp/lib/asr.cpp:138-139); here: a dict, an .npz, or a torch file
    holding a state dict or a TorchScript module, by argument or as
    $ASR_RESOURCE_DIR/{model_weights.npz, model_weights.pt, model.pt}."""
    import os
    if weights is None:
        base = os.environ.get("ASR_RESOURCE_DIR", "")
        for cand in ("model_weights.npz", "model_weights.pt", "model.pt"):
            if base and os.path.exists(os.path.join(base, cand)):
                weights = os.path.join(base, cand)
                break
        if weights is None:
            raise RuntimeError("no network weights: pass weights=... or set ASR_RESOURCE_DIR to a directory "
                               "with model_weights.npz / model_weights.pt")
    if isinstance(weights, str):
        if weights.endswith(".npz"):
            with np.load(weights) as z:
                return {k: z[k] for k in z.files}
        try:  # the reference ships a TorchScript archive (model.pt, cpp/lib/asr.cpp:138-139)
            sd = torch.jit.load(weights, map_location="cpu")
        except RuntimeError:  # not a TorchScript archive: a pickled state dict
            sd = torch.load(weights, map_location="cpu")
        sd = dict(sd.state_dict()) if hasattr(sd, "state_dict") else dict(sd)
        return {k: v for k, v in sd.items() if isinstance(v, torch.Tensor)}
    return weights


def reconstruct_surface(points, normals=None, radii=np.empty((0,), np.float32), point_radius_scale=1.0,
                        density_percentile_threshold=10.0, point_radius_estimation_knn=24,
                        octree_max_depth=21, contouring_value_threshold=1.0,
                        keep_n_connected_components=2**63 - 1, minimum_component_size=3, *, weights=None,
                        precision="f32", vertex_normals=False, point_attributes=None, simplify=0, smooth=0,
                        fill_holes=0, thin=0.0, normal_k=16, viewpoint=None):
    """module.cpp:58-109,291-346 -> asr::ReconstructSurface (cpp/lib/asr.cpp:95-349): pre-filter,
    implicit values, dual contouring, component filter; every stage on the MI355X.
    `weights` (keyword only) replaces the reference's bundled model.pt, see _load_weights.
    `precision` (keyword only): arithmetic of the network's sparse convolutions, one of asr_hip._lib.PRECISIONS --
    "f32" (default, the reference's arithmetic), "bf16x3_2acc" (bf16 matrix cores, a third of the f32 arithmetic's
    rms error, half its U-Net time), "bf16x3", "f16x2" or "f16" (see asr_hip.pipeline.ImplicitPipeline).
    `vertex_normals` (keyword only): the result also holds "vertex_normals" f32 [V,3], the unit gradient of the
    network's field at every final vertex (ImplicitPipeline.query), zero where the gradient vanishes.
    `point_attributes` (keyword only): f32-convertible [num_points] or [num_points, C], e.g. the colours of the scan;
    the result then holds "vertex_attributes" f32 [V,C], the attributes of the inlier points blended at every final
    vertex at the scale of the leaf that contains it (ImplicitPipeline.transfer), 0 where no point is near.
    `simplify` (keyword only): k > 0 merges, after the component filter, all vertices inside one octree cell k levels
    above the leaf that contains them and places the merged vertex on the planes of the triangles around it
    (ImplicitPipeline.mesh); it runs before vertex_normals and point_attributes, which describe the final vertices.
    `smooth` (keyword only): n > 0 runs n iterations of Taubin smoothing (asr_hip.ops.mesh_smooth with its defaults:
    lambda 0.5, mu -0.53, rims smoothed along themselves) after the component filter and after simplify, also before
    vertex_normals and point_attributes.
    `fill_holes` (keyword only): m > 0 closes every simple boundary rim of at most m edges (3 <= m <= 2^20) with a fan
    around the mean of its vertices (asr_hip.ops.mesh_fill_holes), after simplify and before smooth; longer rims, the
    outer border of an open scan among them, stay open.
    `thin` (keyword only): a cell size s > 0 merges the cloud first, before the pre-filter, exactly as
    merge_points(points, normals, radii, point_attributes, cell_size=s) does: one point per occupied cell (and side) of
    the octree level whose voxel size lies in [s, 2 s).  Given radii and point_attributes are averaged alike; without
    given radii they are estimated on the merged cloud.  0 (default): the cloud is taken as it is.
    `normals` None: the cloud has no (or no oriented) normals and they are estimated, after `thin` and before the
    pre-filter, exactly as estimate_normals(points, normal_k, viewpoint) does; points without a usable estimate
    (ok == False) are dropped with their radii and attributes.  `normal_k` (keyword only, 3..64) and `viewpoint`
    (keyword only, [3], or [N,3] for the cloud as it is after thin; None: propagation) are ignored when normals are given."""
    from asr_hip.pipeline import ImplicitPipeline
    if normals is None:
        normal_k = _ops.check_normal_k(normal_k)
    thin = float(thin)
    if not (np.isfinite(thin) and thin >= 0):
        raise ValueError("thin must be a cell size >= 0 (0: off)")
    fill_holes = _ops.check_fill_arguments(fill_holes) if fill_holes != 0 else 0
    simplify = int(simplify)
    if simplify < 0:
        raise ValueError("simplify must be >= 0")
    smooth = int(smooth)
    if not 0 <= smooth <= 1000:
        raise ValueError("smooth must be a number of iterations in 0..1000")
    if precision not in _lib.PRECISIONS:
        raise ValueError("precision must be one of %s" % ", ".join(sorted(_lib.PRECISIONS)))
    points = _f32(points, "points", "[num_points,3]", 2, 3)
    if normals is not None:
        normals = _f32(normals, "normals", "[num_points,3]", 2, 3)
    radii = np.ascontiguousarray(radii, dtype=np.float32)
    if normals is not None and normals.shape != points.shape:
        raise ValueError("normals must have shape [num_points,3]")
    if normals is None and viewpoint is not None:
        viewpoint = _viewpoint(viewpoint, points.shape[0] if thin == 0 else None)
    if radii.ndim != 1 or radii.shape[0] not in (0, points.shape[0]):
        raise ValueError("radii must have shape [num_point3]")
    if point_attributes is not None:
        try:
            point_attributes = np.ascontiguousarray(point_attributes, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("point_attributes must be convertible to float32") from None
        if point_attributes.ndim == 1:
            point_attributes = point_attributes[:, None]
        if point_attributes.ndim != 2 or point_attributes.shape[0] != points.shape[0] or point_attributes.shape[1] < 1:
            raise ValueError("point_attributes must have shape [num_points] or [num_points, C]")
    if points.shape[0] == 0:
        raise RuntimeError("points is null!\n")
    if thin > 0:
        merged = merge_points(points, normals, radii if radii.shape[0] else None, point_attributes, cell_size=thin)
        points, normals, point_attributes = merged["points"], merged["normals"], merged["attributes"]
        if radii.shape[0]:
            radii = merged["radii"]
        if points.shape[0] == 0:
            raise RuntimeError("no points left after thinning")
    if normals is None:
        est = estimate_normals(points, normal_k, viewpoint)
        ok = est["ok"]
        points, normals = np.ascontiguousarray(points[ok]), np.ascontiguousarray(est["normals"][ok])
        if radii.shape[0]:
            radii = np.ascontiguousarray(radii[ok])
        if point_attributes is not None:
            point_attributes = np.ascontiguousarray(point_attributes[ok])
        if points.shape[0] == 0:
            raise RuntimeError("no points left after the normal estimation")
    # preprocess (asr.cpp:116-135)
    _lib.library_print("preprocessing\n", _lib.PRINT_LEVELS["INFO"])  # asr.cpp:117
    tree = KDTree(points)
    if radii.shape[0]:
        counts = _ops.radius_neighbor_count(tree._frame, tree._points, torch.from_numpy(radii).to(tree._points.device))
        inlier = _ops.density_inlier(counts.cpu().numpy(), density_percentile_threshold)
    else:
        r = _ops.knn_radius(tree._frame, tree._points, point_radius_estimation_knn)
        _, inl = _ops.knn_radius(tree._frame, tree._points, point_radius_estimation_knn, r, 0.5, 1,
                                 want_inlier=True)
        radii = r.cpu().numpy()
        inlier = inl.cpu().numpy().astype(bool)
    points, normals, radii = points[inlier], normals[inlier], radii[inlier]
    if point_attributes is not None:
        point_attributes = np.ascontiguousarray(point_attributes[inlier])
    if points.shape[0] == 0:
        raise RuntimeError("no points left after the pre-filter")
    dev = torch.device("cuda")
    pipe = ImplicitPipeline(_load_weights(weights), device="cuda:%d" % torch.cuda.current_device(),
                            point_radius_scale=point_radius_scale, octree_max_depth=octree_max_depth,
                            scale_sdf=True, precision=precision)
    # exact bounding box of the filtered points (asr.cpp:148-150; quirk B.1 applies)
    bb_min, bb_max = points.min(0), points.max(0)
    points_dev, radii_dev = torch.from_numpy(points).to(dev), torch.from_numpy(radii).to(dev)
    pipe.forward(points_dev, torch.from_numpy(normals).to(dev), radii_dev, bb_min, bb_max)
    v, t = pipe.mesh(contouring_value_threshold, keep_n_connected_components, minimum_component_size,
                     **({"simplify": simplify} if simplify else {}), **({"smooth": smooth} if smooth else {}),
                     **({"fill_holes": fill_holes} if fill_holes else {}))
    result = {"vertices": v.cpu().numpy(), "triangles": t.cpu().numpy()}
    if vertex_normals:
        _, grad = pipe.query(v, gradient=True)
        result["vertex_normals"] = _unit_normals(grad.cpu().numpy())
    if point_attributes is not None:
        result["vertex_attributes"] = pipe.transfer(points_dev, radii_dev, torch.from_numpy(point_attributes).to(dev),
                                                    v).cpu().numpy()
    return result


def _unit_normals(grad):
    """grad / |grad| per row as f32 [V,3]; zero rows where |grad| is 0 (or not finite)"""
    grad = np.asarray(grad, np.float32).reshape(-1, 3)
    norm = np.sqrt((grad * grad).sum(1, keepdims=True))
    ok = np.isfinite(norm) & (norm > 0)
    return np.where(ok, grad / np.where(ok, norm, np.float32(1)), np.float32(0)).astype(np.float32)


def remove_connected_components(vertices, triangles, keep_n_largest_components,
                                minimum_component_size=3):
    """module.cpp:111-142,348-370 -> asr::RemoveConnectedComponents (cpp/lib/postprocess.cpp:141-176)"""
    vertices = _f32(vertices, "vertices", "[N,3]", 2, 3)
    triangles = np.ascontiguousarray(triangles, dtype=np.int32)
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [N,3]")
    dev = torch.device("cuda")
    v, t = _ops.remove_components(torch.from_numpy(vertices).to(dev), torch.from_numpy(triangles).to(dev),
                                  keep_n_largest_components, minimum_component_size)
    return {"vertices": v.cpu().numpy(), "triangles": t.cpu().numpy()}


def _margin_frame(points):
    """the octree frame around points [N,3]: their bounding box and a margin of a thousandth of its longest side"""
    lo, hi = points.min(0), points.max(0)
    m = max(1e-3, 1e-3 * float((hi - lo).max()))
    return _lib.frame_init(lo - np.float32(m), hi + np.float32(m))


def _viewpoint(viewpoint, n):
    """viewpoint as f32 [3] or [n,3] (n None: any number of rows), or ValueError"""
    try:
        v = np.ascontiguousarray(viewpoint, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("viewpoint must be convertible to float32") from None
    if not (v.shape == (3,) or (v.ndim == 2 and v.shape[1] == 3 and (n is None or v.shape[0] == n))):
        raise ValueError("viewpoint must have shape [3] or [N,3]")
    if not np.isfinite(v).all():
        raise ValueError("viewpoint must be finite")
    return v


def estimate_normals(points, k=16, viewpoint=None):
    """Not in the reference's module.  Oriented normals for a cloud that has none, every stage on the
    GPU: the exact k nearest neighbours of every point, itself included (asr_hip.ops.knn_index, 3 <= k <= 64, in the
    octree frame around the bounding box with KDTree's margin), a PCA plane through them (ops.point_normals) and
    consistent signs (ops.orient_normals): towards `viewpoint` ([3], the scanner's position, or [N,3], one per point)
    or, with viewpoint None, propagated along the minimum spanning forest of the neighbour graph, each connected part
    signed so that its highest point looks up.  Non-finite points are a ValueError.
    -> {'normals': f32 [N,3] (zero where ok is False), 'ok': bool [N] (False: fewer than three or collinear neighbours),
    'eigenvalues': f32 [N,3] ascending, 'variation': f32 [N] = l0 / (l0 + l1 + l2) (0 where ok is False),
    'neighbors': int32 [N,k], 'report': dict of ints (components, flipped, skipped, rounds)}."""
    k = _ops.check_normal_k(k)
    points = _f32(points, "points", "[N,3]", 2, 3)
    n = points.shape[0]
    if n == 0:
        raise ValueError("points is empty")
    if not np.isfinite(points).all():
        raise ValueError("points must be finite")
    if viewpoint is not None:
        viewpoint = _viewpoint(viewpoint, n)
    frame = _margin_frame(points)
    dev = torch.device("cuda")
    p = torch.from_numpy(points).to(dev)
    index, _ = _ops.knn_index(frame, p, k)
    normals, eig, ok = _ops.point_normals(p, index, return_eigenvalues=True, return_ok=True)
    if viewpoint is None:
        normals, report = _ops.orient_normals(p, normals, index, return_report=True)
    else:
        normals, report = _ops.orient_normals(p, normals, viewpoints=torch.from_numpy(viewpoint).to(dev), return_report=True)
    eig, ok = eig.cpu().numpy(), ok.cpu().numpy()
    total = eig.sum(1, dtype=np.float32)
    good = ok & (total > 0)
    variation = np.where(good, eig[:, 0] / np.where(good, total, np.float32(1)), np.float32(0)).astype(np.float32)
    return {"normals": normals.cpu().numpy(), "ok": ok, "eigenvalues": eig, "variation": variation,
            "neighbors": index.cpu().numpy(), "report": report}


def simplify_mesh(vertices, triangles, cell_size, return_map=False):
    """Not in the reference's module.  Simplifies any triangle mesh by octree vertex clustering with quadric placement
    (asr_hip.ops.mesh_simplify): all vertices inside one cell of a regular grid become one vertex, placed on the planes
    of the triangles around it and kept inside the cell; triangles that collapse or repeat are dropped.  The grid is a
    level of the octree frame around the mesh's bounding box (with KDTree's margin): the deepest level whose voxel size
    is >= cell_size.  THE CELL ACTUALLY USED IS THAT VOXEL SIZE, between cell_size and twice cell_size (the root cube
    when cell_size exceeds it); it is returned as "cell_size".  The result may have non-manifold edges.
    -> {'vertices': f32 [V',3], 'triangles': i32 [T',3], 'cell_size': float, 'level': int}; return_map=True adds
    'vertex_map': int32 [V], the output vertex of every input vertex or -1."""
    vertices = _f32(vertices, "vertices", "[V,3]", 2, 3)
    triangles = np.ascontiguousarray(triangles, dtype=np.int32)
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [T,3]")
    cell_size = float(cell_size)
    if not (np.isfinite(cell_size) and cell_size > 0):
        raise ValueError("cell_size must be a positive number")
    if vertices.shape[0] == 0:
        raise ValueError("the mesh has no vertices")
    if not np.isfinite(vertices).all():
        raise ValueError("vertices must be finite")
    frame = _margin_frame(vertices)
    level = 0
    while level < _lib.ASR_MAX_LEVEL and frame.voxel_size[level + 1] >= cell_size:
        level += 1
    dev = torch.device("cuda")
    out = _ops.mesh_simplify(frame, torch.from_numpy(vertices).to(dev), torch.from_numpy(triangles).to(dev), level=level,
                             return_map=True)
    result = {"vertices": out[0].cpu().numpy(), "triangles": out[1].cpu().numpy(),
              "cell_size": float(frame.voxel_size[level]), "level": level}
    if return_map:
        result["vertex_map"] = out[2].cpu().numpy()
    return result


def merge_points(points, normals=None, radii=None, attributes=None, cell_size=None, radius_factor=None, split_sides=True):
    """Not in the reference's module.  Reduces a point cloud before the reconstruction (asr_hip.ops.points_merge): all
    points inside one octree cell become one point -- the mean position, radius and attributes ([N] or [N,C], C <= 16)
    of its members and their normalised normal sum.  Overlapping scans so stop doubling the density.  The octree frame
    is the one around the bounding box of the FINITE points (with KDTree's margin); points that are not finite are
    dropped.  Exactly one of
      cell_size      one grid for the whole cloud: the deepest level whose voxel size is >= cell_size.  THE CELL ACTUALLY
                     USED IS THAT VOXEL SIZE, between cell_size and twice cell_size (the root cube when cell_size exceeds
                     it); it is returned as "cell_size".
      radius_factor  (needs radii) point i is merged on the level the octree build selects for a point of radius
                     radius_factor * radii[i]: dense regions are thinned on finer cells than sparse ones.
    split_sides (ignored without normals): the members of a cell whose normal points against that of the cell's first
    member form a cluster of their own, so the two faces of a thin wall are not averaged into one.
    -> {'points': f32 [M,3], 'normals': f32 [M,3] or None, 'radii': f32 [M] or None, 'attributes': f32 [M,C] or None,
    'counts': int32 [M], 'cluster': int32 [N] (the output point of every input point, -1: dropped), 'report': dict of
    ints (clusters, dropped, largest_cluster, split_cells), 'cell_size': float or None (radius_factor)}."""
    if (cell_size is None) == (radius_factor is None):
        raise ValueError("give exactly one of cell_size and radius_factor")
    size = float(cell_size if cell_size is not None else radius_factor)
    if not (np.isfinite(size) and size > 0):
        raise ValueError("%s must be a positive number" % ("cell_size" if cell_size is not None else "radius_factor"))
    if radius_factor is not None and radii is None:
        raise ValueError("radius_factor needs radii")
    points = _f32(points, "points", "[N,3]", 2, 3)
    n = points.shape[0]
    if normals is not None:
        normals = _f32(normals, "normals", "[N,3]", 2, 3)
    if radii is not None:
        radii = _f32(radii, "radii", "[N]", 1)
    if attributes is not None:
        try:
            attributes = np.ascontiguousarray(attributes, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("attributes must be convertible to float32") from None
    split_sides = bool(split_sides) and normals is not None
    _ops.check_merge_arguments(points, normals, radii, attributes, 0, None, split_sides)
    finite = np.isfinite(points).all(1)
    if not finite.any():
        raise ValueError("no finite point")
    frame = _margin_frame(points[finite])
    dev = torch.device("cuda")
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    points_dev, radii_dev = t(points), t(radii)
    level, levels, used = None, None, None
    if cell_size is not None:
        level = 0
        while level < _lib.ASR_MAX_LEVEL and frame.voxel_size[level + 1] >= size:
            level += 1
        used = float(frame.voxel_size[level])
    else:
        # the level is the position of the key's marker bit (3 l); a point that will be dropped: level 0
        keys = _ops.point_keys(frame, points_dev, radii_dev * size, 1.0, _lib.ASR_MAX_LEVEL).cpu().numpy().view(np.uint64)
        lv = np.zeros(n, np.int8)
        for l in range(1, _lib.ASR_MAX_LEVEL + 1):
            lv[keys >= np.uint64(1 << (3 * l))] = l
        lv[~finite] = 0
        levels = torch.from_numpy(lv).to(dev)
    p2, n2, r2, a2, cluster, counts, report = _ops.points_merge(
        frame, points_dev, t(normals), radii_dev, t(attributes), level=level, levels=levels, split_sides=split_sides,
        return_map=True, return_counts=True, return_report=True)
    host = lambda a: None if a is None else a.cpu().numpy()  # noqa: E731
    return {"points": host(p2), "normals": host(n2), "radii": host(r2), "attributes": host(a2), "counts": host(counts),
            "cluster": host(cluster), "report": report, "cell_size": used}


def register_points(source, target, target_normals=None, init=None, max_distance=None, max_iterations=50,
                    rotation_tolerance=1e-7, translation_tolerance=None):
    """Not in the reference's module.  Rigid registration of one scan onto another by ICP on the GPU (DESIGN.md 4.16,
    asr_hip.ops.register_points): finds the rotation and translation that move `source` [M,3] into the coordinate frame
    of `target` [N,3], starting from `init` (a 4x4 or 3x4 rigid transform, default: the identity) -- a local method, the
    scans must overlap and be roughly aligned already.  Each iteration pairs every moved source point with its exact
    nearest target point within max_distance and solves the linearised alignment: point-to-plane when target_normals
    [N,3] are given (a few iterations), point-to-point without them (dozens).  Source points without a target point
    within max_distance take no part, so a partial overlap is fine.
      max_distance           None: 5 % of the diagonal of the target's bounding box
      translation_tolerance  None: 1e-7 of that diagonal; the loop stops once an update rotates by at most
                             rotation_tolerance (radians) and moves by at most translation_tolerance
    The octree frame is the one around the target's bounding box (with KDTree's margin); non-finite target points are a
    ValueError, non-finite source points take no part.
    -> {'transform': f64 [4,4], 'fitness': paired share of the source points, 'rmse': of the pairs' distances, both of
    the last evaluated step, 'iterations', 'converged', 'degenerate' (the pairs do not determine a rigid motion, e.g. a
    planar target in point-to-plane mode: the transform is the last determined one), 'pairs'}."""
    target = _f32(target, "target", "[N,3]", 2, 3)
    source = _f32(source, "source", "[M,3]", 2, 3)
    if target_normals is not None:
        target_normals = _f32(target_normals, "target_normals", "[N,3]", 2, 3)
    if target.shape[0] == 0:
        raise ValueError("target is empty")
    if not np.isfinite(target).all():
        raise ValueError("target points must be finite")
    diagonal = float(np.linalg.norm(target.max(0).astype(np.float64) - target.min(0).astype(np.float64)))
    if max_distance is None:
        max_distance = 0.05 * diagonal
    if translation_tolerance is None:
        translation_tolerance = 1e-7 * diagonal
    _ops.check_register_arguments(target, target_normals, source, max_distance, init, max_iterations, rotation_tolerance,
                                  translation_tolerance)
    frame = _margin_frame(target)
    dev = torch.device("cuda")
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    transform, report = _ops.register_points(frame, t(target), t(target_normals), t(source), max_distance, init,
                                             max_iterations, rotation_tolerance, translation_tolerance)
    report["transform"] = np.vstack([transform, [0.0, 0.0, 0.0, 1.0]])
    return report


def _global_cloud(points, normals, cell_size, feature_k, dev):
    """steps 1 and 2 of register_points_global and the lists of step 3 for one cloud -> dict: 'points', 'normals' (numpy,
    the merged cloud), 'pd' (the points on the GPU), 'index' (their feature_k nearest neighbours), 'cell' (the cell used),
    'estimated' (the normals were not given)"""
    merged = merge_points(points, normals, cell_size=cell_size)
    p, n = merged["points"], merged["normals"]
    if len(p) < 3:
        raise ValueError("fewer than 3 points are left after the merge: voxel_size is too large")
    if n is None:
        est = estimate_normals(p, k=16)
        p, n = p[est["ok"]], est["normals"][est["ok"]]
        if len(p) < 3:
            raise ValueError("fewer than 3 points have a usable normal estimate")
    pd = torch.from_numpy(p).to(dev)
    index, _ = _ops.knn_index(_margin_frame(p), pd, feature_k)
    return {"points": p, "normals": n, "pd": pd, "index": index, "cell": merged["cell_size"], "estimated": normals is None}


def _global_descriptors(cloud, dev, flip=False):
    """step 3 -> (the points that have a descriptor f32 [P,3], their FPFH rows as a GPU tensor [P,33]); flip: with the
    cloud's normals negated"""
    normals = torch.from_numpy(-cloud["normals"] if flip else cloud["normals"]).to(dev)
    fpfh, ok = _ops.point_fpfh(cloud["pd"], normals, cloud["index"], return_ok=True)
    return cloud["points"][ok.cpu().numpy()], fpfh[ok].contiguous()


def _global_pose(sp, sf, tp, tf, mutual, max_distance, hypotheses, seed, dev):
    """steps 4 and 5 -> (transform f64 [3,4] or None, the report of ransac_transform plus 'correspondences' and
    'mutual_used')"""
    if len(sp) < 3 or len(tp) < 3:
        raise ValueError("fewer than 3 points of a cloud have a descriptor")
    forth = _ops.feature_match(sf, tf)[0].cpu().numpy()
    rows = np.nonzero(forth >= 0)[0]
    corr = np.stack([rows, forth[rows]], 1).astype(np.int32)
    used = False
    if mutual:
        back = _ops.feature_match(tf, sf)[0].cpu().numpy()
        both = corr[back[corr[:, 1]] == corr[:, 0]]
        if len(both) >= 3:
            corr, used = both, True
    if len(corr) < 3:
        raise RuntimeError("register_points_global: fewer than 3 correspondences")
    transform, report = _ops.ransac_transform(torch.from_numpy(sp).to(dev), torch.from_numpy(tp).to(dev),
                                              torch.from_numpy(np.ascontiguousarray(corr)).to(dev), max_distance, 0.9,
                                              hypotheses, seed)
    return transform, dict(report, correspondences=int(len(corr)), mutual_used=used)


def register_points_global(source, target, source_normals=None, target_normals=None, voxel_size=None, feature_k=48,
                           max_distance=None, hypotheses=100000, seed=0, mutual=True, refine=True):
    """Not in the reference's module.  Registration of two scans that are NOT roughly aligned: a global
    search for the pose by FPFH descriptors and RANSAC, refined by register_points.  Every stage runs on the GPU and is a
    pure function of the arguments.
      1. merge_points(cell_size=voxel_size) on both clouds; voxel_size None: 1.5 % of the diagonal of the target's bounding
         box.  The cell used is the voxel size of an octree level (between voxel_size and twice it), per cloud;
         'cell_size' reports the larger of the two.
      2. normals as given, averaged by the merge; without them estimate_normals(k=16) on the merged cloud (points without a
         usable estimate are dropped).  ESTIMATED normals get their sign per cloud from its highest point, so two scans
         in different poses may get opposite signs, which the descriptors do not survive: when a cloud's normals were
         estimated, steps 3 to 5 run a second time with the source's normals negated and the pose with more inliers is
         kept (a tie: the first; 'normals_flipped' says which).  A cloud whose estimate falls into several separately
         signed parts is not covered by that: give oriented normals then.
      3. asr_hip.ops.knn_index(feature_k) and ops.point_fpfh on both; points without a descriptor are left out.
      4. ops.feature_match source -> target and, with mutual, target -> source: the pairs that choose each other; if fewer
         than 3 remain, all source -> target pairs are used ('mutual_used' False).
      5. ops.ransac_transform(max_distance, edge_ratio 0.9, hypotheses, seed); max_distance None: 1.5 x the cell used.
      6. with refine: register_points(source, target, target_normals, init=that transform) on the clouds as given.
    The method does not resolve near-symmetric shapes: on a smooth surface with a partial overlap the search returned the
    180-degree flip.  RuntimeError when no hypothesis passes the tests.
    -> register_points' dict ('transform' f64 [4,4], 'fitness', 'rmse', 'iterations', 'converged', 'degenerate', 'pairs';
    without refine the transform is RANSAC's and the other fields are 0 / False) plus 'global': {'cell_size',
    'correspondences', 'mutual_used', 'normals_flipped', 'evaluated', 'best_hypothesis', 'inliers', 'transform' f64 [4,4]
    (RANSAC's)}."""
    source = _f32(source, "source", "[M,3]", 2, 3)
    target = _f32(target, "target", "[N,3]", 2, 3)
    if source_normals is not None:
        source_normals = _f32(source_normals, "source_normals", "[M,3]", 2, 3)
    if target_normals is not None:
        target_normals = _f32(target_normals, "target_normals", "[N,3]", 2, 3)
    _ops.check_global_register_arguments(source, target, source_normals, target_normals, voxel_size, feature_k,
                                         max_distance, hypotheses, seed)
    finite = target[np.isfinite(target).all(1)]
    if len(finite) == 0:
        raise ValueError("target has no finite point")
    if voxel_size is None:
        voxel_size = 0.015 * float(np.linalg.norm(finite.max(0).astype(np.float64) - finite.min(0).astype(np.float64)))
        if not voxel_size > 0:
            raise ValueError("the target's bounding box is a point: give voxel_size")
    dev = torch.device("cuda")
    s_cloud = _global_cloud(source, source_normals, voxel_size, feature_k, dev)
    t_cloud = _global_cloud(target, target_normals, voxel_size, feature_k, dev)
    cell = max(s_cloud["cell"], t_cloud["cell"])
    if max_distance is None:
        max_distance = 1.5 * cell
    tp, tf = _global_descriptors(t_cloud, dev)
    transform, report, flipped = None, None, False
    for flip in (False, True) if s_cloud["estimated"] or t_cloud["estimated"] else (False,):
        sp, sf = _global_descriptors(s_cloud, dev, flip)
        try:
            pose, rep = _global_pose(sp, sf, tp, tf, mutual, max_distance, hypotheses, seed, dev)
        except (RuntimeError, ValueError):
            if report is None:
                raise
            continue  # the second pass found nothing to work with: the first one's pose stands
        if report is None or (pose is not None and (transform is None or rep["inliers"] > report["inliers"])):
            transform, report, flipped = pose, rep, flip
    if transform is None:
        raise RuntimeError("register_points_global: no hypothesis passed the edge-length and degeneracy tests")
    transform = np.vstack([transform, [0.0, 0.0, 0.0, 1.0]])
    info = dict(report, cell_size=float(cell), normals_flipped=flipped, transform=transform)
    if refine:
        result = register_points(source, target, target_normals, init=transform)
    else:
        result = {"iterations": 0, "converged": False, "degenerate": False, "pairs": 0, "rmse": 0.0, "fitness": 0.0,
                  "transform": transform.copy()}
    result["global"] = info
    return result


def transform_points(points, transform, normals=None):
    """Applies a rigid transform (4x4 or 3x4, as register_points returns it) to points [N,3] with the arithmetic of the
    registration itself: every coordinate is ((R0 x + R1 y) + R2 z) + t in f64, rounded once to f32.  Normals are rotated
    only.  -> points f32 [N,3], or (points, normals) when normals are given."""
    t = _ops._transform12(transform)
    points = _f32(points, "points", "[N,3]", 2, 3)
    p = points.astype(np.float64)
    moved = (((t[:, 0] * p[:, 0:1] + t[:, 1] * p[:, 1:2]) + t[:, 2] * p[:, 2:3]) + t[:, 3]).astype(np.float32)
    if normals is None:
        return moved
    normals = _f32(normals, "normals", "[N,3]", 2, 3)
    if normals.shape[0] != points.shape[0]:
        raise ValueError("normals must have shape [N,3]")
    n = normals.astype(np.float64)
    return moved, ((t[:, 0] * n[:, 0:1] + t[:, 1] * n[:, 1:2]) + t[:, 2] * n[:, 2:3]).astype(np.float32)


def smooth_mesh(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, boundary="along"):
    """Not in the reference's module.  Taubin smoothing of any triangle mesh (asr_hip.ops.mesh_smooth): `iterations`
    times a step p += lam (mean of the edge neighbours - p) and the same step with mu < -lam, which undoes the shrinking
    of the first (mu = 0: plain Laplacian smoothing).  boundary: "free", "pinned" (the ends of boundary and non-manifold
    edges stay) or "along" (they move along their own rim or seam only).
    -> {'vertices': f32 [V,3], 'triangles': i32 [T,3]}; the triangles are the input's."""
    iterations, lam, mu, _ = _ops.check_smooth_arguments(iterations, lam, mu, boundary)
    vertices = _f32(vertices, "vertices", "[V,3]", 2, 3)
    triangles = np.ascontiguousarray(triangles, dtype=np.int32)
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [T,3]")
    dev = torch.device("cuda")
    v = _ops.mesh_smooth(torch.from_numpy(vertices).to(dev), torch.from_numpy(triangles).to(dev), iterations, lam, mu,
                         boundary)
    return {"vertices": v.cpu().numpy(), "triangles": triangles}


def fill_mesh_holes(vertices, triangles, max_edges):
    """Not in the reference's module.  Closes the small holes of any triangle mesh (asr_hip.ops.mesh_fill_holes): every
    simple boundary rim of at most `max_edges` edges (3..2^20) gets a hub vertex at the mean of its vertices and one
    triangle per rim edge (a rim of three edges: one triangle, no hub).  Longer rims, rims that touch in a vertex and rims
    whose triangles disagree about the orientation stay open.
    -> {'vertices': f32 [V + hubs,3], 'triangles': i32 [T + new,3], 'rims', 'filled', 'too_long', 'not_simple',
    'new_vertices', 'new_triangles': int}; the input vertices and triangles come first, unchanged."""
    max_edges = _ops.check_fill_arguments(max_edges)
    vertices = _f32(vertices, "vertices", "[V,3]", 2, 3)
    triangles = np.ascontiguousarray(triangles, dtype=np.int32)
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [T,3]")
    dev = torch.device("cuda")
    v, t, report = _ops.mesh_fill_holes(torch.from_numpy(vertices).to(dev), torch.from_numpy(triangles).to(dev), max_edges,
                                        return_report=True)
    return {"vertices": v.cpu().numpy(), "triangles": t.cpu().numpy(), **report}


def mesh_topology(triangles, num_vertices=None):
    """Not in the reference's module.  What kind of mesh is this (asr_hip.ops.mesh_topology) -> dict of Python ints and
    bools: num_vertices, used_vertices, triangles, degenerate_triangles, edges, boundary_edges, nonmanifold_edges,
    inconsistent_edges, components, boundary_loops, euler, edge_manifold, oriented, watertight, genus (None unless
    watertight).  num_vertices None: triangles.max() + 1."""
    triangles = np.ascontiguousarray(triangles, dtype=np.int32)
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [T,3]")
    if num_vertices is None:
        num_vertices = int(triangles.max()) + 1 if triangles.size else 0
    if int(num_vertices) < 0:
        raise ValueError("num_vertices must be >= 0")
    return _ops.mesh_topology(torch.from_numpy(triangles).to(torch.device("cuda")), int(num_vertices))


class KDTree:
    """cpp/pybind/module.cpp:237-277,455-489 -> asr::KDTree (cpp/lib/nsearch.cpp:23-105).  The
    reference builds a nanoflann tree; here the points are Morton sorted on the GPU and all three
    queries are exact grid searches (asr_hip_knn_radius / asr_hip_radius_neighbor_count)."""

    def __init__(self, points):
        points = np.ascontiguousarray(points, dtype=np.float32)
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError("points must have shape [N,3]")
        self._points = torch.from_numpy(points).to(torch.device("cuda"))
        self._frame = _margin_frame(points)

    def compute_k_radius(self, k):
        return _ops.knn_radius(self._frame, self._points, k).cpu().numpy()

    def compute_inlier(self, radii, radius_fraction=0.5, k=24, outlier_threshold=1):
        radii = np.ascontiguousarray(radii, dtype=np.float32)
        if radii.ndim != 1 or radii.shape[0] != self._points.shape[0]:
            raise ValueError("radii must have shape [num_points]")
        _, inl = _ops.knn_radius(self._frame, self._points, k, torch.from_numpy(radii).to(self._points.device),
                                 radius_fraction, outlier_threshold, want_inlier=True)
        return inl.cpu().numpy()

    def compute_radius_neighbors(self, radii):
        radii = np.ascontiguousarray(radii, dtype=np.float32)
        cnt = _ops.radius_neighbor_count(self._frame, self._points,
                                         torch.from_numpy(radii).to(self._points.device))
        return [int(c) for c in cnt.cpu().tolist()]

    def knn(self, k):
        """Not in the reference's module.  The k nearest points of every point of the tree, itself included, exactly
        (brute-force result in f32, rows ordered by (squared distance, index); 1 <= k <= 64, rows of a tree with fewer
        than k points are padded with -1 and inf) -> (index int32 [N,k], squared distance f32 [N,k])"""
        idx, sq = _ops.knn_index(self._frame, self._points, k)
        return idx.cpu().numpy(), sq.cpu().numpy()

    def nearest(self, queries):
        """Not in the reference's module.  For each query [M,3] the nearest point of the tree, exactly (brute-force
        result in f32, ties to the smallest index; queries may lie anywhere, a non-finite one gets -1 and inf)
        -> (index int32 [M], distance f32 [M])"""
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        if queries.ndim != 2 or queries.shape[1] != 3:
            raise ValueError("queries must have shape [M,3]")
        idx, sq = _ops.nearest_point(self._frame, self._points, torch.from_numpy(queries).to(self._points.device))
        return idx.cpu().numpy(), np.sqrt(sq.cpu().numpy())


def default_thresholds(reference_points):
    """0.5 % and 1 % of the diagonal of the reference's bounding box: the F-score thresholds used when none are given"""
    p = np.asarray(reference_points, np.float64).reshape(-1, 3)
    diag = float(np.linalg.norm(p.max(0) - p.min(0)))
    return (0.005 * diag, 0.01 * diag)


def evaluate_mesh(vertices, triangles, reference_points=None, reference_normals=None, reference_mesh=None,
                  num_samples=1_000_000, thresholds=None, seed=0):
    """Not in the reference's module.  How far is the mesh from a reference surface: accuracy, completeness, Chamfer
    (L1, L2), Hausdorff, precision / recall / F-score per threshold and -- when the reference has normals -- normal
    consistency, between num_samples area-weighted samples of the mesh and either `reference_points` [N,3] (with
    optional unit `reference_normals`) or num_samples samples of `reference_mesh` = (vertices, triangles).
    Definitions: asr_hip.metrics.  thresholds None: 0.5 % and 1 % of the diagonal of the reference's bounding box
    (its points, or the vertices of its mesh).  -> dict of Python floats (lists of floats per threshold)."""
    from asr_hip import metrics as _metrics
    vertices = _f32(vertices, "vertices", "[V,3]", 2, 3)
    triangles = np.ascontiguousarray(triangles, dtype=np.int32)
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [T,3]")
    if (reference_points is None) == (reference_mesh is None):
        raise ValueError("give exactly one of reference_points and reference_mesh")
    dev = torch.device("cuda")
    if reference_mesh is not None:
        rv = _f32(reference_mesh[0], "reference_mesh vertices", "[V,3]", 2, 3)
        rt = np.ascontiguousarray(reference_mesh[1], dtype=np.int32)
        if rt.ndim != 2 or rt.shape[1] != 3:
            raise ValueError("reference_mesh triangles must have shape [T,3]")
        box, reference = rv, (torch.from_numpy(rv).to(dev), torch.from_numpy(rt).to(dev))
    else:
        rp = _f32(reference_points, "reference_points", "[N,3]", 2, 3)
        rn = None
        if reference_normals is not None:
            rn = _f32(reference_normals, "reference_normals", "[N,3]", 2, 3)
            if rn.shape != rp.shape:
                raise ValueError("reference_normals must have shape [N,3]")
            rn = torch.from_numpy(rn).to(dev)
        box, reference = rp, (torch.from_numpy(rp).to(dev), rn)
    if box.shape[0] == 0:
        raise ValueError("the reference is empty")
    if thresholds is None:
        thresholds = default_thresholds(box)
    return _metrics.mesh_metrics(torch.from_numpy(vertices).to(dev), torch.from_numpy(triangles).to(dev), reference,
                                 int(num_samples), tuple(float(t) for t in thresholds), seed=int(seed))
