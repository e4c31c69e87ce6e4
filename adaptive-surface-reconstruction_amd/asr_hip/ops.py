"""Per-stage operators on GPU torch tensors, thin wrappers over the C ABI (include/asr_hip.h).

Names and argument meaning follow the reference interfaces they stand in for:
  create_octree / create_grids_from_octree  -> cpp/pybind/module.cpp:144-228
  multi_radius_search                        -> cpp/lib/nsearch.cpp:107-162
  continuous_conv / sparse_conv / invert_neighbors_list / reduce_subarrays_sum
                                             -> open3d.ml.torch.ops used by models/common_torch.py
"""
import contextlib
import ctypes

import torch

from . import _lib
from ._lib import AsrHipError, Context, ptr

_ctx = {}  # device index -> Context


def context(device=None):
    """the process-wide context of `device` (default: torch's current device), on torch's current
    stream of that device.  One context per GPU: a context is bound to the device it was created on."""
    if device is None:
        index = torch.cuda.current_device()
    else:
        device = torch.device(device)
        index = device.index if device.index is not None else torch.cuda.current_device()
    ctx = _ctx.get(index)
    if ctx is None:
        with torch.cuda.device(index):
            ctx = _ctx[index] = Context()
    ctx.set_stream(torch.cuda.current_stream(index))
    return ctx


@contextlib.contextmanager
def fresh_context(device=None):
    """`with fresh_context(device) as ctx`: the operators of this module (and what is built on them, KDTree for one) run
    on a new context inside the block -- no option set, no table grown, nothing cached by an earlier call.  The block's
    context is closed at its end and the device's earlier one, untouched meanwhile, serves again."""
    if device is not None and torch.device(device).index is not None:
        index = torch.device(device).index
    else:
        index = torch.cuda.current_device()
    old = _ctx.pop(index, None)
    try:
        yield context(index)
    finally:
        torch.cuda.synchronize(index)
        new = _ctx.pop(index, None)
        if new is not None:
            new.close()
        if old is not None:
            _ctx[index] = old


def _dev(t, dtype):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if not t.is_cuda:
        raise AsrHipError("expected a GPU tensor: the HIP path has no CPU fallback")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _same_device(*tensors):
    """all tensors of one call must live on one GPU; returns that device"""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise AsrHipError("tensors on different devices (%s and %s) in one call" % (dev, t.device))
    return dev


def _rows(t, aligned=True):
    """a float32 matrix as the kernels read it: rows of unit-stride floats, any row stride.  A column slice of a wider
    buffer is read in place (zero-copy concat) when the MFMA kernel can take it as it is -- aligned: it starts on a
    16-byte boundary and its row stride is a multiple of 4 floats; everything else is made contiguous, as before"""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] > 1 and t.stride(1) == 1 and
            t.stride(0) >= t.shape[1] and
            (not aligned or (t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0))):
        return t
    return _dev(t, torch.float32)


i64 = ctypes.c_int64


def point_keys(frame, points, radii, radius_scale=1.0, max_depth=21):
    points = _dev(points, torch.float32)
    radii = _dev(radii, torch.float32)
    n = points.shape[0]
    keys = torch.empty(n, dtype=torch.int64, device=points.device)
    context(_same_device(points, radii)).call("asr_hip_point_keys", ctypes.byref(frame), ptr(points), ptr(radii), i64(n),
                   ctypes.c_float(radius_scale), int(max_depth), ptr(keys))
    return keys  # uint64 bit pattern in an int64 tensor


def octree_build(frame, points, radii, radius_scale=1.0, max_depth=21, grow_steps=0):
    """-> (nodes, leaves) sorted uint64 keys (as int64 tensors)"""
    points = _dev(points, torch.float32)
    radii = _dev(radii, torch.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError("points must have shape [N,3]")
    if radii.ndim != 1 or radii.shape[0] != points.shape[0]:
        raise ValueError("radii must have shape [N]")
    nn, nl = i64(0), i64(0)
    ctx = context(_same_device(points, radii))
    ctx.call("asr_hip_octree_build_grow", ctypes.byref(frame), ptr(points), ptr(radii),
             i64(points.shape[0]), ctypes.c_float(radius_scale), int(grow_steps), int(max_depth), ctypes.byref(nn),
             ctypes.byref(nl))
    nodes = torch.empty(nn.value, dtype=torch.int64, device=points.device)
    leaves = torch.empty(nl.value, dtype=torch.int64, device=points.device)
    ctx.call("asr_hip_octree_get", ptr(nodes), ptr(leaves))
    return nodes, leaves


def octree_build_parts(frame, points, radii, radius_scale=1.0, max_depth=21, extra_keys=None, balance=True):
    """asr_hip_octree_build_parts: closure of the keys of `points` (may be empty) and of `extra_keys` (int64 tensor of
    node keys), balanced unless balance is False -> (nodes, leaves)"""
    points = _dev(points, torch.float32).reshape(-1, 3)
    radii = _dev(radii, torch.float32).reshape(-1)
    ek = _dev(extra_keys, torch.int64) if extra_keys is not None and extra_keys.numel() else None
    nn, nl = i64(0), i64(0)
    ctx = context(_same_device(points, radii, ek))
    ctx.call("asr_hip_octree_build_parts", ctypes.byref(frame), ptr(points) if points.shape[0] else ctypes.c_void_p(0),
             ptr(radii) if points.shape[0] else ctypes.c_void_p(0), i64(points.shape[0]), ctypes.c_float(radius_scale),
             int(max_depth), ptr(ek), i64(ek.shape[0] if ek is not None else 0), int(bool(balance)), ctypes.byref(nn),
             ctypes.byref(nl))
    nodes = torch.empty(nn.value, dtype=torch.int64, device=points.device)
    leaves = torch.empty(nl.value, dtype=torch.int64, device=points.device)
    ctx.call("asr_hip_octree_get", ptr(nodes), ptr(leaves))
    return nodes, leaves


def dual_cells(device, ctx=None, nodes=None, leaves=None):
    """dual_vertex_indices [D,8] (int64): of the octree built last on this context, or of the octree given by
    its sorted node / leaf key tensors (any tree that is still alive)"""
    ctx = ctx or context(device)
    d = i64(0)
    if nodes is not None:
        nodes, leaves = _dev(nodes, torch.int64), _dev(leaves, torch.int64)
        ctx.call("asr_hip_dual_cells_count_for", ptr(nodes), i64(nodes.shape[0]), ptr(leaves), i64(leaves.shape[0]),
                 ctypes.byref(d))
    else:
        ctx.call("asr_hip_dual_cells_count", ctypes.byref(d))
    out = torch.empty((d.value, 8), dtype=torch.int64, device=device)
    if d.value:
        ctx.call("asr_hip_dual_cells_fill", ptr(out))
    return out


def contour(values, dual_vertex_indices, node_positions, threshold=1.0, ctx=None):
    """asr::CreateTriangleMesh (cpp/lib/contouring.cpp:29-460) -> (vertices f32[M,3], triangles i32[T,3])"""
    values = _dev(values, torch.float32)
    duals = _dev(dual_vertex_indices, torch.int64)
    pos = _dev(node_positions, torch.float32)
    if values.dim() != 2 or values.shape[1] != 2:
        raise ValueError("values must have shape [V,2]")
    if duals.dim() != 2 or duals.shape[1] != 8:
        raise ValueError("dual_vertex_indices must have shape [D,8]")
    if pos.dim() != 2 or pos.shape[1] != 3 or pos.shape[0] != values.shape[0]:
        raise ValueError("node_positions must have shape [V,3]")
    ctx = ctx or context(_same_device(values, duals, pos))
    nv, nt = i64(0), i64(0)
    ctx.call("asr_hip_contour_count", ptr(values), i64(values.shape[0]), ptr(duals), i64(duals.shape[0]),
             ptr(pos), ctypes.c_float(threshold), ctypes.byref(nv), ctypes.byref(nt))
    vertices = torch.empty((nv.value, 3), dtype=torch.float32, device=values.device)
    triangles = torch.empty((nt.value, 3), dtype=torch.int32, device=values.device)
    ctx.call("asr_hip_contour_fill", ptr(vertices), ptr(triangles))
    return vertices, triangles


def remove_components(vertices, triangles, keep_n, min_size=3, ctx=None):
    """asr::RemoveConnectedComponents (cpp/lib/postprocess.cpp:141-176)"""
    vertices = _dev(vertices, torch.float32)
    triangles = _dev(triangles, torch.int32)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must have shape [N,3]")
    if triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [M,3]")
    ctx = ctx or context(_same_device(vertices, triangles))
    nv, nt = i64(0), i64(0)
    ctx.call("asr_hip_components_count", ptr(vertices), i64(vertices.shape[0]), ptr(triangles),
             i64(triangles.shape[0]), i64(min(int(keep_n), 2**62)), i64(int(min_size)), ctypes.byref(nv),
             ctypes.byref(nt))
    v2 = torch.empty((nv.value, 3), dtype=torch.float32, device=vertices.device)
    t2 = torch.empty((nt.value, 3), dtype=torch.int32, device=vertices.device)
    ctx.call("asr_hip_components_fill", ptr(v2), ptr(t2))
    return v2, t2


def grid_neighbors(keys):
    keys = _dev(keys, torch.int64)
    v = keys.shape[0]
    rs = torch.empty(v + 1, dtype=torch.int64, device=keys.device)
    p = i64(0)
    ctx = context(_same_device(keys))
    ctx.call("asr_hip_grid_neighbors_count", ptr(keys), i64(v), ptr(rs), ctypes.byref(p))
    idx = torch.empty(p.value, dtype=torch.int32, device=keys.device)
    kidx = torch.empty(p.value, dtype=torch.uint8, device=keys.device)
    ctx.call("asr_hip_grid_neighbors_fill", ptr(keys), i64(v), ptr(rs), ptr(idx), ptr(kidx))
    return idx, kidx, rs


def grid_neighbors_rows(keys, rows):
    """55-slot lists of the voxels `rows` (ascending int32 indices) only: -> (index, kernel_index, row_splits [V + 1]);
    the rows that are not listed are empty, the entries of the listed ones compact and in row order"""
    keys = _dev(keys, torch.int64)
    rows = _dev(rows, torch.int32)
    v = keys.shape[0]
    rs = torch.empty(v + 1, dtype=torch.int64, device=keys.device)
    p = i64(0)
    ctx = context(_same_device(keys, rows))
    ctx.call("asr_hip_grid_neighbors_rows_count", ptr(keys), i64(v), ptr(rows), i64(rows.shape[0]), ptr(rs), ctypes.byref(p))
    idx = torch.empty(p.value, dtype=torch.int32, device=keys.device)
    kidx = torch.empty(p.value, dtype=torch.uint8, device=keys.device)
    ctx.call("asr_hip_grid_neighbors_rows_fill", ptr(keys), i64(v), ptr(rows), i64(rows.shape[0]), ptr(rs), ptr(idx),
             ptr(kidx))
    return idx, kidx, rs


def grid_coarsen(keys):
    keys = _dev(keys, torch.int64)
    v = keys.shape[0]
    vo = i64(0)
    ctx = context(_same_device(keys))
    ctx.call("asr_hip_grid_coarsen_count", ptr(keys), i64(v), ctypes.byref(vo))
    out_keys = torch.empty(vo.value, dtype=torch.int64, device=keys.device)
    up_idx = torch.empty(v, dtype=torch.int32, device=keys.device)
    up_kidx = torch.empty(v, dtype=torch.uint8, device=keys.device)
    up_rs = torch.empty(v + 1, dtype=torch.int64, device=keys.device)
    ctx.call("asr_hip_grid_coarsen_fill", ptr(keys), i64(v), ptr(out_keys), vo, ptr(up_idx),
             ptr(up_kidx), ptr(up_rs))
    return out_keys, up_idx, up_kidx, up_rs


def voxel_info(frame, keys):
    keys = _dev(keys, torch.int64)
    v = keys.shape[0]
    centers = torch.empty((v, 3), dtype=torch.float32, device=keys.device)
    sizes = torch.empty(v, dtype=torch.float32, device=keys.device)
    context(_same_device(keys)).call("asr_hip_voxel_info", ctypes.byref(frame), ptr(keys), i64(v), ptr(centers),
                   ptr(sizes))
    return centers, sizes


def multi_radius_search(frame, points, radii, centers, sizes):
    """-> (index int32, squared dist f32, row_splits int64, scale_compat f32)"""
    points = _dev(points, torch.float32)
    radii = _dev(radii, torch.float32)
    centers = _dev(centers, torch.float32)
    sizes = _dev(sizes, torch.float32)
    n, v = points.shape[0], sizes.shape[0]
    rs = torch.empty(v + 1, dtype=torch.int64, device=points.device)
    p = i64(0)
    ctx = context(_same_device(points, radii, centers, sizes))
    ctx.call("asr_hip_multi_radius_search_count", ctypes.byref(frame), ptr(points), i64(n),
             ptr(centers), ptr(sizes), i64(v), ptr(rs), ctypes.byref(p))
    idx = torch.empty(p.value, dtype=torch.int32, device=points.device)
    dist = torch.empty(p.value, dtype=torch.float32, device=points.device)
    compat = torch.empty(p.value, dtype=torch.float32, device=points.device)
    ctx.call("asr_hip_multi_radius_search_fill", ptr(points), ptr(radii), i64(n), ptr(centers),
             ptr(sizes), i64(v), ptr(rs), ptr(idx), ptr(dist), ptr(compat))
    return idx, dist, rs, compat


def knn_radius(frame, points, k, radii=None, radius_fraction=0.5, outlier_threshold=1,
               want_inlier=False):
    """KDTree.compute_k_radius / compute_inlier (cpp/lib/nsearch.cpp:30-86) -> radii[, inlier]"""
    points = _dev(points, torch.float32)
    n = points.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=points.device)
    rin = _dev(radii, torch.float32) if radii is not None else None
    inl = torch.empty(n, dtype=torch.uint8, device=points.device) if want_inlier else None
    context(_same_device(points, rin)).call("asr_hip_knn_radius", ctypes.byref(frame), ptr(points), i64(n), int(k), ptr(rin),
                   ctypes.c_float(radius_fraction), int(outlier_threshold), ptr(out), ptr(inl))
    return (out, inl.bool()) if want_inlier else out


def radius_neighbor_count(frame, points, radii):
    """KDTree.compute_radius_neighbors (cpp/lib/nsearch.cpp:88-105)"""
    points = _dev(points, torch.float32)
    radii = _dev(radii, torch.float32)
    out = torch.empty(points.shape[0], dtype=torch.int64, device=points.device)
    context(_same_device(points, radii)).call("asr_hip_radius_neighbor_count", ctypes.byref(frame), ptr(points), ptr(radii),
                   i64(points.shape[0]), ptr(out))
    return out


def aggregation_importance(compat, dist):
    compat = _dev(compat, torch.float32)
    dist = _dev(dist, torch.float32)
    out = torch.empty_like(compat)
    context(_same_device(compat, dist)).call("asr_hip_aggregation_importance", ptr(compat), ptr(dist), i64(compat.shape[0]),
                   ptr(out))
    return out


def continuous_conv(filters, out_positions, extents, inp_positions, inp_features, neighbors_index,
                    neighbors_importance, neighbors_row_splits, normalize=True, bias=None,
                    relu=False):
    filters = _dev(filters, torch.float32)
    if filters.ndim != 5 or tuple(filters.shape[:3]) != (4, 4, 4):
        raise RuntimeError("continuous_conv: only kernel_size [4,4,4] is implemented")
    cin, cout = filters.shape[3], filters.shape[4]
    out_positions = _dev(out_positions, torch.float32)
    v = out_positions.shape[0]
    extents = _dev(extents, torch.float32).reshape(-1)
    if extents.shape[0] == 1 and v != 1:
        extents = extents.expand(v).contiguous()
    if extents.shape[0] != v:
        raise RuntimeError("continuous_conv: extents must be a scalar or have one entry per output")
    inp_positions = _dev(inp_positions, torch.float32)
    inp_features = _dev(inp_features, torch.float32)
    if inp_features.shape[1] != cin:
        raise RuntimeError("continuous_conv: feature width does not match the filter")
    nidx = _dev(neighbors_index, torch.int32)
    rs = _dev(neighbors_row_splits, torch.int64)
    nimp = None
    if neighbors_importance is not None and neighbors_importance.numel():
        nimp = _dev(neighbors_importance, torch.float32)
    b = _dev(bias, torch.float32) if bias is not None else None
    out = torch.empty((v, cout), dtype=torch.float32, device=filters.device)
    dev = _same_device(filters, out_positions, extents, inp_positions, inp_features, nidx, rs, nimp, b)
    context(dev).call("asr_hip_continuous_conv_f32", ptr(filters), ptr(out_positions), ptr(extents),
                   ptr(inp_positions), ptr(inp_features), ptr(nidx), ptr(nimp), ptr(rs), i64(v),
                   int(cin), int(cout), int(bool(normalize)), ptr(b), int(bool(relu)), ptr(out))
    return out


def continuous_conv_basis(out_positions, extents, inp_positions, inp_features, neighbors_index,
                          neighbors_importance, neighbors_row_splits):
    """per-output interpolation matrices [V, 64*cin] and importance sums [V] of the continuous conv (cin = 4):
    the filter gradient is basis^T (grad / norm) (asr_hip_continuous_conv_basis_f32)"""
    out_positions = _dev(out_positions, torch.float32)
    v = out_positions.shape[0]
    extents = _dev(extents, torch.float32).reshape(-1)
    if extents.shape[0] == 1 and v != 1:
        extents = extents.expand(v).contiguous()
    inp_positions = _dev(inp_positions, torch.float32)
    inp_features = _dev(inp_features, torch.float32)
    cin = inp_features.shape[1]
    nidx = _dev(neighbors_index, torch.int32)
    rs = _dev(neighbors_row_splits, torch.int64)
    nimp = None
    if neighbors_importance is not None and neighbors_importance.numel():
        nimp = _dev(neighbors_importance, torch.float32)
    basis = torch.empty((v, 64 * cin), dtype=torch.float32, device=out_positions.device)
    norm = torch.empty(v, dtype=torch.float32, device=out_positions.device)
    dev = _same_device(out_positions, extents, inp_positions, inp_features, nidx, rs, nimp)
    context(dev).call("asr_hip_continuous_conv_basis_f32", ptr(out_positions), ptr(extents), ptr(inp_positions),
                      ptr(inp_features), ptr(nidx), ptr(nimp), ptr(rs), i64(v), int(cin), ptr(basis), ptr(norm))
    return basis, norm


def sparse_conv(filters, inp_features, neighbors_index, neighbors_kernel_index,
                neighbors_row_splits, inp_importance=None, normalize=False, bias=None, relu=False,
                residual=None, out=None, return_importance=False, algo=0,
                neighbors_importance=None, row_perm=None, filters_b=None, bias_b=None, force_nt=0,
                force_waves=0, num_rows=None, out_importance=None):
    """SpecialSparseConv.forward (models/common_torch.py:95-148) in one launch.  filters_b / bias_b:
    optional second filter bank (conv1a + conv1b of a SparseConvBlock in one pass): output columns
    [cout, cout + cout_b); importance, normalize and the returned importance sum then belong to bank b.
    num_rows (with row_perm): compute only the rows row_perm[:num_rows] -- a rank of a sharded run computes the
    rows it owns and leaves the other rows of `out` untouched.
    out_importance: a float32 [num_out] tensor that receives the importance sums (implies return_importance).
    inp_features and residual may be column slices of wider buffers: such a view is read in place, not copied (see
    _rows); `out` is always written in place.  With algo 0 or 2 no row of the list may name a slot twice
    (slots_unique_per_row); algo = 1 takes any list."""
    filters = _dev(filters, torch.float32)
    K, cin, cout = filters.shape
    inp_features = _rows(inp_features)
    nidx = _dev(neighbors_index, torch.int32)
    nk = _dev(neighbors_kernel_index, torch.uint8)
    rs = _dev(neighbors_row_splits, torch.int64)
    v = rs.shape[0] - 1
    if inp_features.shape[1] != cin:
        raise RuntimeError("sparse_conv: feature width does not match the filter")
    if nidx.numel() == 0:
        # a list without pairs: an empty tensor has no address and the entry point refuses a null list, although no
        # kernel would read one -- hand it one-element placeholders
        nidx = torch.zeros(1, dtype=torch.int32, device=filters.device)
        nk = torch.zeros(1, dtype=torch.uint8, device=filters.device)
    imp = _dev(inp_importance, torch.float32) if inp_importance is not None else None
    nimp = _dev(neighbors_importance, torch.float32) if neighbors_importance is not None else None
    b = _dev(bias, torch.float32) if bias is not None else None
    res = _rows(residual, aligned=False) if residual is not None else None  # read element by element
    fb = _dev(filters_b, torch.float32) if filters_b is not None else None
    bb = _dev(bias_b, torch.float32) if bias_b is not None else None
    if fb is not None and (fb.dim() != 3 or fb.shape[0] != K or fb.shape[1] != cin):
        raise RuntimeError("sparse_conv: second filter bank does not match the first")
    if out is None:
        out = torch.empty((v, cout + (fb.shape[2] if fb is not None else 0)), dtype=torch.float32,
                          device=filters.device)
    oimp = torch.empty(v, dtype=torch.float32, device=filters.device) if return_importance else None
    if out_importance is not None:
        if (out_importance.dtype != torch.float32 or out_importance.shape != (v,) or not out_importance.is_cuda or
                not out_importance.is_contiguous()):
            raise RuntimeError("sparse_conv: out_importance must be a contiguous float32 GPU tensor with one element per row")
        oimp, return_importance = out_importance, True
    a = _lib.SparseConvArgs()
    a.filters = filters.data_ptr()
    a.inp_features = inp_features.data_ptr()
    a.inp_ld = inp_features.stride(0)
    a.inp_importance = imp.data_ptr() if imp is not None else None
    a.neighbors_importance = nimp.data_ptr() if nimp is not None else None
    a.neighbors_index = nidx.data_ptr()
    a.neighbors_kernel_index = nk.data_ptr()
    a.neighbors_row_splits = rs.data_ptr()
    if num_rows is not None:
        if row_perm is None or not 0 <= int(num_rows) <= row_perm.shape[0]:
            raise RuntimeError("sparse_conv: num_rows needs a row_perm with at least that many rows")
        a.num_out = int(num_rows)
    else:
        a.num_out = v
    a.num_inp = inp_features.shape[0]
    a.kernel_size = K
    a.cin = cin
    a.cout = cout
    a.normalize = int(bool(normalize))
    a.bias = b.data_ptr() if b is not None else None
    a.relu = int(bool(relu))
    a.residual = res.data_ptr() if res is not None else None
    a.residual_ld = res.stride(0) if res is not None else 0
    a.out = out.data_ptr()
    a.out_ld = out.stride(0)
    a.out_importance = oimp.data_ptr() if oimp is not None else None
    a.algo = int(algo)
    perm = _dev(row_perm, torch.int32) if row_perm is not None else None
    a.row_perm = perm.data_ptr() if perm is not None else None
    a.filters_b = fb.data_ptr() if fb is not None else None
    a.bias_b = bb.data_ptr() if bb is not None else None
    a.cout_b = fb.shape[2] if fb is not None else 0
    a.force_nt = int(force_nt)
    a.force_waves = int(force_waves)
    dev = _same_device(filters, inp_features, nidx, nk, rs, imp, nimp, b, res, fb, bb, out, perm, oimp)
    context(dev).call("asr_hip_sparse_conv_f32", ctypes.byref(a))
    if return_importance:
        return out, oimp
    return out


def slots_unique_per_row(kernel_index, row_splits):
    """True when no row of the list names a kernel slot twice: the precondition of sparse_conv with algo 0 or 2 and of
    the 16-bit kernels.  One sort over the pairs on the tensors' device and one read-back; the tensors of a list may
    change between calls, so the verdict belongs to this call only (nothing is cached).  Slots are compared as the
    uint8 values the kernels read."""
    k = kernel_index.reshape(-1).to(torch.uint8)
    pairs = k.shape[0]
    if pairs < 2:
        return True
    rs = row_splits.reshape(-1).to(torch.int64)
    rows = torch.arange(rs.shape[0] - 1, dtype=torch.int64, device=rs.device)
    row = torch.repeat_interleave(rows, rs[1:] - rs[:-1], output_size=pairs).to(k.device)
    key = torch.sort(row * 256 + k.to(torch.int64)).values
    return not bool((key[1:] == key[:-1]).any())


def pack_filters(filters, mode, filters_b=None):
    """re-packed 16-bit copy of a filter tensor [K, cin, cout] (+ second bank [K, cin, cout_b]) for
    sparse_conv16 (asr_hip_sparse_conv_pack); mode: "f16", "bf16x3", "bf16x3_2acc" or "f16x2" ("bf16x3_2acc" packs the
    same bytes as "bf16x3").  Pack once per weight tensor."""
    m = _lib.PRECISIONS[mode]
    filters = _dev(filters, torch.float32)
    fb = _dev(filters_b, torch.float32) if filters_b is not None else None
    K, cin, cout = filters.shape
    cb = fb.shape[2] if fb is not None else 0
    nbytes = _lib.load().asr_hip_sparse_conv_packed_bytes(m, int(K), int(cin), int(cout), int(cb))
    if nbytes == 0:
        raise RuntimeError("pack_filters: bad shape / mode")
    out = torch.empty(nbytes, dtype=torch.uint8, device=filters.device)
    context(_same_device(filters, fb)).call("asr_hip_sparse_conv_pack", m, ptr(filters), ptr(fb), int(K), int(cin),
                                            int(cout), int(cb), ptr(out))
    return out


class ConvPlan:
    """Row-group plan of one neighbour list (asr_hip_sparse_conv_plan_create): build once, pass as plan= to every
    sparse_conv16 over the same (neighbour arrays, row_perm, num_rows).  Keeps the arrays it was built from alive."""

    def __init__(self, kernel_size, neighbors_index, neighbors_kernel_index, neighbors_row_splits, row_perm=None,
                 num_rows=None):
        self.nidx = _dev(neighbors_index, torch.int32)
        self.nk = _dev(neighbors_kernel_index, torch.uint8)
        self.rs = _dev(neighbors_row_splits, torch.int64)
        self.perm = _dev(row_perm, torch.int32) if row_perm is not None else None
        self.num_rows = self.rs.shape[0] - 1 if num_rows is None else int(num_rows)
        self.kernel_size = int(kernel_size)
        self.ctx = context(_same_device(self.nidx, self.nk, self.rs, self.perm))
        h = ctypes.c_void_p(0)
        self.ctx.call("asr_hip_sparse_conv_plan_create", ptr(self.nidx), ptr(self.nk), ptr(self.rs),
                      ptr(self.perm) if self.perm is not None else ctypes.c_void_p(0), i64(self.num_rows),
                      ctypes.c_int(self.kernel_size), ctypes.byref(h))
        self.handle = h

    def nbytes(self):
        f = self.ctx.lib.asr_hip_sparse_conv_plan_bytes
        f.restype = ctypes.c_size_t
        return int(f(self.handle))

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                self.ctx.lib.asr_hip_sparse_conv_plan_destroy(h)
            except Exception:
                pass


def sparse_conv16(mode, packed, kernel_size, cin, cout, inp_features, neighbors_index, neighbors_kernel_index,
                  neighbors_row_splits, inp_importance=None, normalize=False, bias=None, relu=False, residual=None,
                  out=None, out_dtype=None, return_importance=False, neighbors_importance=None, row_perm=None,
                  num_rows=None, cout_b=0, bias_b=None, force_nt=0, force_waves=0, plan=None, inp_absmax=None,
                  out_absmax=None):
    """SpecialSparseConv.forward on the 16-bit matrix cores (asr_hip_sparse_conv_f16 / _bf16x3 / _bf16x3_2acc / _f16x2).
    mode "f16": inp_features / residual are float16 tensors, out is float16 (default) or float32;
    mode "bf16x3" / "bf16x3_2acc" / "f16x2": float32 in and out, fp32-class result.  packed: pack_filters(filters, mode[, filters_b]).
    plan: ConvPlan of this list (one is built for the call otherwise).
    inp_absmax / out_absmax: int32 device scalars with the f32 bits of the largest |element| of the input (f16x2; None:
    computed by one pass) and the running maximum of what is written to out (new_absmax(); the caller zeroes it)."""
    m = _lib.PRECISIONS[mode]
    act = torch.float16 if mode == "f16" else torch.float32
    inp_features = _dev(inp_features, act)
    nidx = _dev(neighbors_index, torch.int32)
    nk = _dev(neighbors_kernel_index, torch.uint8)
    rs = _dev(neighbors_row_splits, torch.int64)
    v = rs.shape[0] - 1
    if inp_features.shape[1] != cin:
        raise RuntimeError("sparse_conv16: feature width does not match the filter")
    imp = _dev(inp_importance, torch.float32) if inp_importance is not None else None
    nimp = _dev(neighbors_importance, torch.float32) if neighbors_importance is not None else None
    b = _dev(bias, torch.float32) if bias is not None else None
    bb = _dev(bias_b, torch.float32) if bias_b is not None else None
    res = _dev(residual, act) if residual is not None else None
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else act
    if out_dtype not in (torch.float32, act):
        raise RuntimeError("sparse_conv16: out must be float32 or the activation type")
    if out is None:
        out = torch.empty((v, cout + cout_b), dtype=out_dtype, device=inp_features.device)
    oimp = torch.empty(v, dtype=torch.float32, device=inp_features.device) if return_importance else None
    perm = _dev(row_perm, torch.int32) if row_perm is not None else None
    a = _lib.SparseConvArgs()
    a.inp_features = inp_features.data_ptr()
    a.inp_ld = inp_features.stride(0)
    a.inp_importance = imp.data_ptr() if imp is not None else None
    a.neighbors_importance = nimp.data_ptr() if nimp is not None else None
    a.neighbors_index = nidx.data_ptr()
    a.neighbors_kernel_index = nk.data_ptr()
    a.neighbors_row_splits = rs.data_ptr()
    a.num_out = v if num_rows is None else int(num_rows)
    a.num_inp = inp_features.shape[0]
    a.kernel_size, a.cin, a.cout, a.cout_b = int(kernel_size), int(cin), int(cout), int(cout_b)
    a.normalize = int(bool(normalize))
    a.bias = b.data_ptr() if b is not None else None
    a.bias_b = bb.data_ptr() if bb is not None else None
    a.relu = int(bool(relu))
    a.residual = res.data_ptr() if res is not None else None
    a.residual_ld = res.stride(0) if res is not None else 0
    a.out = out.data_ptr()
    a.out_ld = out.stride(0)
    a.out_importance = oimp.data_ptr() if oimp is not None else None
    a.row_perm = perm.data_ptr() if perm is not None else None
    a.force_nt, a.force_waves = int(force_nt), int(force_waves)
    if plan is not None:
        if plan.rs.data_ptr() != rs.data_ptr() or plan.nidx.data_ptr() != nidx.data_ptr() or \
                (plan.perm.data_ptr() if plan.perm is not None else None) != (perm.data_ptr() if perm is not None else None):
            raise RuntimeError("sparse_conv16: the plan belongs to other neighbour arrays")
        a.plan = plan.handle
    a.inp_absmax = inp_absmax.data_ptr() if inp_absmax is not None else None
    a.out_absmax = out_absmax.data_ptr() if out_absmax is not None else None
    ctx = context(_same_device(packed, inp_features, nidx, nk, rs, imp, nimp, b, bb, res, out, perm))
    if mode == "f16":
        ctx.call("asr_hip_sparse_conv_f16", ctypes.byref(a), ptr(packed), int(out.dtype == torch.float16))
    elif mode == "f16x2":
        ctx.call("asr_hip_sparse_conv_f16x2", ctypes.byref(a), ptr(packed))
    elif mode == "bf16x3_2acc":
        ctx.call("asr_hip_sparse_conv_bf16x3_2acc", ctypes.byref(a), ptr(packed))
    else:
        ctx.call("asr_hip_sparse_conv_bf16x3", ctypes.byref(a), ptr(packed))
    return (out, oimp) if return_importance else out


def absmax(x, out=None):
    """f32 bits of the largest |element| of a float32 matrix as an int32 device scalar (asr_hip_absmax_f32): the
    inp_absmax of sparse_conv16 in mode "f16x2" """
    x = _dev(x, torch.float32)
    if out is None:
        out = torch.zeros(1, dtype=torch.int32, device=x.device)
    context(x.device).call("asr_hip_absmax_f32", ptr(x), i64(x.shape[0]), ctypes.c_int(x.shape[1]), i64(x.stride(0)),
                           ptr(out))
    return out


def row_groups(neighbors_kernel_index, neighbors_row_splits, segment_rows=0):
    """MFMA tiling order of a CSR's rows (asr_hip_row_groups)"""
    nk = _dev(neighbors_kernel_index, torch.uint8)
    rs = _dev(neighbors_row_splits, torch.int64)
    v = rs.shape[0] - 1
    if nk.numel() == 0:  # a list without pairs: an empty tensor has no address (see sparse_conv); no kernel reads it
        nk = torch.zeros(1, dtype=torch.uint8, device=rs.device)
    perm = torch.empty(v, dtype=torch.int32, device=rs.device)
    context(_same_device(nk, rs)).call("asr_hip_row_groups", ptr(nk), ptr(rs), i64(v), i64(segment_rows), ptr(perm))
    return perm


def _pair_rows(rs, pairs):
    """the row of every pair of a list with row splits rs (int64 [pairs])"""
    rows = torch.arange(rs.shape[0] - 1, dtype=torch.int64, device=rs.device)
    return torch.repeat_interleave(rows, rs[1:] - rs[:-1], output_size=pairs)


def invert_neighbors_list(num_points, inp_neighbors_index, inp_neighbors_row_splits,
                          inp_neighbors_attributes=None):
    """open3d::invert_neighbors_list -> (index int32, row_splits int64 [num_points + 1], attributes).  The attributes
    come back in their own dtype, bit for bit: uint8 (the kernel indices of the model) travel through the kernel, every
    other type is permuted with the same stable order by input (one device-side sort); nothing is ever cast."""
    idx = _dev(inp_neighbors_index, torch.int32)
    rs = _dev(inp_neighbors_row_splits, torch.int64)
    attr = carried = None
    if inp_neighbors_attributes is not None and inp_neighbors_attributes.numel():
        a = inp_neighbors_attributes
        if not a.is_cuda:
            raise AsrHipError("expected a GPU tensor: the HIP path has no CPU fallback")
        if a.shape[0] != idx.shape[0]:
            raise AsrHipError("invert_neighbors_list: one attribute per pair expected")
        if a.dtype == torch.uint8 and a.dim() == 1:
            attr = a.contiguous()
        else:
            carried = a
    p = idx.shape[0]
    out_idx = torch.empty(p, dtype=torch.int32, device=idx.device)
    out_rs = torch.empty(num_points + 1, dtype=torch.int64, device=idx.device)
    out_attr = torch.empty(p if attr is not None else 0, dtype=torch.uint8, device=idx.device)
    context(_same_device(idx, rs, attr, carried)).call("asr_hip_invert_neighbors_list", i64(num_points), ptr(idx), ptr(rs),
                   i64(rs.shape[0] - 1), ptr(attr), ptr(out_idx), ptr(out_rs),
                   ptr(out_attr) if attr is not None else ctypes.c_void_p(0))
    if carried is not None:
        out_attr = carried.index_select(0, torch.argsort(idx.long(), stable=True))
    return out_idx, out_rs, out_attr


_REDUCE_EXACT_TYPES = (torch.float64, torch.int32, torch.int64)


def reduce_subarrays_sum(values, row_splits, gather_index=None):
    """open3d::reduce_subarrays_sum (of values[gather_index] when given) in the dtype of `values`: float32 through the
    kernel (sequential f32 sum per row); float64, int32 and int64 are summed in their own type on the device
    (index_add_); every other dtype is refused."""
    if not isinstance(values, torch.Tensor):
        values = torch.as_tensor(values)
    rs = _dev(row_splits, torch.int64)
    g = _dev(gather_index, torch.int32) if gather_index is not None else None
    rows = rs.shape[0] - 1
    if values.dtype in _REDUCE_EXACT_TYPES:
        if not values.is_cuda:
            raise AsrHipError("expected a GPU tensor: the HIP path has no CPU fallback")
        _same_device(values, rs, g)
        x = values.reshape(-1) if g is None else values.reshape(-1).index_select(0, g.long())
        out = torch.zeros(rows, dtype=values.dtype, device=values.device)
        return out.index_add_(0, _pair_rows(rs, x.shape[0]), x) if x.shape[0] else out
    if values.dtype != torch.float32:
        raise AsrHipError("reduce_subarrays_sum: values must be float32, float64, int32 or int64, not %s" % values.dtype)
    values = _dev(values, torch.float32)
    if values.numel() == 0:
        return torch.zeros(rows, dtype=torch.float32, device=rs.device)  # no value at all: every row is empty
    out = torch.empty(rows, dtype=torch.float32, device=values.device)
    context(_same_device(values, rs, g)).call("asr_hip_reduce_subarrays_sum", ptr(values), ptr(g), ptr(rs),
                   i64(rows), ptr(out))
    return out


def decode_mlp(code, w1, b1, w2, b2, w3, voxel_sizes=None):
    code = _dev(code, torch.float32)
    w1, b1, w2, b2, w3 = (_dev(t, torch.float32) for t in (w1, b1, w2, b2, w3))
    sizes = _dev(voxel_sizes, torch.float32) if voxel_sizes is not None else None
    v, c = code.shape
    out = torch.empty((v, 2), dtype=torch.float32, device=code.device)
    dev = _same_device(code, w1, b1, w2, b2, w3, sizes)
    context(dev).call("asr_hip_decode_mlp", ptr(code), i64(v), int(c), ptr(w1), ptr(b1),
                   int(w1.shape[0]), ptr(w2), ptr(b2), int(w2.shape[0]), ptr(w3), ptr(sizes),
                   ptr(out))
    return out


def leaf_locate(frame, leaf_keys, positions):
    """row of the leaf of `leaf_keys` (sorted ascending, tiling the root cube of `frame`) that contains each position,
    -1 outside the cube or for non-finite positions (asr_hip_leaf_locate) -> int32 [M]"""
    leaf_keys = _dev(leaf_keys, torch.int64)  # uint64 bit patterns
    positions = _dev(positions, torch.float32)
    if positions.ndim != 2 or positions.shape[1] != 3:
        raise ValueError("positions must have shape [M,3]")
    rows = torch.empty(positions.shape[0], dtype=torch.int32, device=positions.device)
    context(_same_device(leaf_keys, positions)).call("asr_hip_leaf_locate", ctypes.byref(frame), ptr(leaf_keys),
                                                     i64(leaf_keys.numel()), ptr(positions), i64(positions.shape[0]),
                                                     ptr(rows))
    return rows


def point_attributes_at(frame, points, radii, attributes, positions, sizes, max_widen=3, min_weight=1e-2, fill=0.0,
                        return_info=False):
    """Per-point attributes [N,C] (or [N]: one channel) blended at positions [M,3] with the aggregation's own weight
    (asr_hip_point_attributes_at): for k = 0..max_widen and R = sizes[j] * 2**k, the points with squared distance
    < R*R weigh (min(R, 2r)/max(R, 2r))**2 * clamp((1 - d/R**2)**3, 0, 1); row j is their weighted mean for the first
    k whose weight sum reaches min_weight.  Rows without such a k, positions outside the frame's cube or non-finite,
    and sizes that are not finite and > 0 get `fill`.  -> f32 [M,C]; return_info=True adds (weight f32 [M], the chosen
    weight sum or 0, and widen int8 [M], the chosen k or -1)."""
    points = _dev(points, torch.float32)
    radii = _dev(radii, torch.float32)
    attributes = _dev(attributes, torch.float32)
    positions = _dev(positions, torch.float32)
    sizes = _dev(sizes, torch.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError("points must have shape [N,3]")
    n = points.shape[0]
    if attributes.ndim == 1:
        attributes = attributes[:, None].contiguous()
    if tuple(radii.shape) != (n,):
        raise ValueError("radii must have shape [N]")
    if attributes.ndim != 2 or attributes.shape[0] != n:
        raise ValueError("attributes must have shape [N] or [N,C]")
    if positions.ndim != 2 or positions.shape[1] != 3:
        raise ValueError("positions must have shape [M,3]")
    m, c = positions.shape[0], attributes.shape[1]
    if tuple(sizes.shape) != (m,):
        raise ValueError("sizes must have shape [M]")
    out = torch.empty((m, c), dtype=torch.float32, device=points.device)
    weight = torch.empty(m, dtype=torch.float32, device=points.device) if return_info else None
    widen = torch.empty(m, dtype=torch.int8, device=points.device) if return_info else None
    context(_same_device(points, radii, attributes, positions, sizes)).call(
        "asr_hip_point_attributes_at", ctypes.byref(frame), ptr(points), ptr(radii), i64(n), ptr(attributes), int(c),
        ptr(positions), ptr(sizes), i64(m), int(max_widen), ctypes.c_float(min_weight), ctypes.c_float(fill), ptr(out),
        ptr(weight), ptr(widen))
    return (out, weight, widen) if return_info else out


def nearest_point(frame, points, queries):
    """For each query [M,3] the nearest of `points` [N,3], another set (asr_hip_nearest_point): exactly the result of a
    brute-force search with d2 = ((dx*dx + dy*dy) + dz*dz) in f32, ties to the smallest point index.  The frame only
    defines the acceleration grid: queries may lie anywhere.  A non-finite query gets index -1 and distance +inf.
    -> (index int32 [M], squared distance f32 [M])"""
    points = _dev(points, torch.float32)
    queries = _dev(queries, torch.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError("points must have shape [N,3]")
    if queries.ndim != 2 or queries.shape[1] != 3:
        raise ValueError("queries must have shape [M,3]")
    n, m = points.shape[0], queries.shape[0]
    index = torch.empty(m, dtype=torch.int32, device=points.device)
    sqdist = torch.empty(m, dtype=torch.float32, device=points.device)
    context(_same_device(points, queries)).call("asr_hip_nearest_point", ctypes.byref(frame), ptr(points), i64(n),
                                                ptr(queries), i64(m), ptr(index), ptr(sqdist))
    return index, sqdist


def mesh_sample(vertices, triangles, num_samples, seed=0, normals=False, return_triangle=False):
    """num_samples points on the triangle mesh (vertices f32 [V,3], triangles int32 [T,3]), area weighted, stratified and
    a pure function of the arguments (asr_hip_mesh_sample) -> points f32 [S,3]; normals=True adds the unit face normals
    f32 [S,3] (corner order), return_triangle=True the triangle of each sample, int32 [S] (in that order)."""
    vertices = _dev(vertices, torch.float32)
    triangles = _dev(triangles, torch.int32)
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must have shape [V,3]")
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [T,3]")
    s = int(num_samples)
    if s < 0:
        raise ValueError("num_samples must be >= 0")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must fit an unsigned 64-bit integer")
    dev = _same_device(vertices, triangles)
    points = torch.empty((s, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((s, 3), dtype=torch.float32, device=dev) if normals else None
    tri = torch.empty(s, dtype=torch.int32, device=dev) if return_triangle else None
    context(dev).call("asr_hip_mesh_sample", ptr(vertices), i64(vertices.shape[0]), ptr(triangles),
                      i64(triangles.shape[0]), i64(s), ctypes.c_uint64(seed), ptr(points), ptr(nrm), ptr(tri))
    out = (points,) + ((nrm,) if normals else ()) + ((tri,) if return_triangle else ())
    return out[0] if len(out) == 1 else out


def mesh_simplify(frame, vertices, triangles, level=None, levels=None, return_map=False, ctx=None):
    """Octree vertex clustering with quadric placement (asr_hip_mesh_simplify_count / _fill; the contract is in
    include/asr_hip.h): all vertices in one cell of `frame` at `level` (0..21, one for the whole mesh) or at `levels`
    (int8-convertible [V], one per vertex) become one vertex, placed on the planes of the triangles around it and kept
    inside the cell; triangles that collapse or repeat are dropped.  Exactly one of level and levels must be given.
    -> (vertices f32 [V',3], triangles int32 [T',3]); return_map=True adds vertex_map int32 [V], the output vertex of
    every input vertex or -1.  The result may have non-manifold edges; it is not filtered (remove_components)."""
    vertices = _dev(vertices, torch.float32)
    triangles = _dev(triangles, torch.int32)
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must have shape [V,3]")
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [T,3]")
    if (level is None) == (levels is None):
        raise ValueError("give exactly one of level and levels")
    nv = vertices.shape[0]
    if levels is not None:
        levels = _dev(levels, torch.int8)
        if tuple(levels.shape) != (nv,):
            raise ValueError("levels must have shape [V]")
    dev = _same_device(vertices, triangles, levels)
    ctx = ctx or context(dev)
    nvo, nto = i64(0), i64(0)
    ctx.call("asr_hip_mesh_simplify_count", ctypes.byref(frame), ptr(vertices), i64(nv), ptr(triangles),
             i64(triangles.shape[0]), ptr(levels), int(level) if levels is None else 0, ctypes.byref(nvo),
             ctypes.byref(nto))
    v2 = torch.empty((nvo.value, 3), dtype=torch.float32, device=dev)
    t2 = torch.empty((nto.value, 3), dtype=torch.int32, device=dev)
    vmap = torch.empty(nv, dtype=torch.int32, device=dev) if return_map else None
    ctx.call("asr_hip_mesh_simplify_fill", ptr(v2), ptr(t2), ptr(vmap))
    return (v2, t2, vmap) if return_map else (v2, t2)


def _triangles(triangles):
    triangles = _dev(triangles, torch.int32)
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [T,3]")
    return triangles


def _num_vertices(num_vertices):
    nv = int(num_vertices)
    if nv < 0:
        raise ValueError("num_vertices must be >= 0")
    return nv


def mesh_edges(triangles, num_vertices, ctx=None):
    """The edge table of a triangle list (asr_hip_mesh_edges_count / _fill; the contract is in include/asr_hip.h): the
    distinct undirected edges (lo, hi) of the triangles with three different corners, in ascending order
    -> (edges int32 [E,2], uses int32 [E], forward int32 [E]): how many triangle sides use each edge and how many of them
    run lo -> hi.  uses == 1: boundary, uses >= 3: non-manifold, uses == 2 with forward != 1: inconsistent orientation."""
    triangles = _triangles(triangles)
    nv = _num_vertices(num_vertices)
    dev = triangles.device
    ctx = ctx or context(dev)
    ne = i64(0)
    ctx.call("asr_hip_mesh_edges_count", ptr(triangles), i64(triangles.shape[0]), i64(nv), ctypes.byref(ne))
    edges = torch.empty((ne.value, 2), dtype=torch.int32, device=dev)
    uses = torch.empty(ne.value, dtype=torch.int32, device=dev)
    forward = torch.empty(ne.value, dtype=torch.int32, device=dev)
    ctx.call("asr_hip_mesh_edges_fill", ptr(edges), ptr(uses), ptr(forward))
    return edges, uses, forward


def topology_summary(counts):
    """the dict of mesh_topology from the counts of asr_mesh_topology (a dict of ints): adds edge_manifold, oriented,
    watertight and genus ((2 components - euler) // 2 when watertight, else None).  Host arithmetic only."""
    out = {k: int(v) for k, v in counts.items()}
    out["edge_manifold"] = out["nonmanifold_edges"] == 0
    out["oriented"] = out["inconsistent_edges"] == 0
    out["watertight"] = (out["boundary_edges"] == 0 and out["nonmanifold_edges"] == 0 and out["inconsistent_edges"] == 0
                         and out["triangles"] > 0)
    out["genus"] = (2 * out["components"] - out["euler"]) // 2 if out["watertight"] else None
    return out


def mesh_topology(triangles, num_vertices, ctx=None):
    """What kind of mesh is this (asr_hip_mesh_topology; definitions in include/asr_hip.h) -> dict of Python ints:
    num_vertices, used_vertices, triangles, degenerate_triangles, edges, boundary_edges, nonmanifold_edges,
    inconsistent_edges, components, boundary_loops, euler; and derived from them edge_manifold, oriented, watertight
    (bools) and genus (int, None unless watertight).  Non-manifold VERTICES are not detected."""
    triangles = _triangles(triangles)
    nv = _num_vertices(num_vertices)
    ctx = ctx or context(triangles.device)
    out = _lib.MeshTopology()
    ctx.call("asr_hip_mesh_topology", ptr(triangles), i64(triangles.shape[0]), i64(nv), ctypes.byref(out))
    return topology_summary({name: getattr(out, name) for name, _ in _lib.MeshTopology._fields_})


SMOOTH_BOUNDARY = {"free": 0, "pinned": 1, "along": 2}


def check_smooth_arguments(iterations, lam, mu, boundary):
    """-> (iterations, lam, mu, boundary mode number) or ValueError; no GPU involved"""
    if isinstance(iterations, bool) or int(iterations) != iterations or not 0 <= int(iterations) <= 1000:
        raise ValueError("iterations must be an integer in 0..1000")
    lam, mu = float(lam), float(mu)
    if not 0.0 < lam <= 1.0:
        raise ValueError("lam must be in (0, 1]")
    if not (mu <= 0.0 and mu > float("-inf")):
        raise ValueError("mu must be a finite number <= 0 (0: plain Laplacian smoothing)")
    if boundary not in SMOOTH_BOUNDARY:
        raise ValueError("boundary must be one of %s" % ", ".join(sorted(SMOOTH_BOUNDARY)))
    return int(iterations), lam, mu, SMOOTH_BOUNDARY[boundary]


def mesh_smooth(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, boundary="along", ctx=None, out=None):
    """Taubin smoothing of a triangle mesh (asr_hip_mesh_smooth; the contract is in include/asr_hip.h): `iterations` times
    a step p += lam (mean of the edge neighbours - p) followed by the same step with mu < -lam, which undoes the
    shrinking of the first; mu = 0 is plain Laplacian smoothing.  boundary: "free" (every vertex uses all neighbours),
    "pinned" (the ends of boundary and non-manifold edges stay where they are) or "along" (they move along their own
    rim or seam only).  f64 between the steps, one rounding to f32 at the end, the same bits on every run.
    -> vertices f32 [V,3] (`out`, when given: it may be `vertices` itself); the triangles do not change."""
    iterations, lam, mu, mode = check_smooth_arguments(iterations, lam, mu, boundary)
    vertices = _dev(vertices, torch.float32)
    triangles = _dev(triangles, torch.int32)
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must have shape [V,3]")
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [T,3]")
    dev = _same_device(vertices, triangles, out)
    if out is None:
        out = torch.empty_like(vertices)
    elif out.dtype != torch.float32 or out.shape != vertices.shape or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of the shape of vertices")
    ctx = ctx or context(dev)
    ctx.call("asr_hip_mesh_smooth", ptr(vertices), i64(vertices.shape[0]), ptr(triangles), i64(triangles.shape[0]),
             iterations, ctypes.c_double(lam), ctypes.c_double(mu), mode, ptr(out))
    return out


FILL_MAX_EDGES = 1 << 20


def check_fill_arguments(max_edges):
    """-> max_edges as an int or ValueError; no GPU involved"""
    if isinstance(max_edges, bool) or int(max_edges) != max_edges or not 3 <= int(max_edges) <= FILL_MAX_EDGES:
        raise ValueError("max_edges must be an integer in 3..%d" % FILL_MAX_EDGES)
    return int(max_edges)


def mesh_fill_holes(vertices, triangles, max_edges, return_report=False, ctx=None):
    """Closes the small holes of a triangle mesh (asr_hip_mesh_fill_holes_count / _fill; the contract is in
    include/asr_hip.h): every simple boundary rim of at most `max_edges` (3..2^20) edges gets a hub vertex at the mean of
    its vertices and one triangle per rim edge, oriented like the triangle on the edge's other side; a rim of three edges
    gets one triangle and no hub.  Rims that are longer (the outer border of an open scan), that touch another rim in a
    vertex or whose triangles disagree about the orientation stay open.
    -> (vertices f32 [V + hubs,3], triangles int32 [T + new,3]): the input arrays come first, unchanged.
    return_report=True adds a dict of ints: rims, filled, too_long, not_simple, new_vertices, new_triangles."""
    max_edges = check_fill_arguments(max_edges)
    vertices = _dev(vertices, torch.float32)
    triangles = _dev(triangles, torch.int32)
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must have shape [V,3]")
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError("triangles must have shape [T,3]")
    dev = _same_device(vertices, triangles)
    ctx = ctx or context(dev)
    nvo, nto, report = i64(0), i64(0), _lib.MeshFillReport()
    ctx.call("asr_hip_mesh_fill_holes_count", ptr(vertices), i64(vertices.shape[0]), ptr(triangles),
             i64(triangles.shape[0]), i64(max_edges), ctypes.byref(nvo), ctypes.byref(nto), ctypes.byref(report))
    v2 = torch.empty((nvo.value, 3), dtype=torch.float32, device=dev)
    t2 = torch.empty((nto.value, 3), dtype=torch.int32, device=dev)
    ctx.call("asr_hip_mesh_fill_holes_fill", ptr(v2), ptr(t2))
    if return_report:
        return v2, t2, {name: int(getattr(report, name)) for name, _ in _lib.MeshFillReport._fields_}
    return v2, t2


def _shape(t):
    return tuple(t.shape) if hasattr(t, "shape") else tuple(torch.as_tensor(t).shape)


def check_merge_arguments(points, normals, radii, attributes, level, levels, split_sides):
    """the shapes and options of points_merge, or ValueError; no GPU involved -> (n, c)"""
    shape = _shape(points)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("points must have shape [N,3]")
    n = shape[0]
    if n >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 points")
    if normals is not None and _shape(normals) != (n, 3):
        raise ValueError("normals must have shape [N,3]")
    if radii is not None and _shape(radii) != (n,):
        raise ValueError("radii must have shape [N]")
    c = 0
    if attributes is not None:
        shape = _shape(attributes)
        if len(shape) == 1:
            shape = shape + (1,)
        if len(shape) != 2 or shape[0] != n:
            raise ValueError("attributes must have shape [N] or [N,C]")
        c = shape[1]
        if not 1 <= c <= _lib.ASR_MAX_ATTRIBUTE_CHANNELS:
            raise ValueError("%d attribute channels, supported are 1 to %d" % (c, _lib.ASR_MAX_ATTRIBUTE_CHANNELS))
    if (level is None) == (levels is None):
        raise ValueError("give exactly one of level and levels")
    if level is not None and (isinstance(level, bool) or int(level) != level or not 0 <= int(level) <= _lib.ASR_MAX_LEVEL):
        raise ValueError("level must be an integer in 0..%d" % _lib.ASR_MAX_LEVEL)
    if levels is not None and _shape(levels) != (n,):
        raise ValueError("levels must have shape [N]")
    if split_sides and normals is None:
        raise ValueError("split_sides needs normals")
    return n, c


def points_merge(frame, points, normals=None, radii=None, attributes=None, level=None, levels=None, split_sides=False,
                 return_map=False, return_counts=False, return_report=False, ctx=None):
    """One point per occupied octree cell (asr_hip_points_merge_count / _fill; the contract is in include/asr_hip.h): all
    points in one cell of `frame` at `level` (0..21, one for the whole cloud) or at `levels` (int8-convertible [N], one per
    point) become one point -- position, radius and attributes [N] or [N,C] (C <= 16) are the f64 mean of the members,
    the normal their normalised sum.  split_sides=True (needs normals) keeps the members whose normal points against
    that of the cell's first member as a cluster of their own: the two faces of a thin wall stay apart.  Points that are
    not finite or lie outside the frame's root cube are dropped.  Clusters come in ascending key order, the same bits on
    every run.  Exactly one of level and levels must be given.
    -> (points f32 [M,3], normals f32 [M,3] or None, radii f32 [M] or None, attributes f32 [M,C] or None), followed by
    cluster int32 [N] (the output point of every input point, -1: dropped) with return_map, counts int32 [M] with
    return_counts and a dict of ints (clusters, dropped, largest_cluster, split_cells) with return_report."""
    n, c = check_merge_arguments(points, normals, radii, attributes, level, levels, split_sides)
    points = _dev(points, torch.float32)
    normals = _dev(normals, torch.float32) if normals is not None else None
    radii = _dev(radii, torch.float32) if radii is not None else None
    if attributes is not None:
        attributes = _dev(attributes, torch.float32).reshape(n, c)
    if levels is not None:
        levels = _dev(levels, torch.int8)
    dev = _same_device(points, normals, radii, attributes, levels)
    ctx = ctx or context(dev)
    m, report = i64(0), _lib.PointsMergeReport()
    ctx.call("asr_hip_points_merge_count", ctypes.byref(frame), ptr(points), i64(n), ptr(normals), ptr(radii),
             ptr(attributes), int(c), ptr(levels), int(level) if levels is None else 0, int(bool(split_sides)),
             ctypes.byref(m), ctypes.byref(report))
    m = m.value
    p2 = torch.empty((m, 3), dtype=torch.float32, device=dev)
    n2 = torch.empty((m, 3), dtype=torch.float32, device=dev) if normals is not None else None
    r2 = torch.empty(m, dtype=torch.float32, device=dev) if radii is not None else None
    a2 = torch.empty((m, c), dtype=torch.float32, device=dev) if attributes is not None else None
    counts = torch.empty(m, dtype=torch.int32, device=dev) if return_counts else None
    cluster = torch.empty(n, dtype=torch.int32, device=dev) if return_map else None
    ctx.call("asr_hip_points_merge_fill", ptr(p2), ptr(n2), ptr(r2), ptr(a2), ptr(counts), ptr(cluster))
    out = (p2, n2, r2, a2) + ((cluster,) if return_map else ()) + ((counts,) if return_counts else ())
    if return_report:
        out += ({name: int(getattr(report, name)) for name, _ in _lib.PointsMergeReport._fields_},)
    return out


KNN_INDEX_MAX_K = 64
ORIENT_REPORT = ("components", "flipped", "skipped", "rounds")


def _check_int(value, lo, hi, what):
    try:
        good = not isinstance(value, bool) and int(value) == value and lo <= int(value) <= hi
    except (TypeError, ValueError):
        good = False
    if not good:
        raise ValueError("%s must be an integer in %d..%d" % (what, lo, hi))
    return int(value)


def check_normal_k(k):
    """the neighbour count of a normal estimate (3..64) as an int, or ValueError; no GPU involved"""
    return _check_int(k, 3, KNN_INDEX_MAX_K, "the number of neighbours of a normal estimate")


def check_knn_index_arguments(points, k):
    """the shapes and ranges of knn_index, or ValueError; no GPU involved -> (n, k)"""
    shape = _shape(points)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("points must have shape [N,3]")
    if not 1 <= shape[0] < 2 ** 31:
        raise ValueError("1 <= N < 2^31 points are required")
    return shape[0], _check_int(k, 1, KNN_INDEX_MAX_K, "k")


def knn_index(frame, points, k):
    """Exact k-nearest-neighbour lists (asr_hip_knn_index; the contract is in include/asr_hip.h): row i holds the k
    smallest pairs (d2(i, j), j), the point itself included, ascending, with d2 = ((dx*dx + dy*dy) + dz*dz) in f32 -- a
    brute-force search's result, ties to the smaller index.  1 <= k <= 64; rows of a cloud with N < k are padded with -1
    and +inf.  The frame must contain the points.  -> (index int32 [N,k], squared distance f32 [N,k])"""
    n, k = check_knn_index_arguments(points, k)
    points = _dev(points, torch.float32)
    index = torch.empty((n, k), dtype=torch.int32, device=points.device)
    sqdist = torch.empty((n, k), dtype=torch.float32, device=points.device)
    context(_same_device(points)).call("asr_hip_knn_index", ctypes.byref(frame), ptr(points), i64(n), k, ptr(index),
                                       ptr(sqdist))
    return index, sqdist


def check_point_normals_arguments(points, index):
    """the shapes and ranges of point_normals, or ValueError; no GPU involved -> (n, k)"""
    shape = _shape(points)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("points must have shape [N,3]")
    if shape[0] >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 points")
    ishape = _shape(index)
    if len(ishape) != 2 or ishape[0] != shape[0]:
        raise ValueError("index must have shape [N,k]")
    if not 3 <= ishape[1] <= KNN_INDEX_MAX_K:
        raise ValueError("index must have 3 to %d columns" % KNN_INDEX_MAX_K)
    return shape[0], ishape[1]


def point_normals(points, index, return_eigenvalues=False, return_ok=False):
    """PCA normals over given neighbour lists (asr_hip_point_normals): index int32 [N,k] with 3 <= k <= 64, from knn_index
    or hand-made, entries -1 skipped.  f64 two-pass covariance of each row's points, Jacobi eigen-decomposition; the
    normal is the unit eigenvector of the smallest eigenvalue with its component of largest magnitude positive, or
    (0,0,0) with ok = False where fewer than three neighbours are valid or they are collinear (l1 <= 1e-10 l2).
    -> normals f32 [N,3][, eigenvalues f32 [N,3] ascending][, ok bool [N]]"""
    n, k = check_point_normals_arguments(points, index)
    points = _dev(points, torch.float32)
    index = _dev(index, torch.int32)
    dev = _same_device(points, index)
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    eig = torch.empty((n, 3), dtype=torch.float32, device=dev) if return_eigenvalues else None
    ok = torch.empty(n, dtype=torch.uint8, device=dev) if return_ok else None
    context(dev).call("asr_hip_point_normals", ptr(points), i64(n), ptr(index), k, ptr(normals), ptr(eig), ptr(ok))
    out = (normals,) + ((eig,) if return_eigenvalues else ()) + ((ok.bool(),) if return_ok else ())
    return out if len(out) > 1 else normals


def check_orient_arguments(points, normals, index, viewpoints):
    """the shapes and ranges of orient_normals, or ValueError; no GPU involved -> (n, k, number of viewpoints)"""
    shape = _shape(points)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("points must have shape [N,3]")
    n = shape[0]
    if n >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 points")
    if _shape(normals) != (n, 3):
        raise ValueError("normals must have shape [N,3]")
    k = 0
    if index is not None:
        ishape = _shape(index)
        if len(ishape) != 2 or ishape[0] != n or ishape[1] < 1:
            raise ValueError("index must have shape [N,k] with k >= 1")
        k = ishape[1]
    if viewpoints is None:
        if index is None:
            raise ValueError("give the neighbour lists (propagation) or viewpoints")
        if n * k >= 2 ** 32:
            raise ValueError("N k must be below 2^32")
        return n, k, 0
    vshape = _shape(viewpoints)
    if vshape == (3,) or vshape == (1, 3):
        return n, k, 1
    if vshape == (n, 3):
        return n, k, n
    raise ValueError("viewpoints must have shape [3], [1,3] or [N,3]")


def orient_normals(points, normals, index=None, viewpoints=None, return_flips=False, return_report=False):
    """Consistent signs for unoriented normals (asr_hip_normals_orient; the contract is in include/asr_hip.h).
    viewpoints [3] or [N,3]: every normal is turned towards its viewpoint.  viewpoints None: Hoppe's propagation along the
    minimum spanning forest of the graph of `index` (int32 [N,k], -1 = no entry) under the weights 1 - |n_i . n_j|, each
    tree signed so that its highest point looks up.  Points with a zero normal are skipped.
    -> normals f32 [N,3][, flips bool [N]][, dict of ints: components, flipped, skipped, rounds]"""
    n, k, nv = check_orient_arguments(points, normals, index, viewpoints)
    points = _dev(points, torch.float32)
    normals = _dev(normals, torch.float32)
    index = _dev(index, torch.int32) if index is not None else None
    if viewpoints is not None:
        viewpoints = _dev(viewpoints, torch.float32).reshape(-1, 3)
    dev = _same_device(points, normals, index, viewpoints)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    flips = torch.empty(n, dtype=torch.uint8, device=dev) if return_flips else None
    report = (i64 * 4)()
    context(dev).call("asr_hip_normals_orient", ptr(points), ptr(normals), i64(n), ptr(index), max(k, 1), ptr(viewpoints),
                      i64(nv), ptr(out), ptr(flips), report)
    res = (out,) + ((flips.bool(),) if return_flips else ())
    if return_report:
        res += (dict(zip(ORIENT_REPORT, (int(x) for x in report))),)
    return res if len(res) > 1 else out


ICP_MAX_ITERATIONS = 1000
ICP_SUMS = ("ata", "atb", "sq_residual", "sq_distance", "pairs", "mode")
ICP_REPORT = ("iterations", "converged", "degenerate", "pairs", "rmse", "fitness")


def _transform12(transform, what="transform"):
    """a rigid transform given as [3,4] or [4,4] (last row 0 0 0 1) -> 12 finite floats, the rows of (R | t)"""
    import numpy as np
    try:
        t = np.array(transform.detach().cpu().numpy() if isinstance(transform, torch.Tensor) else transform,
                     dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s must be a 3x4 or 4x4 matrix" % what)
    if t.shape == (4, 4):
        if not np.array_equal(t[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("the last row of a 4x4 %s must be 0 0 0 1" % what)
        t = t[:3]
    if t.shape != (3, 4):
        raise ValueError("%s must be a 3x4 or 4x4 matrix" % what)
    if not np.isfinite(t).all():
        raise ValueError("%s is not finite" % what)
    return t.copy()


def icp_origin(frame):
    """the centre of the frame's root cube in f64, the origin asr_hip_register_points linearises about:
    (2^20 - offset[a]) * voxel_size[21]"""
    return [float((1 << (_lib.ASR_MAX_LEVEL - 1)) - frame.offset[a]) * float(frame.voxel_size[_lib.ASR_MAX_LEVEL])
            for a in range(3)]


def check_register_arguments(target, target_normals, source, max_distance, init=None, max_iterations=50,
                             rotation_tolerance=1e-7, translation_tolerance=0.0):
    """the shapes and ranges of icp_step / register_points, or ValueError; no GPU involved
    -> (n, m, the initial transform as a float64 [3,4] array)"""
    import math
    import numpy as np
    shape = _shape(target)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("target must have shape [N,3]")
    n = shape[0]
    if not 1 <= n < 2 ** 31:
        raise ValueError("1 <= N < 2^31 target points are required")
    if target_normals is not None and _shape(target_normals) != (n, 3):
        raise ValueError("target_normals must have shape [N,3]")
    shape = _shape(source)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("source must have shape [M,3]")
    m = shape[0]
    if m >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 source points")
    try:
        cap = float(np.float32(max_distance))
    except (TypeError, ValueError):
        raise ValueError("max_distance must be a number")
    if not (math.isfinite(cap) and cap > 0.0):
        raise ValueError("max_distance must be finite and > 0 (as a float32)")
    _check_int(max_iterations, 1, ICP_MAX_ITERATIONS, "max_iterations")
    for name, tol in (("rotation_tolerance", rotation_tolerance), ("translation_tolerance", translation_tolerance)):
        try:
            good = float(tol) >= 0.0
        except (TypeError, ValueError):
            good = False
        if not good:
            raise ValueError("%s must be a number >= 0" % name)
    t = _transform12(init, "init") if init is not None else np.hstack([np.eye(3), np.zeros((3, 1))])
    return n, m, t


def _doubles(values, count):
    return (ctypes.c_double * count)(*[float(v) for v in values])


def _sums_struct(sums):
    if isinstance(sums, _lib.IcpSums):
        return sums
    s = _lib.IcpSums()
    ata, atb = [float(v) for v in sums["ata"]], [float(v) for v in sums["atb"]]
    if len(ata) != 21 or len(atb) != 6:
        raise ValueError("sums: ata has 21 entries (upper triangle, row by row) and atb 6")
    s.ata[:], s.atb[:] = ata, atb
    s.sq_residual, s.sq_distance = float(sums["sq_residual"]), float(sums["sq_distance"])
    s.pairs, s.mode = int(sums["pairs"]), int(sums["mode"])
    return s


def icp_step(frame, target, target_normals, source, transform, origin, max_distance, return_index=False):
    """One ICP step (asr_hip_icp_step; the contract is in include/asr_hip.h): every source point, moved by `transform`
    ([3,4] or [4,4], f64), is paired with its nearest target point within max_distance -- a brute-force search's result --
    and the normal equations of the linearised alignment about `origin` are summed in f64, in a fixed order: point-to-plane
    with target_normals, point-to-point with None.  -> dict(ata [21], atb [6], sq_residual, sq_distance, pairs, mode)
    [, index int32 [M], -1 = no pair]"""
    import numpy as np
    n, m, _ = check_register_arguments(target, target_normals, source, max_distance)
    t = _transform12(transform)
    origin = [float(v) for v in np.asarray(origin, dtype=np.float64).reshape(3)]
    if not all(np.isfinite(origin)):
        raise ValueError("origin is not finite")
    target = _dev(target, torch.float32)
    normals = _dev(target_normals, torch.float32) if target_normals is not None else None
    source = _dev(source, torch.float32)
    dev = _same_device(target, normals, source)
    index = torch.empty(m, dtype=torch.int32, device=dev) if return_index else None
    sums = _lib.IcpSums()
    context(dev).call("asr_hip_icp_step", ctypes.byref(frame), ptr(target), i64(n), ptr(normals), ptr(source), i64(m),
                      _doubles(t.reshape(-1), 12), _doubles(origin, 3), ctypes.c_float(max_distance), ctypes.byref(sums),
                      ptr(index))
    out = {"ata": np.array(sums.ata[:]), "atb": np.array(sums.atb[:]), "sq_residual": sums.sq_residual,
           "sq_distance": sums.sq_distance, "pairs": int(sums.pairs), "mode": int(sums.mode)}
    return (out, index) if return_index else out


def icp_update(sums, origin, transform):
    """Solves a step's normal equations and applies the result (asr_hip_icp_update, host only, no GPU): A xi = -b by
    Cholesky, xi = (omega, v), R <- Rw R, t <- Rw (t - o) + v + o.  `sums`: what icp_step returned (or a dict with the
    same keys).  -> (transform f64 [3,4], xi f64 [6], degenerate bool); a degenerate system (too few pairs, a pivot at
    rounding level) returns the transform as given and xi = 0."""
    import numpy as np
    t = _doubles(_transform12(transform).reshape(-1), 12)
    xi = (ctypes.c_double * 6)()
    rc = _lib.load().asr_hip_icp_update(ctypes.byref(_sums_struct(sums)), _doubles(np.asarray(origin).reshape(3), 3), t, xi)
    if rc < 0:
        raise AsrHipError("asr_hip_icp_update: null argument")
    return np.array(t[:]).reshape(3, 4), np.array(xi[:]), rc == 1


def register_points(frame, target, target_normals, source, max_distance, init=None, max_iterations=50,
                    rotation_tolerance=1e-7, translation_tolerance=None):
    """Rigid registration of `source` [M,3] onto `target` [N,3] by ICP (asr_hip_register_points): the target's index is
    built once, every iteration is icp_step + icp_update about the centre of the frame's root cube (icp_origin), until an
    update is within both tolerances (converged), the system is degenerate or max_iterations (1..1000) steps were taken.
    Point-to-plane with target_normals, point-to-point with None.  translation_tolerance None: 1e-7 of the root cube's edge.
    -> (transform f64 [3,4], dict(iterations, converged, degenerate, pairs, rmse, fitness))"""
    import numpy as np
    if translation_tolerance is None:
        translation_tolerance = 1e-7 * float(frame.voxel_size[0])
    n, m, t = check_register_arguments(target, target_normals, source, max_distance, init, max_iterations,
                                       rotation_tolerance, translation_tolerance)
    target = _dev(target, torch.float32)
    normals = _dev(target_normals, torch.float32) if target_normals is not None else None
    source = _dev(source, torch.float32)
    dev = _same_device(target, normals, source)
    params = _lib.IcpParams(float(max_distance), int(max_iterations), float(rotation_tolerance),
                            float(translation_tolerance))
    report = _lib.IcpReport()
    tt = _doubles(t.reshape(-1), 12)
    context(dev).call("asr_hip_register_points", ctypes.byref(frame), ptr(target), i64(n), ptr(normals), ptr(source),
                      i64(m), ctypes.byref(params), tt, ctypes.byref(report))
    out = {name: getattr(report, name) for name in ICP_REPORT}
    out["converged"], out["degenerate"] = bool(out["converged"]), bool(out["degenerate"])
    return np.array(tt[:]).reshape(3, 4), out


FPFH_DIM = 33
FEATURE_MATCH_MAX_DIM = 64
FEATURE_MATCH_TILE = 128  # rows of b per LDS tile (csrc/asr_common.h ASR_FEATURE_MATCH_TILE): the tests' tile edges
RANSAC_MAX_HYPOTHESES = 2 ** 24
RANSAC_REPORT = ("evaluated", "best_hypothesis", "inliers")


def check_point_fpfh_arguments(points, normals, index):
    """the shapes and ranges of point_fpfh, or ValueError; no GPU involved -> (n, k)"""
    n, k = check_point_normals_arguments(points, index)
    if _shape(normals) != (n, 3):
        raise ValueError("normals must have shape [N,3]")
    return n, k


def point_fpfh(points, normals, index, return_spfh=False, return_ok=False):
    """Fast point feature histograms over given neighbour lists (asr_hip_point_fpfh; the contract is in include/asr_hip.h):
    index int32 [N,k] with 3 <= k <= 64, from knn_index or hand-made, entries -1 skipped.  33 bins, theta | alpha | phi of
    PCL's Darboux frame, all in f64 from the f32 inputs in a fixed order: the same bits on every run.  A point without a
    usable normal (zero or not finite) has zero rows and ok = False and is no neighbour of anyone; ok is also False where
    no pair of the row is valid.  -> fpfh f32 [N,33][, spfh f32 [N,33]][, ok bool [N]]"""
    n, k = check_point_fpfh_arguments(points, normals, index)
    points = _dev(points, torch.float32)
    normals = _dev(normals, torch.float32)
    index = _dev(index, torch.int32)
    dev = _same_device(points, normals, index)
    fpfh = torch.empty((n, FPFH_DIM), dtype=torch.float32, device=dev)
    spfh = torch.empty((n, FPFH_DIM), dtype=torch.float32, device=dev) if return_spfh else None
    ok = torch.empty(n, dtype=torch.uint8, device=dev) if return_ok else None
    context(dev).call("asr_hip_point_fpfh", ptr(points), ptr(normals), i64(n), ptr(index), k, ptr(fpfh), ptr(spfh), ptr(ok))
    out = (fpfh,) + ((spfh,) if return_spfh else ()) + ((ok.bool(),) if return_ok else ())
    return out if len(out) > 1 else fpfh


def check_feature_match_arguments(a, b):
    """the shapes and ranges of feature_match, or ValueError; no GPU involved -> (m, n, dim)"""
    sa, sb = _shape(a), _shape(b)
    if len(sa) != 2 or len(sb) != 2 or sa[1] != sb[1]:
        raise ValueError("a and b must have the shapes [M,D] and [N,D]")
    if not 1 <= sa[1] <= FEATURE_MATCH_MAX_DIM:
        raise ValueError("the rows must have 1 to %d entries" % FEATURE_MATCH_MAX_DIM)
    if not 1 <= sb[0] < 2 ** 31:
        raise ValueError("1 <= N < 2^31 rows of b are required")
    if sa[0] >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 rows of a")
    return sa[0], sb[0], sa[1]


def feature_match(a, b):
    """The exact nearest row of b [N,D] for every row of a [M,D], 1 <= D <= 64 (asr_hip_feature_match): the squared
    distance is s = 0; s = s + (a_c - b_c)^2 over c ascending in f32, the result the smallest (s, j) -- a brute-force
    search's, ties to the smaller row.  A row of a that is not finite gets -1 / +inf, a row of b that is not finite is never
    chosen.  -> (index int32 [M], squared distance f32 [M])"""
    m, n, dim = check_feature_match_arguments(a, b)
    a = _dev(a, torch.float32)
    b = _dev(b, torch.float32)
    dev = _same_device(a, b)
    index = torch.empty(m, dtype=torch.int32, device=dev)
    sqdist = torch.empty(m, dtype=torch.float32, device=dev)
    context(dev).call("asr_hip_feature_match", ptr(a), i64(m), ptr(b), i64(n), dim, ptr(index), ptr(sqdist))
    return index, sqdist


def check_ransac_arguments(source, target, corr, max_distance, edge_ratio=0.9, hypotheses=100000, seed=0):
    """the shapes and ranges of ransac_transform, or ValueError; no GPU involved -> (m, n, c)"""
    import math
    import numpy as np
    for name, t in (("source", source), ("target", target)):
        shape = _shape(t)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError("%s must have shape [N,3]" % name)
        if not 1 <= shape[0] < 2 ** 31:
            raise ValueError("1 <= N < 2^31 %s points are required" % name)
    shape = _shape(corr)
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError("corr must have shape [C,2]")
    if not 3 <= shape[0] < 2 ** 31:
        raise ValueError("3 <= C < 2^31 correspondences are required")
    try:
        cap = float(np.float32(max_distance))
    except (TypeError, ValueError):
        raise ValueError("max_distance must be a number")
    if not (math.isfinite(cap) and cap > 0.0):
        raise ValueError("max_distance must be finite and > 0 (as a float32)")
    try:
        good = 0.0 < float(edge_ratio) <= 1.0
    except (TypeError, ValueError):
        good = False
    if not good:
        raise ValueError("edge_ratio must be a number in (0, 1]")
    _check_int(hypotheses, 1, RANSAC_MAX_HYPOTHESES, "hypotheses")
    _check_int(seed, 0, 2 ** 64 - 1, "seed")
    return _shape(source)[0], _shape(target)[0], shape[0]


def ransac_transform(source, target, corr, max_distance, edge_ratio=0.9, hypotheses=100000, seed=0):
    """RANSAC over given correspondences (asr_hip_ransac_transform; the contract is in include/asr_hip.h): corr int32 [C,2]
    of (source row, target row).  Hypothesis h draws three correspondences by splitmix64 of (seed, h), is rejected when two
    coincide, when an edge of the source triangle and its partner differ by more than edge_ratio, or when a triangle is
    degenerate; otherwise the rigid motion that maps one triangle's frame onto the other's is scored by the number of
    correspondences it brings within max_distance.  The best score wins, ties go to the smallest h: a pure function of
    the arguments.  -> (transform f64 [3,4], or None when no hypothesis passed, dict(evaluated, best_hypothesis, inliers))"""
    import numpy as np
    m, n, c = check_ransac_arguments(source, target, corr, max_distance, edge_ratio, hypotheses, seed)
    source = _dev(source, torch.float32)
    target = _dev(target, torch.float32)
    corr = _dev(corr, torch.int32)
    dev = _same_device(source, target, corr)
    params = _lib.RansacParams(float(max_distance), 0, float(edge_ratio), int(hypotheses), int(seed))
    report = _lib.RansacReport()
    tt = (ctypes.c_double * 12)()
    ctx = context(dev)
    rc = ctx.lib.asr_hip_ransac_transform(ctx._h, ptr(source), i64(m), ptr(target), i64(n), ptr(corr), i64(c),
                                          ctypes.byref(params), tt, ctypes.byref(report))
    out = {name: int(getattr(report, name)) for name in RANSAC_REPORT}
    if rc == 1 and not ctx.lib.asr_hip_last_error(ctx._h):  # no hypothesis passed: no error text
        return None, out
    ctx.check(rc)
    return np.array(tt[:]).reshape(3, 4), out


def check_global_register_arguments(source, target, source_normals=None, target_normals=None, voxel_size=None,
                                    feature_k=48, max_distance=None, hypotheses=100000, seed=0):
    """the shapes and ranges of register_points_global, or ValueError; no GPU involved -> (m, n)"""
    import math
    shapes = []
    for name, t, nrm in (("source", source, source_normals), ("target", target, target_normals)):
        shape = _shape(t)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError("%s must have shape [N,3]" % name)
        if not 3 <= shape[0] < 2 ** 31:
            raise ValueError("3 <= N < 2^31 %s points are required" % name)
        if nrm is not None and _shape(nrm) != shape:
            raise ValueError("%s_normals must have shape [N,3]" % name)
        shapes.append(shape[0])
    for name, v in (("voxel_size", voxel_size), ("max_distance", max_distance)):
        if v is None:
            continue
        try:
            good = math.isfinite(float(v)) and float(v) > 0.0
        except (TypeError, ValueError):
            good = False
        if not good:
            raise ValueError("%s must be a positive number" % name)
    _check_int(feature_k, 3, KNN_INDEX_MAX_K, "feature_k")
    _check_int(hypotheses, 1, RANSAC_MAX_HYPOTHESES, "hypotheses")
    _check_int(seed, 0, 2 ** 64 - 1, "seed")
    return shapes[0], shapes[1]


def decode_mlp_at(code, shifts, w1, b1, w2, b2, w3, rows=None, voxel_sizes=None, gradient=False):
    """UNet5.decode(shifts, code[rows]) (net_definitions_torch.py:655-666) -> values [M,2]; with gradient=True
    (values, grad [M,3]) where grad is decode_with_gradient's d values[:,0] / d shift (:668-686, unscaled).
    rows (int32 [M], None: row i) picks the code row of each shift, a row < 0 gives NaN; voxel_sizes (indexed by row)
    multiplies values[:,0] (sdf scale)."""
    code = _dev(code, torch.float32)
    shifts = _dev(shifts, torch.float32)
    w1, b1, w2, b2, w3 = (_dev(t, torch.float32) for t in (w1, b1, w2, b2, w3))
    rows = _dev(rows, torch.int32) if rows is not None else None
    sizes = _dev(voxel_sizes, torch.float32) if voxel_sizes is not None else None
    if shifts.ndim != 2 or shifts.shape[1] != 3:
        raise ValueError("shifts must have shape [M,3]")
    m = shifts.shape[0]
    if rows is None and code.shape[0] != m:
        raise ValueError("without rows, code and shifts need the same number of rows")
    if rows is not None and tuple(rows.shape) != (m,):
        raise ValueError("rows must have shape [M]")
    values = torch.empty((m, 2), dtype=torch.float32, device=shifts.device)
    grad = torch.empty((m, 3), dtype=torch.float32, device=shifts.device) if gradient else None
    dev = _same_device(code, shifts, w1, b1, w2, b2, w3, rows, sizes)
    context(dev).call("asr_hip_decode_mlp_at", ptr(code), int(code.shape[1]), ptr(rows), ptr(shifts), i64(m),
                      ptr(w1), ptr(b1), int(w1.shape[0]), ptr(w2), ptr(b2), int(w2.shape[0]), ptr(w3), ptr(sizes),
                      ptr(values), ptr(grad))
    return (values, grad) if gradient else values


def density_inlier(counts, density_percentile_threshold):
    """asr::ComputeInlierFromDensity (cpp/lib/preprocess.cpp:41-62) on host counts, literally
    (see asr_density_inlier in include/asr_hip.h)"""
    import numpy as np
    counts = np.ascontiguousarray(counts, np.int64)
    out = np.zeros(counts.shape[0], np.uint8)
    rc = _lib.load().asr_density_inlier(counts.ctypes.data_as(ctypes.c_void_p), i64(counts.shape[0]),
                                        ctypes.c_double(density_percentile_threshold),
                                        out.ctypes.data_as(ctypes.c_void_p))
    if rc:
        raise AsrHipError("asr_density_inlier failed (%d)" % rc)
    return out.astype(bool)
