"""Distance between two surfaces from point samples: accuracy / completeness, Chamfer, Hausdorff, F-score and normal
consistency -- the measures the paper this project follows reports.  Not part of the reference's module.

`a` is the surface under evaluation, `b` the reference.  With sq_ab[i] the f32 squared distance from a_i to its nearest
point in b (asr_hip.ops.nearest_point: exact, d2 = ((dx*dx + dy*dy) + dz*dz)), d_ab = sqrt(sq_ab) in f32, and the same
in the other direction; every mean and sum below is taken in float64:

    accuracy     = mean d_ab                       completeness = mean d_ba
    chamfer_l1   = (accuracy + completeness) / 2   chamfer_l2   = (mean sq_ab + mean sq_ba) / 2
    hausdorff    = max(max d_ab, max d_ba)
    precision(t) = #{sq_ab < f32(t) * f32(t)} / |a|      (strict, on the f32 squared distances: exact integer counts)
    recall(t)    = #{sq_ba < f32(t) * f32(t)} / |b|
    fscore(t)    = 2 P R / (P + R), 0 when P + R == 0
    normal_consistency = (mean |n_a . n_b[nn]| + mean |n_b . n_a[nn]|) / 2      (orientation does not matter)

The searches and the sampling run on the GPU (no CPU fallback); `from_distances`, the reduction, takes CPU or GPU input.
"""
import numpy as np
import torch

from . import _lib, ops


def _t(x, dtype):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(dtype).reshape(-1)


def from_distances(sq_ab, sq_ba, thresholds, dots_ab=None, dots_ba=None):
    """The pure reduction: sq_ab [|a|] and sq_ba [|b|] are the f32 squared nearest distances a -> b and b -> a (numpy
    arrays or tensors, CPU or GPU), thresholds a sequence of distances, dots_ab / dots_ba (both or neither) the
    products n_a . n_b[nn] and n_b . n_a[nn].  -> dict of Python floats; "thresholds", "precision", "recall" and
    "fscore" are lists in the order of `thresholds`; "normal_consistency" only with the dots."""
    sq_ab, sq_ba = _t(sq_ab, torch.float32), _t(sq_ba, torch.float32)
    if sq_ab.numel() == 0 or sq_ba.numel() == 0:
        raise ValueError("both point sets must be non-empty")
    if (dots_ab is None) != (dots_ba is None):
        raise ValueError("normal products are needed in both directions or in neither")
    d_ab, d_ba = torch.sqrt(sq_ab).double(), torch.sqrt(sq_ba).double()
    out = {"accuracy": float(d_ab.mean()), "completeness": float(d_ba.mean())}
    out["chamfer_l1"] = (out["accuracy"] + out["completeness"]) / 2
    out["chamfer_l2"] = (float(sq_ab.double().mean()) + float(sq_ba.double().mean())) / 2
    out["hausdorff"] = max(float(d_ab.max()), float(d_ba.max()))
    out["thresholds"], out["precision"], out["recall"], out["fscore"] = [], [], [], []
    for t in thresholds:
        t2 = float(np.float32(t) * np.float32(t))  # the f32 product, exactly representable
        p = int((sq_ab < t2).sum()) / sq_ab.numel()
        r = int((sq_ba < t2).sum()) / sq_ba.numel()
        out["thresholds"].append(float(t))
        out["precision"].append(p)
        out["recall"].append(r)
        out["fscore"].append(2 * p * r / (p + r) if p + r > 0 else 0.0)
    if dots_ab is not None:
        dots_ab, dots_ba = _t(dots_ab, torch.float32), _t(dots_ba, torch.float32)
        if dots_ab.numel() != sq_ab.numel() or dots_ba.numel() != sq_ba.numel():
            raise ValueError("one normal product per distance is needed")
        out["normal_consistency"] = (float(dots_ab.abs().double().mean()) + float(dots_ba.abs().double().mean())) / 2
    return out


def _points(x, name):
    x = ops._dev(x, torch.float32)
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError("%s must have shape [N,3]" % name)
    if x.shape[0] == 0:
        raise ValueError("%s must not be empty" % name)
    return x


def search_frame(points):
    """the acceleration grid of a search among `points` (GPU tensor [N,3]): their bounding box with a small margin"""
    t = points.t().contiguous()  # reductions over the contiguous dimension (see synth.bounding_box)
    lo, hi = torch.stack([t.amin(dim=1), t.amax(dim=1)]).cpu().numpy()
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("points contain non-finite values")
    m = np.float32(max(1e-3, 1e-3 * float((hi - lo).max())))
    return _lib.frame_init(lo - m, hi + m)


def point_set_metrics(a, b, thresholds, normals_a=None, normals_b=None):
    """Metrics between the point sets a [Na,3] and b [Nb,3] (GPU tensors), see the module docstring; with unit normals
    on both sides also the normal consistency.  Two nearest-point searches, one per direction."""
    a, b = _points(a, "a"), _points(b, "b")
    if (normals_a is None) != (normals_b is None):
        raise ValueError("normals are needed on both sides or on neither")
    idx_ab, sq_ab = ops.nearest_point(search_frame(b), b, a)
    idx_ba, sq_ba = ops.nearest_point(search_frame(a), a, b)
    dots_ab = dots_ba = None
    if normals_a is not None:
        na, nb = ops._dev(normals_a, torch.float32), ops._dev(normals_b, torch.float32)
        if na.shape != a.shape or nb.shape != b.shape:
            raise ValueError("normals must have the shape of their points")
        dots_ab = (na * nb[idx_ab.long()]).sum(1)
        dots_ba = (nb * na[idx_ba.long()]).sum(1)
    return from_distances(sq_ab, sq_ba, thresholds, dots_ab, dots_ba)


def _is_mesh(reference):
    if not isinstance(reference, (tuple, list)) or len(reference) != 2 or reference[1] is None:
        return False
    second = reference[1]
    dtype = second.dtype if isinstance(second, torch.Tensor) else np.asarray(second).dtype
    return dtype in (torch.int32, torch.int64) or (not isinstance(dtype, torch.dtype) and np.issubdtype(dtype, np.integer))


def mesh_metrics(vertices, triangles, reference, num_samples, thresholds, seed=0):
    """Metrics between the triangle mesh (vertices, triangles) and `reference`, both as point samples: num_samples
    area-weighted points of the mesh (ops.mesh_sample with `seed`, face normals included) against
      - (vertices, triangles) of a reference mesh (integer second entry): num_samples points of it, seed + 1, or
      - reference points [N,3], or (points, normals) / (points, None): as they are.
    Normal consistency is reported when the reference has normals."""
    pa, na = ops.mesh_sample(vertices, triangles, num_samples, seed=seed, normals=True)
    if _is_mesh(reference):
        pb, nb = ops.mesh_sample(reference[0], reference[1], num_samples, seed=int(seed) + 1, normals=True)
    elif isinstance(reference, (tuple, list)):
        pb, nb = reference
    else:
        pb, nb = reference, None
    if nb is None:
        na = None
    return point_set_metrics(pa, pb, thresholds, na, nb)
