"""numpy restatement of the contract of asr_hip_points_merge_count / _fill (include/asr_hip.h): one point
per occupied octree cell, optionally per side of it.  Needs no GPU; the frame is the ctypes struct of
asr_hip._lib.frame_init (host code).  The cell arithmetic is mesh_simplify_ref.vertex_cells, imported, not restated.
Every sum runs in f64 in ascending input index (np.add.at is unbuffered and walks its indices in order), which is the
order of the library's chain for clusters of at most ASR_MERGE_LONG_CLUSTER members.  Also the clouds the tests share."""
import numpy as np

import mesh_simplify_ref as R

MAX_LEVEL = R.MAX_LEVEL
MAX_CHANNELS = 16
REPORT_FIELDS = ("clusters", "dropped", "largest_cluster", "split_cells")


def inside(frame, points):
    """bool [N]: the points that are kept -- finite and inside the root cube, by the f32 test of the cell arithmetic
    (vertex_cells refuses every other point, so a mask that kept too much would raise there)"""
    _, ivs, off = R.frame_arrays(frame)
    p = np.asarray(points, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor(p * ivs[MAX_LEVEL])
        lim = np.float32(1 << MAX_LEVEL)
        ok = (t >= (-off).astype(np.float32)) & (t < lim - off.astype(np.float32))
    return ok.all(1)


def merge(frame, points, normals=None, radii=None, attributes=None, level=None, levels=None, split_sides=False):
    """-> dict: points f32 [M,3]; normals f32 [M,3], radii f32 [M], attributes f32 [M,C] (None where the input is);
    counts int32 [M]; cluster int32 [N]; report {clusters, dropped, largest_cluster, split_cells}; and for the tests
    keys uint64 [M], sides int [M], levels int [M] of the clusters and normal_ok bool [M]: |sum n| >= 1e-3 sum |n|, or
    the sum has no finite positive length and the first member's normal was copied."""
    p = np.ascontiguousarray(points, np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must have shape [N,3]")
    n = len(p)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(n, 3)
    rad = None if radii is None else np.ascontiguousarray(radii, np.float32).reshape(n)
    att = None
    if attributes is not None:
        att = np.ascontiguousarray(attributes, np.float32).reshape(n, -1)
        if not 1 <= att.shape[1] <= MAX_CHANNELS:
            raise ValueError("1 to 16 attribute channels")
    if (level is None) == (levels is None):
        raise ValueError("give exactly one of level and levels")
    lv = np.full(n, level, np.int64) if levels is None else np.asarray(levels, np.int64).reshape(-1)
    if len(lv) != n:
        raise ValueError("levels must have one entry per point")
    if (levels is None and not 0 <= level <= MAX_LEVEL) or (lv < 0).any() or (lv > MAX_LEVEL).any():
        raise ValueError("level is not in 0..21")
    if split_sides and nrm is None:
        raise ValueError("split_sides needs normals")
    kept = np.nonzero(inside(frame, p))[0]  # ascending input index
    cluster = np.full(n, -1, np.int32)
    out = {"normals": None, "radii": None, "attributes": None}
    if len(kept) == 0:
        out.update(points=np.zeros((0, 3), np.float32), counts=np.zeros(0, np.int32), cluster=cluster,
                   keys=np.zeros(0, np.uint64), sides=np.zeros(0, np.int64), levels=np.zeros(0, np.int64),
                   normal_ok=np.zeros(0, bool), report=dict(clusters=0, dropped=n, largest_cluster=0, split_cells=0))
        if nrm is not None:
            out["normals"] = np.zeros((0, 3), np.float32)
        if rad is not None:
            out["radii"] = np.zeros(0, np.float32)
        if att is not None:
            out["attributes"] = np.zeros((0, att.shape[1]), np.float32)
        return out
    _, key = R.vertex_cells(frame, p[kept], lv[kept])
    ckey, first_in_cell, cell = np.unique(key, return_index=True, return_inverse=True)  # first = smallest input index
    cell = cell.reshape(-1)
    side = np.zeros(len(kept), np.int64)
    if split_sides:
        a, r = nrm[kept], nrm[kept[first_in_cell[cell]]]
        with np.errstate(invalid="ignore", over="ignore"):
            d = (a[:, 0] * r[:, 0] + a[:, 1] * r[:, 1]) + a[:, 2] * r[:, 2]  # f32, one rounding per operation
            side = (d < np.float32(0)).astype(np.int64)
    pair, first, cl = np.unique(2 * cell + side, return_index=True, return_inverse=True)  # ascending key, side 0 first
    cl = cl.reshape(-1)
    m = len(pair)
    cluster[kept] = cl
    count = np.bincount(cl, minlength=m)
    single = count == 1
    head = kept[first]  # first member of every cluster

    def mean(x):
        x = x.reshape(n, -1)
        s = np.zeros((m, x.shape[1]))
        with np.errstate(invalid="ignore", over="ignore"):
            np.add.at(s, cl, x[kept].astype(np.float64))
            o = (s / count[:, None]).astype(np.float32)
        o[single] = x[head[single]]
        return o

    out["points"] = mean(p)
    if rad is not None:
        out["radii"] = mean(rad).reshape(m)
    if att is not None:
        out["attributes"] = mean(att)
    normal_ok = np.ones(m, bool)
    if nrm is not None:
        s = np.zeros((m, 3))
        total = np.zeros(m)
        x = nrm[kept].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            np.add.at(s, cl, x)
            np.add.at(total, cl, np.sqrt((x * x).sum(1)))
            length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
            good = np.isfinite(length) & (length > 0)
            o = (s / length[:, None]).astype(np.float32)
            normal_ok = ~good | (length >= 1e-3 * total)
        copy = ~good | single
        o[copy] = nrm[head[copy]]
        out["normals"] = o
    out.update(counts=count.astype(np.int32), cluster=cluster, keys=ckey[pair // 2], sides=pair % 2,
               levels=lv[head], normal_ok=normal_ok,
               report=dict(clusters=int(m), dropped=int(n - len(kept)), largest_cluster=int(count.max()),
                           split_cells=int(m - len(ckey))))
    return out


def boxes(frame, points, levels, result):
    """(lo, hi) f64 [M,3]: the cell of every merged point (levels: int [N] or one int)"""
    keep = result["cluster"] >= 0
    lv = np.broadcast_to(np.asarray(levels, np.int64), (len(points),))
    return R.cluster_boxes(frame, np.asarray(points, np.float32)[keep], lv[keep], result["cluster"][keep],
                           len(result["points"]))


def ulp_distance(a, b):
    """number of f32 values between a and b, elementwise (0: the same value or both NaN; huge: one NaN)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)  # -0.0 and +0.0 both map to 0

    d = np.abs(ordered(a) - ordered(b))
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na & nb, 0, np.where(na | nb, np.int64(1) << 40, d))


# ---- the clouds of the tests ------------------------------------------------------------------------------------------
UNIT_BOX = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])


def unit_frame():
    from asr_hip import _lib
    return _lib.frame_init(*UNIT_BOX)


def margin_frame(points):
    """the frame merge_points uses: around the finite points, with a margin of a thousandth of the longest side"""
    from asr_hip import _lib
    p = np.asarray(points, np.float32)
    p = p[np.isfinite(p).all(1)]
    lo, hi = p.min(0), p.max(0)
    m = max(1e-3, 1e-3 * float((hi - lo).max()))
    return _lib.frame_init(lo - np.float32(m), hi + np.float32(m))


def cell_corner(frame, level, cell):
    """f64 [3]: the lower corner of integer cell [3] of `level`, and the cell's edge"""
    vs, _, off = R.frame_arrays(frame)
    s = MAX_LEVEL - level
    return ((np.asarray(cell, np.int64) << s) - off) * np.float64(vs[MAX_LEVEL]), float(vs[level])


def root_cell(frame, level, position):
    """the integer cell of `level` that holds a position (one point)"""
    cell, _ = R.vertex_cells(frame, np.asarray(position, np.float32).reshape(1, 3), np.array([level]))
    return cell[0]


def _hemisphere_normals(rng, n):
    """unit normals in a cone round +z (x, y in +-0.5 to z in 1..2): any two have a positive product, no sum cancels"""
    v = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(1.0, 2.0, (n, 1))], 1)
    return (v / np.sqrt((v * v).sum(1, keepdims=True))).astype(np.float32)


def _extras(rng, n, channels=3):
    """positive radii f32 [n] and attributes f32 [n,channels] (colour-like, 0..255)"""
    return (rng.uniform(0.01, 0.05, n).astype(np.float32),
            rng.uniform(0.0, 255.0, (n, channels)).astype(np.float32))


def sized_clusters(sizes, level=4, seed=5):
    """-> (frame, points, normals, radii, attributes): one cluster of every given size, each in its own cell of `level`
    of the unit box (cells (2k+1, 3, 5): never neighbours), the points well inside the cell, the input order shuffled"""
    rng = np.random.default_rng(seed)
    frame = unit_frame()
    pts = []
    for k, size in enumerate(sizes):
        lo, h = cell_corner(frame, level, root_cell(frame, level, [(2 * k + 1.5) / 16, 3.5 / 16, 5.5 / 16]))
        pts.append(lo + h * rng.uniform(0.1, 0.9, (size, 3)))
    pts = np.concatenate(pts).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    rad, att = _extras(rng, len(pts))
    return frame, pts, _hemisphere_normals(rng, len(pts)), rad, att


def one_cell_cloud(n=50000, seed=6):
    """n points of the unit box (all of them one cluster at level 0) with normals, radii and 3 attribute channels"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.05, 0.95, (n, 3)).astype(np.float32)
    rad, att = _extras(rng, n)
    return unit_frame(), pts, _hemisphere_normals(rng, n), rad, att


WALL_LEVEL = 4


def thin_wall(zero_first=False, seed=7):
    """-> (frame, points, normals, level): two sheets with opposite normals in the same layer of cells of WALL_LEVEL of
    the unit box, 0.2 cells apart: the upper one (normal +z) with 3 x 3 points per cell, the lower one (normal -z) with
    2 x 2 -- the unequal numbers keep the normal sum of an unsplit cell away from zero.  6 x 6 cells are occupied; the
    input order is shuffled.  zero_first: the first member of the cell that holds point 0 gets a zero normal (no member
    of that cell is then on side 1)."""
    rng = np.random.default_rng(seed)
    frame = unit_frame()
    base = root_cell(frame, WALL_LEVEL, [4.5 / 16, 4.5 / 16, 7.5 / 16])
    lo, h = cell_corner(frame, WALL_LEVEL, base)
    pts, nrm = [], []
    for per_cell, z, nz in ((3, 0.6, 1.0), (2, 0.4, -1.0)):
        g = (np.arange(6 * per_cell) + 0.5) / per_cell  # in cells
        x, y = np.meshgrid(g, g, indexing="ij")
        q = np.stack([x.reshape(-1), y.reshape(-1), np.full(x.size, z)], 1)
        pts.append(lo + h * q)
        nrm.append(np.tile([0.0, 0.0, nz], (len(q), 1)))
    pts, nrm = np.concatenate(pts).astype(np.float32), np.concatenate(nrm).astype(np.float32)
    order = rng.permutation(len(pts))
    pts, nrm = pts[order], nrm[order]
    if zero_first:
        _, key = R.vertex_cells(frame, pts, np.full(len(pts), WALL_LEVEL))
        nrm[np.nonzero(key == key[0])[0][0]] = 0.0  # (point 0 itself: the smallest index of its cell)
    return frame, pts, nrm, WALL_LEVEL


def scan_case(n=20000, seed=11):
    """-> (frame, points, normals, radii, attributes, level): synth.scan_cloud with its 24-NN radii and 3 attribute
    channels in the frame merge_points would use, and the level at which the mean cluster has closest to 4 members"""
    from asr_hip import synth
    p, q = synth.scan_cloud(n, seed=seed, device="cpu")
    pts, nrm = p.numpy(), q.numpy()
    rad = synth.knn_radii(pts, 24)
    rng = np.random.default_rng(seed)
    att = rng.uniform(0.0, 255.0, (len(pts), 3)).astype(np.float32)
    frame = margin_frame(pts)
    best = min(range(MAX_LEVEL + 1), key=lambda l: abs(
        len(pts) / len(np.unique(R.vertex_cells(frame, pts, np.full(len(pts), l))[1])) - 4.0))
    return frame, pts, nrm, rad, att, best


def radius_levels(frame, radii, factor):
    """the level asr_hip_point_keys selects for a point of radius factor * radii[i] (scale 1, depth 21): one above the
    first level whose voxel size is smaller than that radius, the deepest level when there is none (a NaN radius)"""
    vs, _, _ = R.frame_arrays(frame)
    scale = np.float32(factor) * np.asarray(radii, np.float32)
    lv = np.full(len(scale), MAX_LEVEL, np.int64)
    with np.errstate(invalid="ignore"):
        for l in range(MAX_LEVEL, -1, -1):
            lv[vs[l] < scale] = max(l - 1, 0)
    return lv
