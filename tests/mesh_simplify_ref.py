"""numpy float64 restatement of the contract of asr_hip_mesh_simplify_count / _fill (include/asr_hip.h):
octree vertex clustering with quadric placement.  Needs no GPU; the frame is the ctypes struct of
asr_hip._lib.frame_init (host code).  Also the small meshes the tests share."""
import numpy as np

MAX_LEVEL = 21


def dilate21(x):
    x = np.asarray(x, np.uint64)
    x = (x | (x << np.uint64(32))) & np.uint64(0x001F00000000FFFF)
    x = (x | (x << np.uint64(16))) & np.uint64(0x00FF0000FF0000FF)
    x = (x | (x << np.uint64(8))) & np.uint64(0xF00F00F00F00F00F)
    x = (x | (x << np.uint64(4))) & np.uint64(0x30C30C30C30C30C3)
    x = (x | (x << np.uint64(2))) & np.uint64(0x9249249249249249)
    return x


def coord_key(cell, level):
    """location code of integer cells [N,3] at levels [N]: Morton code with a marker bit above it"""
    cell = np.asarray(cell, np.uint64)
    m = dilate21(cell[:, 0]) | (dilate21(cell[:, 1]) << np.uint64(1)) | (dilate21(cell[:, 2]) << np.uint64(2))
    return m | (np.uint64(1) << (np.uint64(3) * np.asarray(level, np.uint64)))


def frame_arrays(frame):
    return (np.array(frame.voxel_size[:], np.float32), np.array(frame.inv_voxel_size[:], np.float32),
            np.array(frame.offset[:], np.int64))


def vertex_cells(frame, vertices, lv):
    """-> (cell int64 [N,3], key uint64 [N]); ValueError for a vertex outside the frame"""
    _, ivs, off = frame_arrays(frame)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor(v * ivs[MAX_LEVEL])  # f32
        lim = np.float32(1 << MAX_LEVEL)
        ok = (t >= (-off).astype(np.float32)) & (t < lim - off.astype(np.float32))
    if not ok.all():
        raise ValueError("vertex outside the frame")
    c21 = t.astype(np.int64) + off
    cell = c21 >> (MAX_LEVEL - lv)[:, None]
    return cell, coord_key(cell, lv)


def simplify(frame, vertices, triangles, level=None, levels=None, mean_only=False, corner_order=None):
    """-> (vertices f32 [V',3], triangles int32 [T',3], vertex_map int32 [V]).  mean_only: the plain mean instead of
    the quadric (for comparison); corner_order: a permutation of the 3T corners, the order in which they are summed."""
    vs, _, off = frame_arrays(frame)
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    nv, nt = len(v), len(tri)
    if (level is None) == (levels is None):
        raise ValueError("give exactly one of level and levels")
    lv = np.full(nv, level, np.int64) if levels is None else np.asarray(levels, np.int64).reshape(-1)
    if len(lv) != nv:
        raise ValueError("levels must have one entry per vertex")
    if (levels is None and not 0 <= level <= MAX_LEVEL) or (lv < 0).any() or (lv > MAX_LEVEL).any():
        raise ValueError("level is not in 0..21")
    if nt and (nv == 0 or tri.min() < 0 or tri.max() >= nv):
        raise ValueError("triangle index out of range")
    vmap = np.full(nv, -1, np.int32)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), vmap)
    if nv == 0:
        return empty
    cell, key = vertex_cells(frame, v, lv)
    ckey, first, cl = np.unique(key, return_index=True, return_inverse=True)  # clusters in ascending key order
    cl = cl.reshape(-1)
    nc = len(ckey)
    if nt == 0:
        return empty
    # triangles
    ct = cl[tri]
    good = (ct[:, 0] != ct[:, 1]) & (ct[:, 1] != ct[:, 2]) & (ct[:, 0] != ct[:, 2])
    idx = np.nonzero(good)[0]
    _, firsts = np.unique(np.sort(ct[idx], axis=1), axis=0, return_index=True)  # first occurrence = smallest index
    surv = np.sort(idx[firsts])
    used = np.zeros(nc, bool)
    used[ct[surv].reshape(-1)] = True
    out_index = np.cumsum(used) - 1
    vmap = np.where(used[cl], out_index[cl], -1).astype(np.int32)
    t_out = out_index[ct[surv]].astype(np.int32).reshape(-1, 3)
    # positions
    ccell, clev = cell[first], lv[first]
    s = MAX_LEVEL - clev
    centre = (((ccell << s[:, None]) - off).astype(np.float64) + 0.5 * (2.0 ** s)[:, None]) * np.float64(vs[MAX_LEVEL])
    h = vs[clev].astype(np.float64)
    count = np.bincount(cl, minlength=nc)
    p = v.astype(np.float64)
    m = np.zeros((nc, 3))
    np.add.at(m, cl, p - centre[cl])
    m /= count[:, None]
    A = np.zeros((nc, 3, 3))
    b = np.zeros((nc, 3))
    q = np.arange(3 * nt) if corner_order is None else np.asarray(corner_order)
    t_of, c_of = q // 3, cl[tri.reshape(-1)[q]]
    p0 = p[tri[t_of, 0]] - centre[c_of]
    p1 = p[tri[t_of, 1]] - centre[c_of]
    p2 = p[tri[t_of, 2]] - centre[c_of]
    N = np.cross(p1 - p0, p2 - p0)
    ln = np.sqrt((N * N).sum(1))
    ok = ln > 0
    N, ln, p0, c_ok = N[ok], ln[ok], p0[ok], c_of[ok]
    np.add.at(A, c_ok, N[:, :, None] * N[:, None, :] / (2 * ln)[:, None, None])
    np.add.at(b, c_ok, (-(N * p0).sum(1) / (2 * ln))[:, None] * N)
    trA = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
    x = m.copy()
    solve = (trA > 0) & (not mean_only)
    if solve.any():
        eps = 1e-3 * trA[solve] / 3
        M = A[solve] + eps[:, None, None] * np.eye(3)
        rhs = -b[solve] + eps[:, None] * m[solve]
        x[solve] = np.linalg.solve(M, rhs[:, :, None])[:, :, 0]
    x = np.clip(x, -h[:, None] / 2, h[:, None] / 2)
    pos = (centre + x).astype(np.float32)
    single = count == 1
    pos[single] = v[first[single]]
    return pos[used], t_out, vmap


def cluster_boxes(frame, vertices, levels, vmap, num_out):
    """(lo, hi) f64 [num_out,3]: the cell of every output vertex"""
    vs, _, off = frame_arrays(frame)
    lv = np.asarray(levels, np.int64)
    cell, _ = vertex_cells(frame, vertices, lv)
    keep = vmap >= 0
    lo = np.zeros((num_out, 3))
    hi = np.zeros((num_out, 3))
    s = (MAX_LEVEL - lv[keep])[:, None]
    w = np.float64(vs[MAX_LEVEL])
    lo[vmap[keep]] = ((cell[keep] << s) - off) * w
    hi[vmap[keep]] = (((cell[keep] + 1) << s) - off) * w
    return lo, hi


# ---- the meshes of the tests -------------------------------------------------------------------------------------
SPHERE_BOX = ([-1.3, -1.2, -1.25], [1.3, 1.2, 1.35])


def uv_sphere(nlat=30, nlon=60):
    """unit sphere: 2 poles + nlat rings of nlon vertices; 2 nlon nlat triangles, outward"""
    th = np.pi * np.arange(1, nlat + 1) / (nlat + 1)
    ph = 2 * np.pi * np.arange(nlon) / nlon
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)),
                     np.outer(np.cos(th), np.ones(nlon))], -1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]).astype(np.float32)
    tri = []
    at = lambda i, j: 1 + i * nlon + j % nlon  # noqa: E731
    south = len(v) - 1
    for j in range(nlon):
        tri.append((0, at(0, j), at(0, j + 1)))
        for i in range(nlat - 1):
            tri.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
            tri.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
        tri.append((south, at(nlat - 1, j + 1), at(nlat - 1, j)))
    return v, np.array(tri, np.int32)


def grid_mesh(n, zfun):
    """n x n vertices over [-0.5, 0.5]^2, z = zfun(x, y), two triangles per square"""
    g = np.linspace(-0.5, 0.5, n)
    x, y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([x, y, zfun(x, y)], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1)
    tri = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)])
    return v, tri.astype(np.int32)


GRID_BOX = ([-0.65, -0.65, -0.65], [0.65, 0.65, 0.65])
ROOF_X = 3.0 / 32


def plane_mesh():
    return grid_mesh(33, lambda x, y: np.full_like(x, 0.25))


def roof_mesh():
    return grid_mesh(65, lambda x, y: 0.25 - np.abs(x - ROOF_X))


def roof_distance(p):
    """vertical distance of points [N,3] from the roof z = 0.25 - |x - ROOF_X|: never less than the true distance"""
    p = np.asarray(p, np.float64)
    return np.abs(p[:, 2] - (0.25 - np.abs(p[:, 0] - ROOF_X)))
