"""numpy restatement of the contracts of asr_hip_mesh_edges_count / _fill, asr_hip_mesh_topology and asr_hip_mesh_smooth
(include/asr_hip.h): the edge table, the topology report and Taubin smoothing.  Needs no GPU.  Also the
small meshes the tests share (the sphere, the plane and the grids come from mesh_simplify_ref)."""
import numpy as np

import mesh_simplify_ref as S

BOUNDARY_MODES = ("free", "pinned", "along")
SMOOTH_CUT = 128  # rows longer than this take the library's wave-per-row kernel


def _tri(triangles, num_vertices):
    tri = np.ascontiguousarray(triangles, np.int64).reshape(-1, 3)
    nv = int(num_vertices)
    if len(tri) and (nv <= 0 or tri.min() < 0 or tri.max() >= nv):
        raise ValueError("triangle index out of range")
    return tri, nv


def edge_table(triangles, num_vertices):
    """-> (edges int32 [E,2] ascending (lo, hi), uses int32 [E], forward int32 [E])"""
    tri, nv = _tri(triangles, num_vertices)
    good = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    t = tri[good]
    u = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    v = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    key, inverse, uses = np.unique(lo * max(nv, 1) + hi, return_inverse=True, return_counts=True)
    forward = np.bincount(inverse.reshape(-1), weights=(u < v), minlength=len(key))
    edges = np.stack([key // max(nv, 1), key % max(nv, 1)], 1)
    return edges.astype(np.int32).reshape(-1, 2), uses.astype(np.int32), forward.astype(np.int32)


def _components(n, a, b, members):
    """number of connected components among the vertices `members` (bool [n]) under the edges (a, b)"""
    label = np.arange(n)
    while True:  # min-label propagation with pointer jumping
        m = np.minimum(label[a], label[b])
        new = label.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            break
        label = new
    return int(len(np.unique(label[members])))


def topology(triangles, num_vertices):
    """the dict of ops.mesh_topology"""
    tri, nv = _tri(triangles, num_vertices)
    edges, uses, forward = edge_table(tri, nv)
    good = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    used = np.zeros(nv, bool)
    used[edges.reshape(-1)] = True
    bnd = edges[uses == 1]
    on_bnd = np.zeros(nv, bool)
    on_bnd[bnd.reshape(-1)] = True
    out = {
        "num_vertices": nv,
        "used_vertices": int(used.sum()),
        "triangles": int(good.sum()),
        "degenerate_triangles": int((~good).sum()),
        "edges": len(edges),
        "boundary_edges": int((uses == 1).sum()),
        "nonmanifold_edges": int((uses >= 3).sum()),
        "inconsistent_edges": int(((uses == 2) & (forward != 1)).sum()),
        "components": _components(nv, edges[:, 0], edges[:, 1], used),
        "boundary_loops": _components(nv, bnd[:, 0], bnd[:, 1], on_bnd),
    }
    out["euler"] = out["used_vertices"] - out["edges"] + out["triangles"]
    out["edge_manifold"] = out["nonmanifold_edges"] == 0
    out["oriented"] = out["inconsistent_edges"] == 0
    out["watertight"] = (out["boundary_edges"] == 0 and out["nonmanifold_edges"] == 0 and out["inconsistent_edges"] == 0
                         and out["triangles"] > 0)
    out["genus"] = (2 * out["components"] - out["euler"]) // 2 if out["watertight"] else None
    return out


def neighbour_rows(triangles, num_vertices):
    """directed edges sorted by (source, target): (source, target, feature bool)"""
    edges, uses, _ = edge_table(triangles, num_vertices)
    src = np.concatenate([edges[:, 0], edges[:, 1]]).astype(np.int64)
    dst = np.concatenate([edges[:, 1], edges[:, 0]]).astype(np.int64)
    feat = np.concatenate([uses != 2, uses != 2])
    order = np.lexsort((dst, src))
    return src[order], dst[order], feat[order]


def _ranks(src):
    """position of every entry inside its row (src ascending)"""
    if len(src) == 0:
        return np.zeros(0, np.int64)
    start = np.r_[0, np.flatnonzero(src[1:] != src[:-1]) + 1]
    length = np.diff(np.r_[start, len(src)])
    return np.arange(len(src)) - np.repeat(start, length)


def smooth(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, boundary="along", descending=False):
    """-> vertices f32 [V,3].  f64 throughout, every row summed sequentially in ascending (descending=True: descending)
    neighbour order, one cast to f32 at the end; a vertex that never moves keeps its input bits."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    nv = len(v)
    tri, _ = _tri(triangles, nv)
    if not 0 <= int(iterations) <= 1000 or not 0 < lam <= 1 or not (np.isfinite(mu) and mu <= 0) or boundary not in BOUNDARY_MODES:
        raise ValueError("bad smoothing argument")
    if not np.isfinite(v).all():
        raise ValueError("a vertex is not finite")
    src, dst, feat = neighbour_rows(tri, nv)
    vfeat = np.zeros(nv, bool)
    vfeat[src[feat]] = True
    if boundary == "pinned":
        keep = ~vfeat[src]
    elif boundary == "along":
        keep = ~vfeat[src] | feat
    else:
        keep = np.ones(len(src), bool)
    src, dst = src[keep], dst[keep]
    if descending:
        order = np.lexsort((-dst, src))
        src, dst = src[order], dst[order]
    rank = _ranks(src)
    count = np.bincount(src, minlength=nv)
    moves = count > 0
    by_rank = [np.flatnonzero(rank == k) for k in range(int(rank.max()) + 1 if len(rank) else 0)]
    p = v.astype(np.float64)
    for _ in range(int(iterations)):
        for f in ((lam, mu) if mu != 0 else (lam,)):
            s = np.zeros((nv, 3))
            for sel in by_rank:  # one entry per row at a time: a sequential sum per row
                s[src[sel]] += p[dst[sel]]
            mean = s[moves] / count[moves][:, None]
            q = p.copy()
            q[moves] = p[moves] + f * (mean - p[moves])
            p = q
    out = p.astype(np.float32)
    out[~moves] = v[~moves]
    return out


# ---- the meshes of the tests -------------------------------------------------------------------------------------
def holed_plane():
    """plane_mesh() without the triangles whose centroid has |x| < 0.1 and |y| < 0.1: a disc with one hole"""
    v, t = S.plane_mesh()
    c = v[t].astype(np.float64).mean(1)
    return v, np.ascontiguousarray(t[~((np.abs(c[:, 0]) < 0.1) & (np.abs(c[:, 1]) < 0.1))])


def torus(nu=24, nv=12, big=1.0, small=0.35):
    u = 2 * np.pi * np.arange(nu) / nu
    w = 2 * np.pi * np.arange(nv) / nv
    uu, ww = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(big + small * np.cos(ww)) * np.cos(uu), (big + small * np.cos(ww)) * np.sin(uu), small * np.sin(ww)], -1)
    at = lambda i, j: (i % nu) * nv + j % nv  # noqa: E731
    tri = []
    for i in range(nu):
        for j in range(nv):
            tri.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
            tri.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
    return v.reshape(-1, 3).astype(np.float32), np.array(tri, np.int32)


def two_spheres():
    v, t = S.uv_sphere()
    return np.concatenate([v, v + np.float32([3, 0, 0])]).astype(np.float32), np.concatenate([t, t + len(v)]).astype(np.int32)


def three_on_one_edge():
    """three triangles around the edge (0, 1)"""
    v = np.float32([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0.2], [0.5, 0, 1]])
    return v, np.int32([[0, 1, 2], [1, 0, 3], [0, 1, 4]])


def flipped_sphere(which=100):
    v, t = S.uv_sphere()
    t = t.copy()
    t[which] = t[which, [0, 2, 1]]
    return v, t


def duplicate_and_degenerate():
    """the sphere with triangle 7 twice, a triangle with two equal corners and one with three"""
    v, t = S.uv_sphere()
    return v, np.concatenate([t, t[[7]], [[5, 5, 9]], [[11, 11, 11]]]).astype(np.int32)


def unused_tail():
    """the sphere followed by 70 vertices no triangle references"""
    v, t = S.uv_sphere()
    return np.concatenate([v, np.full((70, 3), 2.5, np.float32)]), t


def renumbered_sphere(seed=3):
    v, t = S.uv_sphere()
    perm = np.random.default_rng(seed).permutation(len(v))  # old -> new
    v2 = np.empty_like(v)
    v2[perm] = v
    return v2, perm[t].astype(np.int32)


def fan(spokes, centre=(0.0, 0.0, 0.0), closed=False):
    """a hub (vertex 0) with `spokes` rim vertices on a wavy circle: an open fan of spokes - 1 triangles (the hub and the
    rim are boundary), or a closed one of `spokes` triangles (the hub is interior).  The hub's row has `spokes` entries."""
    th = 2 * np.pi * np.arange(spokes) / (spokes + (0 if closed else 1))
    rim = np.stack([np.cos(th), np.sin(th), 0.1 * np.sin(5 * th)], 1)
    v = (np.concatenate([[[0, 0, 0.3]], rim]) + np.asarray(centre)).astype(np.float32)
    n = spokes if closed else spokes - 1
    tri = [(0, 1 + i, 1 + (i + 1) % spokes) for i in range(n)]
    return v, np.array(tri, np.int32)


def fans_around_the_cut():
    """closed fans whose hubs have SMOOTH_CUT - 1, SMOOTH_CUT and SMOOTH_CUT + 1 neighbours, an open fan of 5 000 spokes, two
    isolated vertices and a vertex used by a degenerate triangle only"""
    vs, ts, base = [], [], 0
    for k, (spokes, closed) in enumerate([(SMOOTH_CUT - 1, True), (SMOOTH_CUT, True), (SMOOTH_CUT + 1, True), (5000, False)]):
        v, t = fan(spokes, centre=(3.0 * k, 0.0, 0.0), closed=closed)
        vs.append(v)
        ts.append(t + base)
        base += len(v)
    vs.append(np.float32([[0.5, 7, 1], [-0.25, 7, 2], [1.5, 7, 3]]))
    ts.append(np.int32([[base + 2, base + 2, 0]]))
    return np.concatenate(vs).astype(np.float32), np.concatenate(ts).astype(np.int32)


def noisy_sphere(sigma=0.01, seed=0):
    v, t = S.uv_sphere()
    r = 1.0 + sigma * np.random.default_rng(seed).standard_normal(len(v))
    return (v.astype(np.float64) * r[:, None]).astype(np.float32), t


def jittered_holed_plane(seed=1):
    """in-plane jitter of a third of the grid step; z stays 0.25"""
    v, t = holed_plane()
    v = v.copy()
    v[:, :2] += (np.random.default_rng(seed).uniform(-1, 1, (len(v), 2)) / 32 / 3).astype(np.float32)
    return v, t


def wavy_grid(n=300):
    return S.grid_mesh(n, lambda x, y: 0.05 * np.sin(20 * x) * np.cos(14 * y) + 0.02 * np.sin(90 * x * y))
