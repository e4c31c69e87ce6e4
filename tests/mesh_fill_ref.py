"""numpy restatement of the contract of asr_hip_mesh_fill_holes_count / _fill (include/asr_hip.h): centroid
fans over the simple boundary rims of at most max_edges edges.  Needs no GPU.  Also the meshes of the hole-filling tests
that tests/mesh_adjacency_ref.py does not already have."""
import numpy as np

import mesh_adjacency_ref as A
import mesh_simplify_ref as S

FILL_CUT = 128          # rims longer than this are summed in the library's wave shape
MAX_EDGES_LIMIT = 1 << 20
REPORT_FIELDS = ("rims", "filled", "too_long", "not_simple", "new_vertices", "new_triangles")


def directed_boundary(triangles, num_vertices):
    """-> (tail, head) int64 [B]: the boundary edges as their one triangle runs through them, in edge-table order"""
    edges, uses, forward = A.edge_table(triangles, num_vertices)
    b = uses == 1
    lo, hi, fw = edges[b, 0].astype(np.int64), edges[b, 1].astype(np.int64), forward[b] == 1
    return np.where(fw, lo, hi), np.where(fw, hi, lo)


def rim_ids(tail, head, num_vertices):
    """int64 [V]: the smallest vertex of the rim every vertex lies on, -1 off the boundary"""
    label = np.arange(num_vertices)
    while len(tail):  # min-label propagation over the boundary edges alone
        m = np.minimum(label[tail], label[head])
        new = label.copy()
        np.minimum.at(new, tail, m)
        np.minimum.at(new, head, m)
        if np.array_equal(new, label):
            break
        label = new
    on = np.zeros(num_vertices, bool)
    on[tail] = True
    on[head] = True
    return np.where(on, label, -1)


def hub_position(points):
    """the mean of f32 points [n,3], given in ascending vertex index, in the library's summation shape -> f32 [3]"""
    p = np.asarray(points, np.float32).astype(np.float64)
    n = len(p)
    if n <= FILL_CUT:
        s = np.zeros(3)
        for row in p:
            s = s + row
    else:
        part = np.zeros((64, 3))
        for k in range(n):  # lane k % 64 takes the entries k % 64, k % 64 + 64, ... in order
            part[k % 64] = part[k % 64] + p[k]
        lane = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            part = part + part[lane ^ m]
        s = part[0]
    return (s / np.float64(n)).astype(np.float32)


def fill_holes(vertices, triangles, max_edges):
    """-> (vertices f32 [V + hubs,3], triangles int32 [T + new,3], report dict).  ValueError: max_edges outside 3..2^20, a
    corner out of range ("out of range"), a vertex of a filled rim that is not finite ("not finite")."""
    if isinstance(max_edges, bool) or int(max_edges) != max_edges or not 3 <= int(max_edges) <= MAX_EDGES_LIMIT:
        raise ValueError("max_edges must be an integer in 3..2^20")
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    nv = len(v)
    tri = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    report = dict.fromkeys(REPORT_FIELDS, 0)
    if len(tri) == 0:
        return v.copy(), tri.copy(), report
    A._tri(tri, nv)  # the range check
    tail, head = directed_boundary(tri, nv)
    rim_of = rim_ids(tail, head, nv)
    out_deg = np.bincount(tail, minlength=nv)
    in_deg = np.bincount(head, minlength=nv)
    hubs, new = [], []
    for rim in np.unique(rim_of[rim_of >= 0]):  # ascending rim id
        report["rims"] += 1
        members = np.flatnonzero(rim_of == rim)  # ascending vertex index
        n = int((rim_of[tail] == rim).sum())
        if not (np.all(out_deg[members] == 1) and np.all(in_deg[members] == 1)):
            report["not_simple"] += 1
            continue
        assert n == len(members) and n >= 3
        if n > max_edges:
            report["too_long"] += 1
            continue
        report["filled"] += 1
        if not np.isfinite(v[members]).all():
            raise ValueError("a vertex of a filled rim is not finite")
        succ = dict(zip(tail[rim_of[tail] == rim].tolist(), head[rim_of[tail] == rim].tolist()))
        if n == 3:
            m = int(rim)
            s = succ[m]
            p = succ[s]
            assert succ[p] == m
            new.append((m, p, s))
            continue
        hub = nv + len(hubs)
        hubs.append(hub_position(v[members]))
        new.extend((succ[int(a)], int(a), hub) for a in members)
    report["new_vertices"], report["new_triangles"] = len(hubs), len(new)
    v2 = np.concatenate([v, np.array(hubs, np.float32).reshape(-1, 3)])
    t2 = np.concatenate([tri, np.array(new, np.int32).reshape(-1, 3)])
    return v2, t2, report


# ---- the meshes of the tests -----------------------------------------------------------------------------------------
def open_tetrahedron():
    """a tetrahedron, outward, without the face opposite vertex 3: one rim of 3 edges"""
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    return v, np.int32([[0, 1, 3], [1, 2, 3], [2, 0, 3]])


def open_cube():
    """a cube, outward, without its top face: one rim of 4 edges"""
    v = np.float32([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)])
    quads = [(0, 2, 3, 1), (0, 1, 5, 4), (1, 3, 7, 5), (3, 2, 6, 7), (2, 0, 4, 6)]  # bottom and the four sides
    tri = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.int32(tri)


def open_cylinder(n=12, rings=4):
    """a tube of `rings` rings of n vertices, open at both ends: two rims of n edges"""
    th = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([np.stack([np.cos(th), np.sin(th), np.full(n, 0.5 * k)], 1) for k in range(rings)]).astype(np.float32)
    tri = []
    for k in range(rings - 1):
        for i in range(n):
            a, b = k * n + i, k * n + (i + 1) % n
            tri += [(a, b, b + n), (a, b + n, a + n)]
    return v, np.int32(tri)


def disk(n):
    """A.fan's closed fan of n spokes: a disc around vertex 0 whose rim has n vertices and n edges"""
    return A.fan(n, closed=True)


def disks_around_the_cut():
    """disks of 127, 128, 129 and 200 rim vertices side by side: the two sides of the summation cut"""
    vs, ts, base = [], [], 0
    for k, n in enumerate((FILL_CUT - 1, FILL_CUT, FILL_CUT + 1, 200)):
        v, t = A.fan(n, centre=(3.0 * k, 0.25 * k, 0.0), closed=True)
        vs.append(v)
        ts.append(t + base)
        base += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(ts).astype(np.int32)


def bow_tie():
    """a 5 x 5 grid of squares without the squares (1, 1) and (2, 2): two holes of 4 edges that share a vertex"""
    n = 6
    v = np.float32([[i, j, 0] for i in range(n) for j in range(n)])
    tri = []
    for i in range(n - 1):
        for j in range(n - 1):
            if (i, j) in ((1, 1), (2, 2)):
                continue
            a = i * n + j
            tri += [(a, a + n, a + n + 1), (a, a + n + 1, a + 1)]
    return v, np.int32(tri)


def flipped_rim_plane():
    """A.holed_plane() with one triangle on the hole's rim turned over: the hole's triangles disagree about its direction"""
    v, t = A.holed_plane()
    tail, head = directed_boundary(t, len(v))
    rim_of = rim_ids(tail, head, len(v))
    hole = np.unique(rim_of[rim_of >= 0])[1]  # the border holds vertex 0
    a, b = next((a, b) for a, b in zip(tail.tolist(), head.tolist()) if rim_of[a] == hole)
    which = next(i for i, c in enumerate(t.tolist()) if (a, b) in ((c[0], c[1]), (c[1], c[2]), (c[2], c[0])))
    t = t.copy()
    t[which] = t[which, [0, 2, 1]]
    return v, t


def renumbered_holes(seed=5):
    """the open cylinder and the open cube under a random renumbering of the vertices, with 9 unused vertices mixed in:
    ascending vertex index is not the order in which a rim is walked"""
    cv, ct = open_cylinder()
    bv, bt = open_cube()
    v = np.concatenate([cv, bv + np.float32([3, 0, 0]), np.full((9, 3), 7.5, np.float32)]).astype(np.float32)
    t = np.concatenate([ct, bt + len(cv)])
    perm = np.random.default_rng(seed).permutation(len(v))  # old -> new
    v2 = np.empty_like(v)
    v2[perm] = v
    return v2, perm[t].astype(np.int32)


def single_triangle():
    return np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int32([[2, 0, 1]])


FILL_MESHES = {
    "open tetrahedron": open_tetrahedron, "open cube": open_cube, "open cylinder": open_cylinder,
    "disks around the cut": disks_around_the_cut, "bow tie": bow_tie, "flipped rim": flipped_rim_plane,
    "renumbered holes": renumbered_holes, "single triangle": single_triangle,
}
