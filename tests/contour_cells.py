"""Hand-made dual cells for the contouring (k_contour_* of csrc/asr_mesh.hip) and a plain numpy restatement of what
can be said about their mesh without ordering anything.  Numpy only; shares no code with the oracle or the kernel.

A face-balanced octree never puts more than 8 cells round an edge, never repeats more than three corners of a cell and
never holds a zero, so its fields leave most of the contouring's guards untouched.  The generators here build the cells
directly.  Each returns (values f32[V,2], duals i64[D,8], positions f32[V,3]).

The restatement gives, per input: the active flag of every cell, every active cell's vertex (f64 mean of the crossing
points, rounded once), the number n of active cells round every owned crossing edge, and from those the vertex and
triangle counts.  The corner order of the triangles stays the oracle's business."""
import numpy as np

CUBE_EDGES = ((0, 1), (1, 3), (3, 2), (2, 0), (4, 5), (5, 7), (7, 6), (6, 4), (0, 4), (1, 5), (3, 7), (2, 6))
CUBE_FACES = ((0, 1, 3, 2), (4, 6, 7, 5), (1, 5, 7, 3), (2, 3, 7, 6), (0, 2, 6, 4), (0, 4, 5, 1))
OWNED_EDGES = ((0, 1), (1, 3), (1, 5))
CAP = 29  # cells round one edge that the kernel orders (csrc/asr_uset.h)

# the half turn about the cube's x axis, corner k -> k ^ 6: keeps the sense of every face cycle of CUBE_FACES and
# takes the owned edge (0, 1) to (6, 7), which no cell owns
HALF_TURN = tuple(k ^ 6 for k in range(8))


# ---- generators ----------------------------------------------------------------------------------------------------
def ring(n, missing=(), pad=0, seed=0, owner=None):
    """n wedge cells round the edge (a, b) = voxels (0, 1); voxel 2 + i is spoke i.  Wedge i is
    [a, b, s_i, s_i, s_j, s_j, s_i, s_i] with j = (i + 1) % n: its face 0 is {a, b, s_i}, its face 5 {a, b, s_j}, so
    neighbouring wedges share a face.  `missing` drops wedges (one gap: an open fan, two gaps: two arcs).  `pad`
    unrelated active cubes (8 fresh voxels each, corner 0 negative) come first in the cell list and shift every vertex
    id.  With `owner` = i every wedge but i is turned by HALF_TURN, which puts (a, b) on an edge it does not own: the
    edge is emitted once, not once per wedge."""
    rng = np.random.default_rng([seed, n, pad])
    nvox = 2 + n + 8 * pad
    values = np.empty((nvox, 2), np.float32)
    values[:, 0] = rng.uniform(0.25, 1.0, nvox)
    values[0, 0] = -rng.uniform(0.25, 1.0)
    values[:, 1] = 0.5
    positions = rng.uniform(-1, 1, (nvox, 3)).astype(np.float32)
    cells = []
    for p in range(pad):
        base = 2 + n + 8 * p
        values[base, 0] = -values[base, 0]
        cells.append(list(range(base, base + 8)))
    for i in range(n):
        if i in missing:
            continue
        s, t = 2 + i, 2 + (i + 1) % n
        w = [0, 1, s, s, t, t, s, s]
        if owner is not None and i != owner:
            w = [w[HALF_TURN[k]] for k in range(8)]
        cells.append(w)
    return values, np.array(cells, np.int64).reshape(-1, 8), positions


def ring_wedges(n, missing=(), pad=0):
    """vertex id -> wedge number for the cells of ring(n, missing, pad) (the pad cubes map to -1)"""
    return np.array([-1] * pad + [i for i in range(n) if i not in missing])


def merged_lattice(m, frac, seed=0):
    """the (m-1)^3 unit cubes of an m^3 voxel lattice, corner k at (x + (k & 1), y + (k >> 1 & 1), z + (k >> 2 & 1)),
    after a random share `frac` of the voxels was merged into a +x, +y or +z neighbour (chains resolved to their root,
    the map applied to every cell): coarse cells next to fine ones, without the balance of a real tree.  Cells with
    3..8 distinct corners, degenerate faces, n from 1 to about 10 and, at larger frac, edges that cannot be sorted."""
    rng = np.random.default_rng([seed, m, int(round(frac * 1000))])
    nvox = m ** 3
    vid = lambda x, y, z: (z * m + y) * m + x
    target = np.arange(nvox)
    for v in np.flatnonzero(rng.random(nvox) < frac):
        x, y, z = v % m, v // m % m, v // (m * m)
        step = [(1, 0, 0), (0, 1, 0), (0, 0, 1)][int(rng.integers(3))]
        w = (x + step[0], y + step[1], z + step[2])
        if max(w) < m:
            target[v] = vid(*w)  # always a larger id: no cycles
    for v in range(nvox - 1, -1, -1):
        target[v] = target[target[v]]
    cells = [[vid(x + (k & 1), y + (k >> 1 & 1), z + (k >> 2 & 1)) for k in range(8)]
             for z in range(m - 1) for y in range(m - 1) for x in range(m - 1)]
    duals = target[np.array(cells, np.int64).reshape(-1, 8)]
    values = np.stack([rng.standard_normal(nvox), rng.uniform(0, 2, nvox)], 1).astype(np.float32)
    site = np.stack([np.arange(nvox) % m, np.arange(nvox) // m % m, np.arange(nvox) // (m * m)], 1)
    positions = (site + rng.uniform(-0.2, 0.2, (nvox, 3))).astype(np.float32)
    return values, duals, positions


SIGNED_SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 3.4e38, -3.4e38,
                            np.finfo(np.float32).tiny], np.float32)


def with_special_values(values, seed=0, thr=1.0):
    """a copy with a quarter of the signed values drawn from SIGNED_SPECIALS and a sixth of the unsigned ones from
    {thr, nextafter(thr, 2), 0, NaN, inf}.  Positions are not touched: a NaN or infinite vertex has a sign and payload
    that may differ between two correct machines, and the comparison is on bits."""
    rng = np.random.default_rng([seed, len(values)])
    out = np.array(values, np.float32, copy=True)
    thr = np.float32(thr)
    unsigned = np.array([thr, np.nextafter(thr, np.float32(2)), 0.0, np.nan, np.inf], np.float32)
    pick = rng.random(len(out)) < 0.25
    out[pick, 0] = SIGNED_SPECIALS[rng.integers(len(SIGNED_SPECIALS), size=int(pick.sum()))]
    pick = rng.random(len(out)) < 1 / 6
    out[pick, 1] = unsigned[rng.integers(len(unsigned), size=int(pick.sum()))]
    return out


# ---- the restatement -----------------------------------------------------------------------------------------------
def _crossing(values, thr, a, b):
    """contouring.cpp:81-111 on index arrays: not both unsigned values above the threshold, and signed values of
    strictly opposite sign (a zero of either sign, or a NaN, crosses nothing).  Compared in f32, as stored."""
    with np.errstate(invalid="ignore"):
        gate = ~((values[a, 1] > thr) & (values[b, 1] > thr))
        va, vb = values[a, 0], values[b, 0]
        return gate & (((va < 0) & (vb > 0)) | ((va > 0) & (vb < 0)))


class Restatement:
    """.active bool[D]; .vertices f32[#active,3]; .edges: list of (vertex id, owned edge 0..2, a, b, n, cells) with
    cells the ascending vertex ids of the active cells that hold both a and b; .num_vertices, .num_triangles"""

    def __init__(self, values, duals, positions, thr=1.0):
        values = np.asarray(values, np.float32)
        duals = np.asarray(duals, np.int64).reshape(-1, 8)
        pos = np.asarray(positions, np.float32).astype(np.float64)
        thr = np.float32(thr)
        cross = np.zeros((len(duals), 12), bool)
        for e, (i, j) in enumerate(CUBE_EDGES):
            cross[:, e] = _crossing(values, thr, duals[:, i], duals[:, j])
        self.active = cross.any(1)
        act = np.flatnonzero(self.active)
        cells = duals[act]
        total = np.zeros((len(act), 3))
        count = np.zeros(len(act))
        with np.errstate(all="ignore"):
            for e, (i, j) in enumerate(CUBE_EDGES):  # the sum runs in edge order
                a, b = cells[:, i], cells[:, j]
                v1, v2 = values[a, 0].astype(np.float64), values[b, 0].astype(np.float64)
                t = -v1 / (v2 - v1)
                t = np.where(np.isfinite(t) & (t >= 0) & (t <= 1), t, 0.5)
                p = (1 - t)[:, None] * pos[a] + t[:, None] * pos[b]
                on = cross[act, e]
                total[on] = total[on] + p[on]
                count[on] += 1
            self.vertices = (total / count[:, None]).astype(np.float32)
        holders = {}
        for vid, c in enumerate(cells):
            for v in set(c.tolist()):
                holders.setdefault(v, set()).add(vid)
        self.edges = []
        for vid, c in enumerate(cells):
            for e, (i, j) in enumerate(OWNED_EDGES):
                a, b = int(c[i]), int(c[j])
                if a != b and bool(_crossing(values, thr, np.array([a]), np.array([b]))[0]):
                    around = sorted(holders[a] & holders[b])
                    self.edges.append((vid, e, a, b, len(around), around))
        self.cells = cells
        self.values = values
        ns = np.array([e[4] for e in self.edges], np.int64)
        self.n_histogram = {int(k): int(c) for k, c in zip(*np.unique(ns, return_counts=True))}
        self.num_vertices = len(act) + int((ns > 4).sum())
        self.num_triangles = int((ns == 3).sum() + 2 * (ns == 4).sum() + ns[ns > 4].sum())

    def min_reversals(self, edge):
        """the walk of contouring.cpp:247-299 round `edge` (an entry of .edges) from every possible first cell: the
        smallest number of reversals over the starts, and whether every start orders all cells.  Which cell the
        reference starts from is libstdc++'s business; what holds for every start holds for that one."""
        _, _, a, b, n, around = edge
        if self.values[a, 0] > self.values[b, 0]:
            a, b = b, a
        fewest, sorts = None, True
        for start in around:
            order, rest, e0, e1, rev = [start], [c for c in around if c != start], a, b, 0
            for _ in range(n * n):
                if not rest:
                    break
                face = _face_with_oriented_edge(self.cells[order[-1]], e0, e1)
                nxt = next((c for c in rest if face in _faces(self.cells[c])), None)
                if nxt is None:
                    order.reverse()
                    e0, e1 = e1, e0
                    rev += 1
                else:
                    order.append(nxt)
                    rest.remove(nxt)
            sorts &= not rest
            fewest = rev if fewest is None else min(fewest, rev)
        return fewest, sorts


def _faces(cell):
    return [frozenset(int(cell[k]) for k in f) for f in CUBE_FACES]


def _face_with_oriented_edge(cell, e0, e1):
    for f in CUBE_FACES:
        for j in range(4):
            if cell[f[j]] == e0 and cell[f[(j + 1) % 4]] == e1:
                face = frozenset(int(cell[k]) for k in f)
                if len(face) >= 3:
                    return face
    return frozenset()


def deciding_classes(values, duals, thr=1.0):
    """which kinds of odd signed value sit on a cube edge that the threshold lets through and whose other end is an
    ordinary non-zero number, so that the odd value alone decides the crossing -> {kind: number of cells}"""
    values = np.asarray(values, np.float32)
    thr = np.float32(thr)
    s = values[:, 0]
    tiny = np.finfo(np.float32).tiny
    with np.errstate(invalid="ignore"):
        kinds = {"zero": (s == 0) & ~np.signbit(s), "negative zero": (s == 0) & np.signbit(s), "nan": np.isnan(s),
                 "infinity": np.isinf(s), "denormal": (s != 0) & (np.abs(s) < tiny)}
        ordinary = np.isfinite(s) & (np.abs(s) >= tiny)
        found = {}
        for name, odd in kinds.items():
            hit = np.zeros(len(duals), bool)
            for i, j in CUBE_EDGES:
                a, b = duals[:, i], duals[:, j]
                open_ = ~((values[a, 1] > thr) & (values[b, 1] > thr))
                hit |= open_ & ((odd[a] & ordinary[b]) | (odd[b] & ordinary[a]))
            found[name] = int(hit.sum())
    return found


# ---- the cases both test files run -----------------------------------------------------------------------------------
RING_N = (1, 2, 3, 4, 5, 8, 9, 13, 14, 15, 28, 29)
RING_PADS = (0, 5, 1000)
OPEN_RINGS = ((6, 0), (6, 3), (12, 11), (20, 7), (29, 13))  # (n, the missing wedge)
ONCE_RINGS = ((5, 0), (8, 3), (14, 13), (29, 7))  # (n, the one wedge that owns the edge)
TWO_GAPS = (8, (1, 5))
# (m, frac, seed); m = 2 is a single cell
LATTICES = ((2, 0.0, 0), (2, 0.0, 1), (3, 0.0, 0), (7, 0.0, 0), (3, 0.3, 1), (3, 0.3, 2), (7, 0.05, 0), (7, 0.05, 1),
            (7, 0.05, 2), (7, 0.05, 3), (7, 0.1, 0), (7, 0.1, 1), (7, 0.1, 2), (7, 0.1, 3), (7, 0.15, 0), (7, 0.15, 1),
            (7, 0.15, 2), (7, 0.15, 3), (7, 0.3, 0), (7, 0.3, 1))
THRESHOLDS = (1.0, 0.0, -1.0, float("inf"), float("nan"))


def special_cases():
    """(name, values, duals, positions, thr): the odd values on a plain lattice, a merged one and a ring of 6, at every
    threshold"""
    out = []
    for thr in THRESHOLDS:
        for name, (v, d, p) in (("lattice", merged_lattice(7, 0.0, 5)), ("merged", merged_lattice(7, 0.05, 0)),
                                ("ring6", ring(6, pad=3))):
            for seed in (0, 1):
                out.append(("%s-thr%s-s%d" % (name, thr, seed), with_special_values(v, seed, thr), d, p, thr))
    return out


def plane_field(n=5000, seed=0, noise=0.0):
    """a plane through a mixed-density scan cloud on the oracle's own octree: the field [(c - mean) . nrm, |.| / voxel
    size] -- unlike the sphere of parity.sphere_field the surface runs through the coarse rim cells, which gives
    n = 1, 3, 5 in numbers"""
    from asr_hip import synth
    from oracle import oracle as O
    p, _ = synth.scan_cloud(n, seed=seed, device="cpu", density_variance=10.0)
    pts = p.numpy()
    rad = synth.knn_radii(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    o = O.Oracle()
    o.build_octree(pts, rad, *bb)
    g = o.create_grids(1)[0]
    du = o.create_dual_vertex_indices().astype(np.int64)
    c, vs = g["voxel_centers"], g["voxel_sizes"]
    nrm = np.array([0.3, 0.5, 0.81], np.float64)
    nrm /= np.linalg.norm(nrm)
    sd = ((c - pts.mean(0)) @ nrm).astype(np.float32)
    if noise:
        sd = sd + np.random.default_rng(seed + 11).normal(0, noise, sd.shape).astype(np.float32) * vs
    values = np.stack([sd, np.abs(sd) / vs], 1).astype(np.float32)
    return values, du, c
