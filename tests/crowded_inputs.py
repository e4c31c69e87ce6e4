"""Inputs that crowd the buckets of the geometry half's hash tables, and inputs that make its tables regrow for other reasons.

Bucket arithmetic (csrc/asr_geom.hip, HashTab / TabProbe).  Every table is keyed on location codes with a leading bit
(1 << 3 * level | Morton code of the cell; the searches' cell tables too, k_cell_bounds inserts `prefix | marker`).  The
low 6 bits of such a code are the child indices of the two finest levels, i.e. (x & 3, y & 3, z & 3) of the cell's integer
coordinates on its level.  A table keeps those 6 bits as the slot inside a 64-slot bucket and hashes only the rest, so a
table of capacity C has C / 64 buckets and holds at most C / 64 keys with the same low 6 bits, however empty it is.  A key
set whose coordinates are all congruent mod 4 shares its low 6 bits: S such keys overflow every table with C / 64 < S.  The
hosts then rebuild the table four times the size (capacity << 2 per step, at most << 6).

All builders are deterministic.  The properties the GPU tests rely on are asserted on the CPU, with the oracle only, in
test_crowded_inputs.py."""
import numpy as np

from oracle import oracle as O

UNIT_BOX = (np.zeros(3, np.float32), np.ones(3, np.float32))


def level_keys(coords, level):
    """sorted uint64 location codes of integer cell coordinates [V,3] on `level`"""
    return np.sort(np.array([O.coord_key(int(x), int(y), int(z), level) for x, y, z in coords], np.uint64))


def _pitch4_coords(V, level, residue):
    side = (1 << level) // 4
    assert V <= side ** 3, "level too coarse for %d sites" % V
    m = 1
    while m ** 3 < V:
        m += 1
    m = min(m, side)
    # the first V sites of a z-fastest walk over a block of m x m x (whatever is needed) sites
    i = np.arange(V)
    s = np.stack([i // (m * m), (i // m) % m, i % m], 1)
    assert s.max() < side
    return 4 * s + residue


def pitch4_keys(V, level=8, residue=1):
    """V sorted keys of one level whose cell coordinates are all == residue (mod 4): one value of `key & 63`, no two
    cells adjacent.  A key map of capacity C holds them only when C / 64 >= V."""
    return level_keys(_pitch4_coords(V, level, residue), level)


def pitch4_mixed_keys(level=8, residue=1):
    """2048 pitch-4 keys (16 x 16 x 8 sites in the low corner of the level) plus a fully adjacent 16 x 16 x 8 block of
    cells far from them (2048 keys, every row with face neighbours; 4 x 4 x 2 = 32 of its cells have the
    crowded residue).  -> (sorted keys [4096], number of keys with the crowded low 6 bits = 2080).  The map's capacity is
    8192 (128 buckets), << 4 gives 2048 buckets < 2080: only the last permitted size, << 6, holds them."""
    i = np.arange(2048)
    sites = 4 * np.stack([i // 128, (i // 8) % 16, i % 8], 1) + residue
    half = 1 << (level - 1)
    block = np.stack([i // 128, (i // 8) % 16, i % 8], 1) + half
    assert sites.max() < half and block.max() < (1 << level)
    keys = level_keys(np.concatenate([sites, block]), level)
    crowded = int(((keys & np.uint64(63)) == (keys[0] & np.uint64(63))).sum())
    return keys, crowded


def radius_for_level(level, edge=1.0):
    """a point radius that puts a point on `level` of a frame with root edge `edge` (radius scale 1): the key's level is
    the last one whose voxel size is >= the radius"""
    return np.float32(0.75 * edge / (1 << level))


def lattice_sites(m, per_site, level, seed=0, residue=1, anchors=False):
    """m^3 sites at a pitch of four level-`level` cells of the unit box's frame: site (i, j, k) is the cell
    (4 i + residue, ...), its `per_site` points are jittered inside the central half of that cell (so a frame that differs
    from the unit box's by rounding keeps every point in its cell), radii put every point on `level`.
    -> (points [n,3], normals [n,3], radii [n], (bb_min, bb_max)), points in a shuffled order.

    Every site cell has the same low 6 bits on `level`; on level - 1 the sites fall into 8 classes, on level - 2 and
    coarser they spread.  m = 8, level = 5: 512 + 512 + 512 + 64 + 8 + 1 = 1609 occupied cells on the levels 0..5, a cell
    table of 4096 slots = 64 buckets against 512 keys with one residue.

    anchors: two more points close to the box's corners (1e-3 inside), for callers that derive the frame from the points'
    own bounding box plus a margin of 1e-3 (KDTree): with them that frame is the unit box's up to rounding."""
    assert 4 * (m - 1) + residue < (1 << level)
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)
    cell = np.repeat(4 * g + residue, per_site, axis=0).astype(np.float64)
    pts = (cell + 0.25 + 0.5 * rng.random(cell.shape)) / (1 << level)
    if anchors:
        pts = np.concatenate([pts, [[1e-3] * 3, [1 - 1e-3] * 3]])
    pts = pts[rng.permutation(len(pts))].astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (len(pts), 1))
    rad = np.full(len(pts), radius_for_level(level), np.float32)
    return pts, nrm, rad, UNIT_BOX


def margin_box(points):
    """the bounding box KDTree puts its frame around (adaptivesurfacereconstruction._margin_frame), restated"""
    lo, hi = points.min(0), points.max(0)
    m = max(1e-3, 1e-3 * float((hi - lo).max()))
    return lo - np.float32(m), hi + np.float32(m)


def sparse_deep(n, level, seed=0):
    """n isolated uniform points of the unit box whose radii put them on `level`: every point brings its own chain of
    ancestors with their siblings, 8 nodes per level below the depth at which the chains part, and the 2:1 balance fills
    the space between them.  n = 3000, level = 14: about 2 * 10^6 nodes against the octree table's 65536 slots, which may
    be half full at most."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.02, 0.98, size=(n, 3)).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (n, 1))
    rad = np.full(n, radius_for_level(level), np.float32)
    return pts, nrm, rad, UNIT_BOX


def deep_clump(n_scan=2000, n_clump=500, shrink=1e-3, seed=41):
    """a scan cloud plus a clump: the first `n_clump` points of the scan again, shrunk by `shrink` about their centroid and
    moved onto a point of the scan, radii shrunk alike.  The clump's leaves are ~10 levels finer than the scan's (>= 14):
    the early point sort of the overlapped build goes deeper than its least depth."""
    from asr_hip import synth
    p, q = synth.scan_cloud(n_scan, seed=seed, device="cpu")
    pts, nrm = p.numpy(), q.numpy()
    rad = synth.knn_radii(pts, 24)
    s = np.float32(shrink)
    c = pts[:n_clump]
    c = ((c - c.mean(0, dtype=np.float32)) * s + pts[n_clump]).astype(np.float32)
    pts = np.concatenate([pts, c]).astype(np.float32)
    nrm = np.concatenate([nrm, nrm[:n_clump]]).astype(np.float32)
    rad = np.concatenate([rad, rad[:n_clump] * s]).astype(np.float32)
    return pts, nrm, rad, synth.bounding_box(pts, 0.1)
