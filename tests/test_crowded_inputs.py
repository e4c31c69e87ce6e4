"""The inputs of test_gpu_table_regrow.py have the properties that test relies on: checked here on the CPU with the oracle
alone (never with the library under test).  Bucket arithmetic: see crowded_inputs.py."""
import numpy as np
import pytest

import crowded_inputs as C
from oracle import oracle as O

LOW = np.uint64(63)


def _levels(keys):
    return np.array([(int(k).bit_length() - 1) // 3 for k in keys])


def _map_capacity(v):
    """capacity of a voxel key map for v keys, before any growth (nb_key_maps: next_pow2(max(1024, 2 v)))"""
    c = 1024
    while c < 2 * v:
        c *= 2
    return c


def regrows_needed(crowded, capacity):
    """times a table of `capacity` slots is rebuilt four times the size until capacity / 64 >= crowded"""
    n = 0
    while capacity // 64 < crowded:
        capacity *= 4
        n += 1
    return n


@pytest.mark.parametrize("V,regrows", [(17, 1), (512, 3), (5000, 3)])
def test_pitch4_keys_share_their_low_bits(V, regrows):
    keys = C.pitch4_keys(V)
    assert keys.dtype == np.uint64 and len(keys) == V and np.all(keys[1:] > keys[:-1])
    assert set(_levels(keys)) == {8}
    coords = np.array([O.key_coord(k)[:3] for k in keys])
    assert np.all(coords % 4 == coords[0] % 4)
    assert len(np.unique(keys & LOW)) == 1
    # the capacity rule the GPU test asserts: the last permitted size (<< 6) holds the keys, and it takes `regrows` steps
    assert regrows_needed(V, _map_capacity(V)) == regrows <= 3
    # no two cells adjacent: every row of the 55-slot list holds the voxel itself only
    idx, kidx, rs = O.Oracle().leaf_neighbors(keys)
    assert np.array_equal(rs, np.arange(V + 1)) and np.array_equal(idx, np.arange(V))


def test_pitch4_mixed_keys():
    keys, crowded = C.pitch4_mixed_keys()
    assert len(keys) == 4096 and np.all(keys[1:] > keys[:-1]) and set(_levels(keys)) == {8}
    low = keys & LOW
    assert crowded == 2048 + 32 == np.bincount(low.astype(np.int64)).max()
    assert crowded * 2 >= len(keys)  # the crowded share is at least half
    assert regrows_needed(crowded, _map_capacity(len(keys))) == 3
    idx, kidx, rs = O.Oracle().leaf_neighbors(keys)
    n = np.diff(rs)
    assert (n == 1).sum() == 2048 and n.max() == 7  # isolated sites; the block's interior cells have their 6 face neighbours


@pytest.mark.parametrize("m,per_site,level,anchors", [(8, 9, 5, False), (8, 9, 5, True), (8, 3, 5, False)])
def test_lattice_sites(m, per_site, level, anchors):
    pts, nrm, rad, bb = C.lattice_sites(m, per_site, level, anchors=anchors)
    n_sites = m ** 3
    assert len(pts) == n_sites * per_site + (2 if anchors else 0) and pts.dtype == np.float32
    # anchors: the frame KDTree derives from the points alone; otherwise the builder's box
    box = C.margin_box(pts) if anchors else bb
    o = O.Oracle()
    o.build_octree(pts, rad, *box)
    vs, _, off = o.frame()
    assert abs(vs[0] - 1.0) < 1e-6 and np.all(np.abs(off) <= 1)
    keys = o.point_keys(pts, rad, 1.0, 21)
    assert set(_levels(keys)) == {level}  # the radii put every point on that level
    site = np.ones(len(pts), bool)
    if anchors:
        site = (pts.min(1) > 2e-3) & (pts.max(1) < 1 - 2e-3)
        assert site.sum() == n_sites * per_site
    cells = np.unique(keys[site])
    assert len(cells) == n_sites and len(np.unique(cells & LOW)) == 1  # one cell per site, one residue
    per_level = [np.unique(o.point_keys(pts, rad, 1.0, L)) for L in range(level + 1)]
    total = sum(len(k) for k in per_level)
    assert [len(k) for k in per_level][:4] == [1, 8, 64, 512] and total <= 1609 + 2 * (level + 1)
    if 8 ** (level - 1) < len(pts) <= 8 ** level:
        # the kNN search hashes all cells of the levels 0..lfine, 8^lfine >= n, here lfine = level: 4096 slots = 64 buckets
        # against 512 keys of one residue, then 256 buckets, then 1024
        cap = 1024
        while cap < 2 * total:
            cap *= 2
        assert cap == 4096 and regrows_needed(n_sites, cap) == 2
    else:
        assert per_site < 9
    if anchors:
        return
    # octree: the site's cell and its 7 siblings on `level`, the 7 siblings of their parent on level - 1; every site is
    # alone in its cell of level - 2, and with m = 2^(level - 2) those cells fill the cube: no outer shell
    lv = _levels(o.leaves)
    anc = np.array([int(k) >> 6 for k in cells], np.uint64)  # the site cells' ancestors on level - 2
    assert len(np.unique(anc)) == n_sites
    leaf_anc = np.array([int(k) >> (3 * (l - (level - 2))) if l >= level - 2 else 0 for k, l in zip(o.leaves, lv)],
                        np.uint64)
    under = np.isin(leaf_anc, anc)
    shell = int((~under).sum())
    assert np.array_equal(np.bincount(np.searchsorted(anc, leaf_anc[under])), np.full(n_sites, 15))
    assert len(o.leaves) == 15 * n_sites + shell and shell == (0 if m == 1 << (level - 2) else shell)
    assert (lv == level).sum() == 8 * n_sites and (lv[under] == level - 1).sum() == 7 * n_sites
    # the whole path: at least as many aggregation pairs as level-0 voxels (the reference indexes the pair
    # importances with voxel indices)
    g0 = o.create_grids(5)[0]
    idx, dist, rs, compat = o.radius_search(pts, rad, g0["voxel_centers"], g0["voxel_sizes"])
    assert len(idx) >= len(g0["voxel_keys"])


def test_sparse_deep_overfills_the_octree_table():
    pts, nrm, rad, bb = C.sparse_deep(3000, 14)
    o = O.Oracle()
    o.build_octree(pts, rad, *bb)
    assert set(_levels(o.point_keys(pts, rad))) == {14}
    assert len(o.nodes) > 32768  # the first table has 65536 slots and may be half full
    assert len(o.nodes) * 2 <= 65536 << 12  # ... and the last permitted size holds them


def test_deep_clump_is_deeper_than_the_early_sort():
    pts, nrm, rad, bb = C.deep_clump()
    assert len(pts) == 2500
    o = O.Oracle()
    o.build_octree(pts, rad, *bb)
    assert _levels(o.leaves).max() >= 14  # PRESORT_LEVEL is 13
    g0 = o.create_grids(5)[0]
    idx, dist, rs, compat = o.radius_search(pts, rad, g0["voxel_centers"], g0["voxel_sizes"])
    assert len(idx) >= len(g0["voxel_keys"])
