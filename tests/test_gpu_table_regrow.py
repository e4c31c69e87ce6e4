"""GPU tests of the host-side retry loops around the geometry half's hash tables (csrc/asr_geom.hip, HashTab / TabProbe):
inputs that overflow a table although it is far from full (crowded_inputs.py: keys that share their low 6 bits) or that
overfill it, so that the table is rebuilt four times the size and the work run again.  A retry that goes wrong does not
crash -- a key map that lost keys gives lists with entries missing -- so every case compares the results with the oracle
or with brute force, bit for bit where the operation is exact, and reads the context's cumulative "table_regrows"
diagnostic before and after to show that a loop was entered.  The inputs' properties are asserted in test_crowded_inputs.py.

Also here: the host-chosen paths of the whole build (options overlap / early_sort / early_cells), which decide where the
aggregation search gets its point order and its cell table from."""
import numpy as np
import pytest
import torch

import crowded_inputs as C
import parity
from asr_hip import _lib, ops, synth
from asr_hip.pipeline import ImplicitPipeline
from oracle import oracle as O
from test_gpu_attributes import MIN_WEIGHT, _check_against_reference
from test_gpu_nearest import check_nearest
from test_attributes import transfer_reference

pytestmark = pytest.mark.gpu

_close = parity.assert_close  # the tolerance of test_gpu_network.py


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _t(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _regrows(ctx):
    return ctx.get_option("table_regrows")


fresh_ops_context = ops.fresh_context  # the operators (and KDTree, which uses them) with nothing grown by an earlier call


def _scan(n, seed, density_variance=1.0):
    p, q = synth.scan_cloud(n, seed=seed, device="cpu", density_variance=density_variance)
    pts, nrm = p.numpy(), q.numpy()
    return pts, nrm, synth.knn_radii(pts, 24), synth.bounding_box(pts, 0.1)


# ---- case 1: the voxel key maps alone ---------------------------------------------------------------------------------
def _key_sets():
    return {"17": (lambda: C.pitch4_keys(17), 1), "512": (lambda: C.pitch4_keys(512), 3),
            "5000": (lambda: C.pitch4_keys(5000), 3), "mixed": (lambda: C.pitch4_mixed_keys()[0], 3)}


@pytest.mark.parametrize("which", ["17", "512", "5000", "mixed"])
def test_key_map_regrows_and_keeps_every_key(gpu, which):
    """55-slot lists of key sets with one residue mod 4.  The map of V keys has next_pow2(max(1024, 2 V)) slots = that / 64
    buckets, and holds S keys of one residue only with >= S buckets: 17 keys -> 16 buckets, then 64: one regrow; 512 and
    5000 keys -> fewer buckets than keys at << 0, 2, 4: three regrows, the last permitted size holds them; the mixed set
    (2080 crowded keys of 4096) -> 128, 512, 2048 buckets fail, 8192 hold: three.  The fill call starts at the size the
    count call ended with, so the counts are those of one map."""
    make, want = _key_sets()[which]
    keys = make()
    tk = _t(keys.view(np.int64), gpu)
    ctx = ops.context(gpu)
    before = _regrows(ctx)
    idx, kidx, rs = ops.grid_neighbors(tk)
    got = _regrows(ctx) - before
    print("key set %s: %d keys, %d regrows" % (which, len(keys), got))
    o_idx, o_kidx, o_rs = O.Oracle().leaf_neighbors(keys)
    assert np.array_equal(rs.cpu().numpy(), o_rs)
    assert np.array_equal(idx.cpu().numpy(), o_idx)
    assert np.array_equal(kidx.cpu().numpy(), o_kidx)
    assert got == want


def test_key_map_regrows_for_a_row_subset(gpu):
    """the row-subset operator on the mixed set: the listed rows of the full lists, the other rows empty"""
    keys = C.pitch4_mixed_keys()[0]
    v = len(keys)
    o_idx, o_kidx, o_rs = O.Oracle().leaf_neighbors(keys)
    rows = np.sort(np.random.default_rng(5).choice(v, size=v // 3, replace=False))
    ctx = ops.context(gpu)
    before = _regrows(ctx)
    idx, kidx, rs = ops.grid_neighbors_rows(_t(keys.view(np.int64), gpu), _t(rows.astype(np.int32), gpu))
    got = _regrows(ctx) - before
    print("row subset of the mixed set: %d regrows" % got)
    lens = np.zeros(v, np.int64)
    lens[rows] = np.diff(o_rs)[rows]
    assert np.array_equal(rs.cpu().numpy(), np.concatenate([[0], np.cumsum(lens)]))
    assert np.array_equal(idx.cpu().numpy(), np.concatenate([o_idx[o_rs[q]:o_rs[q + 1]] for q in rows]))
    assert np.array_equal(kidx.cpu().numpy(), np.concatenate([o_kidx[o_rs[q]:o_rs[q + 1]] for q in rows]))
    assert got == 3


# ---- case 2: the octree's table ---------------------------------------------------------------------------------------
def test_octree_table_regrows(gpu):
    """3000 isolated points on level 14: ~2 * 10^6 nodes against a first table of 65536 slots that may be half full (the
    list-full retry), without and with one growth step of the keys; an ordinary scan on the same context afterwards"""
    pts, nrm, rad, bb = C.sparse_deep(3000, 14)
    frame = _lib.frame_init(*bb)
    tp, tr = _t(pts, gpu), _t(rad, gpu)
    ctx = ops.context(gpu)
    for grow_steps in (0, 1):
        o = O.Oracle()
        o.build_octree(pts, rad, *bb, grow_steps=grow_steps)
        before = _regrows(ctx)
        nodes, leaves = ops.octree_build(frame, tp, tr, 1.0, 21, grow_steps)
        got = _regrows(ctx) - before
        print("sparse octree, grow_steps %d: %d nodes, %d regrows" % (grow_steps, len(o.nodes), got))
        assert np.array_equal(_u64(nodes), o.nodes)
        assert np.array_equal(_u64(leaves), o.leaves)
        assert got >= 1
    pts, nrm, rad, bb = _scan(6000, 5)
    o = O.Oracle()
    o.build_octree(pts, rad, *bb)
    nodes, leaves = ops.octree_build(_lib.frame_init(*bb), _t(pts, gpu), _t(rad, gpu))
    assert np.array_equal(_u64(nodes), o.nodes) and np.array_equal(_u64(leaves), o.leaves)


# ---- case 3: the pre-filter queries -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice9():
    """lattice_sites(8, 9, 5) with the two corner points that make KDTree's own frame the unit box's, and its brute-force
    references (computed once, never changed)"""
    pts, nrm, rad, bb = C.lattice_sites(8, 9, 5, anchors=True)
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2)
    d2 = (d2[..., 0] + d2[..., 1]) + d2[..., 2]
    order = np.argsort(d2, axis=1, kind="stable")[:, :24]  # stable: equal distances keep index order
    ref = {k: O.knn_radius(pts, k) for k in (1, 24, 40)}
    for a in (order, *ref.values()):
        a.setflags(write=False)
    return dict(pts=pts, nrm=nrm, rad=rad, bb=bb, order=order, knn=ref)


@pytest.mark.parametrize("knn_cells", [1, 0], ids=["cell-path", "wave-path"])
def test_prefilter_queries_on_a_crowded_lattice(gpu, lattice9, knn_cells):
    """KDTree.compute_k_radius (here; compute_inlier and compute_radius_neighbors in the two tests below) on 8^3 sites at a
    pitch of four level-5 cells, nine points each: the kNN search hashes the levels 0..5, 1611 cells in 4096 slots = 64
    buckets, and 512 of the keys share their low 6 bits -- 64 buckets fail, 256 fail, 1024 hold: two regrows on a fresh
    context.  Before these calls had a retry loop (the parent of this change) the first of them returned the error "cell
    table overflow"."""
    import adaptivesurfacereconstruction as asr
    pts = lattice9["pts"]
    with fresh_ops_context(gpu) as ctx:
        ctx.set_option("knn_cells", knn_cells)
        tree = asr.KDTree(pts)
        before = _regrows(ctx)
        for k in (1, 24, 40):
            r = tree.compute_k_radius(k)
            if k == 1:
                got = _regrows(ctx) - before
                print("kNN radius (knn_cells %d): %d regrows" % (knn_cells, got))
                assert got >= 2
            assert r.dtype == np.float32 and np.array_equal(r, lattice9["knn"][k]), (k, np.abs(r - lattice9["knn"][k]).max())
        assert _regrows(ctx) - before == got  # the growth is kept: the later calls start with the table that fits


def test_inlier_vote_on_a_crowded_lattice(gpu, lattice9):
    """KDTree.compute_inlier as the first call on a fresh context: it enters the retry loop by itself, two regrows as for
    the kNN radius.  The vote always takes the wave path (the cell path serves the radii alone), so knn_cells is not varied."""
    import adaptivesurfacereconstruction as asr
    r24 = np.array(lattice9["knn"][24])
    with fresh_ops_context(gpu) as ctx:
        tree = asr.KDTree(lattice9["pts"])
        before = _regrows(ctx)
        inl = tree.compute_inlier(r24, radius_fraction=0.9, k=24, outlier_threshold=3)
        got = _regrows(ctx) - before
        print("inlier vote: %d regrows" % got)
        votes = (r24[lattice9["order"]] < (r24 * np.float32(0.9))[:, None]).sum(1)
        assert np.array_equal(inl, votes < 3)
        assert got >= 2


def test_radius_neighbor_count_on_a_crowded_lattice(gpu, lattice9):
    """KDTree.compute_radius_neighbors, the first call on a fresh context with radii of the levels 3..5: that search hashes
    those levels, 1538 cells in 4096 slots = 64 buckets, 512 keys of level 5 with one residue -- 64 buckets fail, 256 fail,
    1024 hold: two regrows.  The second call (the radii of the 24 nearest neighbours, coarser levels) starts with the grown
    table of 1024 buckets, which holds the at most 514 cells (sites and the two corner points) of any of this cloud's levels
    up to 5 whatever their residues: no further regrow."""
    import adaptivesurfacereconstruction as asr
    pts = lattice9["pts"]
    r24 = np.array(lattice9["knn"][24])
    small = (np.float32(0.75) / np.float32([32, 16, 8]))[np.arange(len(pts)) % 3]
    with fresh_ops_context(gpu) as ctx:
        tree = asr.KDTree(pts)
        before = _regrows(ctx)
        cnt = tree.compute_radius_neighbors(small)
        got = _regrows(ctx) - before
        print("radius neighbour count: %d regrows" % got)
        assert cnt == O.radius_count(pts, small).tolist()
        assert got >= 2
        cnt = tree.compute_radius_neighbors(r24 * 1.3)
        again = _regrows(ctx) - before - got
        print("radius neighbour count, second call: %d regrows" % again)
        assert cnt == O.radius_count(pts, (r24 * 1.3).astype(np.float32)).tolist()
        assert again == 0


# ---- case 4: nearest point and attribute transfer on the same cloud ---------------------------------------------------
def test_nearest_and_attributes_keep_the_grown_table(gpu, lattice9):
    """the two entry points that had a retry loop already: the first call on a fresh context regrows the cell table, the
    second starts with the grown one (the growth is kept on the context)"""
    pts, rad, bb = lattice9["pts"], lattice9["rad"], lattice9["bb"]
    frame = _lib.frame_init(*bb)
    rng = np.random.default_rng(9)
    q = np.concatenate([pts[rng.integers(0, len(pts), 3000)] + rng.normal(size=(3000, 3)).astype(np.float32) * np.float32(0.01),
                        rng.uniform(0, 1, size=(1000, 3)).astype(np.float32)]).astype(np.float32)
    with fresh_ops_context(gpu) as ctx:
        check_nearest(gpu, pts, q, frame=frame, what="crowded lattice, first call")
        first = _regrows(ctx)
        check_nearest(gpu, pts, q, frame=frame, what="crowded lattice, second call")
        print("nearest point: %d regrows, then %d" % (first, _regrows(ctx) - first))
        assert first >= 1 and _regrows(ctx) == first
    # attributes: queries near the points, sizes of the level-5 voxels, widened up to three times (levels 5..2)
    q = np.clip(q[:3000], 0.001, 0.999).astype(np.float32)
    sizes = np.full(len(q), 1 / 32, np.float32)
    attr = rng.uniform(0, 255, size=(len(pts), 4)).astype(np.float32)
    ref = transfer_reference(pts, rad, attr, q, sizes, 3, MIN_WEIGHT, -7.0, frame=frame)
    with fresh_ops_context(gpu) as ctx:
        tp, tr, ta, tq, ts = (_t(a, gpu) for a in (pts, rad, attr, q, sizes))
        seen = []
        for call in ("first", "second"):
            before = _regrows(ctx)
            out, weight, widen = ops.point_attributes_at(frame, tp, tr, ta, tq, ts, 3, MIN_WEIGHT, -7.0, return_info=True)
            seen.append(_regrows(ctx) - before)
            _check_against_reference(out.cpu().numpy(), weight.cpu().numpy(), widen.cpu().numpy(), ref,
                                     float(np.abs(attr).max()), MIN_WEIGHT, -7.0, "crowded lattice, %s call" % call)
        print("attributes: %d regrows, then %d" % tuple(seen))
        assert seen[0] >= 1 and seen[1] == 0


# ---- cases 5 and 6: the whole build -----------------------------------------------------------------------------------
def _geometry(pts, rad, bb):
    ref = parity.oracle_geometry(pts, rad, bb[0], bb[1])
    for i in range(4):  # the down lists are the inverted up lists (net_definitions_torch.py:548-559)
        d = O.invert_neighbors_list(len(ref["voxel_keys%d" % (i + 1)]), ref["up_neighbors_index%d" % i],
                                    ref["up_neighbors_row_splits%d" % i], ref["up_neighbors_kernel_index%d" % i])
        ref["down_neighbors_index%d" % i], ref["down_neighbors_row_splits%d" % i], ref["down_neighbors_kernel_index%d" % i] = d
    return ref


def _check_build(pipe, ref, what):
    """integer structures of all five grids and the aggregation arrays of the last build, bit for bit"""
    for i in range(5):
        assert np.array_equal(_u64(pipe.get("voxel_keys%d" % i)), ref["voxel_keys%d" % i]), (what, i)
        lists = ["neighbors"] + (["up_neighbors", "down_neighbors"] if i < 4 else [])
        for name in (l + s for l in lists for s in ("_index", "_kernel_index", "_row_splits")):
            assert np.array_equal(pipe.get(name + str(i)).cpu().numpy(), ref[name + str(i)]), (what, name, i)
    for name in ("aggregation_row_splits", "aggregation_neighbors_index", "aggregation_neighbors_dist"):
        assert np.array_equal(pipe.get(name).cpu().numpy(), ref[name]), (what, name)


def test_whole_path_on_a_crowded_lattice(gpu):
    """lattice_sites(8, 3, 5) through the whole path: 512 leaves of level 5 with one residue, so the search's cell tables
    (the early one and the query's own) overflow and are rebuilt; structures bit for bit, values within the tolerance of
    test_gpu_network.py; the stand-alone coarsening chain on the build's grids"""
    pts, nrm, rad, bb = C.lattice_sites(8, 3, 5)
    weights = synth.make_weights(4, seed=5)
    with O.precise():
        ref = parity.oracle_forward(pts, nrm, rad, bb[0], bb[1], weights)
    ref.update(_geometry(pts, rad, bb))
    pipe = ImplicitPipeline(weights, device=gpu)
    values = pipe.forward(_t(pts, gpu), _t(nrm, gpu), _t(rad, gpu), bb[0], bb[1]).clone()
    got = _regrows(pipe.ctx)
    print("whole path on the lattice: %d regrows" % got)
    _check_build(pipe, ref, "lattice forward")
    _close(pipe.get("feats1").cpu().numpy(), ref["feats1"])
    _close(values.cpu().numpy(), ref["values"])
    keys = pipe.get("voxel_keys0")
    for i in range(4):
        nxt, up_idx, up_kidx, up_rs = ops.grid_coarsen(keys)
        assert np.array_equal(_u64(nxt), ref["voxel_keys%d" % (i + 1)])
        assert np.array_equal(up_idx.cpu().numpy(), ref["up_neighbors_index%d" % i])
        assert np.array_equal(up_kidx.cpu().numpy(), ref["up_neighbors_kernel_index%d" % i])
        assert np.array_equal(up_rs.cpu().numpy(), ref["up_neighbors_row_splits%d" % i])
        keys = nxt
    assert got >= 1


@pytest.fixture(scope="module")
def build_clouds():
    """the three clouds of the driver matrix with their oracle geometry (computed once, never changed)"""
    out = {}
    for name, (pts, nrm, rad, bb) in (("lattice", C.lattice_sites(8, 3, 5)), ("clump", C.deep_clump()),
                                      ("scan", _scan(20000, 21, 10.0))):
        out[name] = (pts, rad, bb, _geometry(pts, rad, bb))
    return out


@pytest.mark.parametrize("overlap,early_sort,early_cells", [(1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 1, 1)])
def test_build_driver_matrix(gpu, build_clouds, overlap, early_sort, early_cells):
    """the host-chosen paths of implicit_build: search on the auxiliary stream or after the grids, its point sort and its
    cell table started beside the octree or not.  Lattice cloud on a fresh context (with early_cells the early table
    overflows and is dropped, the query grows its own), again on the same context (the early table is built at the grown
    size and used), then the clump whose leaves are deeper than the early sort's least depth, then the mixed scan.
    The driver reads early_sort and early_cells only when overlap is set, so (0, 1, 1) is the build without overlap and
    nothing more; the three tuples with overlap = 1 are the combinations that differ."""
    pipe = ImplicitPipeline(synth.make_weights(4, seed=1), device=gpu)
    opts = dict(overlap=overlap, early_sort=early_sort, early_cells=early_cells)
    saved = {k: pipe.ctx.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            pipe.ctx.set_option(k, v)
        seen = []
        for name in ("lattice", "lattice", "clump", "scan"):
            pts, rad, bb, ref = build_clouds[name]
            before = _regrows(pipe.ctx)
            pipe.build(_t(pts, gpu), _t(rad, gpu), bb[0], bb[1])
            seen.append(_regrows(pipe.ctx) - before)
            _check_build(pipe, ref, (name, len(seen)))
        print("build overlap=%d early_sort=%d early_cells=%d: regrows %s" % (overlap, early_sort, early_cells, seen))
        assert seen[0] >= 1
        assert seen[1] < seen[0]  # the cell table's growth is kept on the context (the key maps' is not)
    finally:
        for k, v in saved.items():
            pipe.ctx.set_option(k, v)
