"""GPU test of what the four point-index entry points share (csrc/asr_geom.hip, build_point_index_grown): the cell table's
growth is kept on the context, so the growth one entry point had to find serves the others.  test_gpu_table_regrow.py shows
that each of them regrows by itself on a fresh context and keeps its own growth; here they run one after the other on ONE
context and only the first may regrow.

The cloud is that file's lattice9 (lattice_sites(8, 9, 5) with the two corner points, 4 610 points); its docstrings give
the counts.  The kNN radius and the nearest-point search hash the levels 0..5: 1611 cells in 4096 slots = 64 buckets, 512
keys with one residue -- 64 and 256 buckets fail, 1024 hold, two regrows.  1024 buckets then hold the cells of every level
up to 5 of this cloud (at most 514 of one residue), so the radius count (levels 3..5, 1538 cells), the attribute search
(levels 5..2) and the two searches on the levels 0..5 all fit the first table they build: zero regrows."""
import numpy as np
import pytest

from asr_hip import _lib, ops
from oracle import oracle as O
from test_attributes import transfer_reference
from test_gpu_attributes import MIN_WEIGHT, _check_against_reference
from test_gpu_nearest import check_nearest
from test_gpu_table_regrow import _regrows, _t, lattice9  # noqa: F401 (lattice9: the module-scoped fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lattice9_queries(lattice9):  # noqa: F811
    """the queries, sizes and attributes of test_nearest_and_attributes_keep_the_grown_table with the attribute reference,
    and the radius counts of the level-3..5 radii of test_radius_neighbor_count_on_a_crowded_lattice (computed once)"""
    pts, rad, bb = lattice9["pts"], lattice9["rad"], lattice9["bb"]
    frame = _lib.frame_init(*bb)
    rng = np.random.default_rng(9)
    q = np.concatenate([pts[rng.integers(0, len(pts), 3000)] + rng.normal(size=(3000, 3)).astype(np.float32) * np.float32(0.01),
                        rng.uniform(0, 1, size=(1000, 3)).astype(np.float32)]).astype(np.float32)
    qa = np.clip(q[:3000], 0.001, 0.999).astype(np.float32)
    sizes = np.full(len(qa), 1 / 32, np.float32)
    attr = rng.uniform(0, 255, size=(len(pts), 4)).astype(np.float32)
    ref = transfer_reference(pts, rad, attr, qa, sizes, 3, MIN_WEIGHT, -7.0, frame=frame)
    small = (np.float32(0.75) / np.float32([32, 16, 8]))[np.arange(len(pts)) % 3]
    return dict(frame=frame, q=q, qa=qa, sizes=sizes, attr=attr, ref=ref, small=small,
                small_counts=O.radius_count(pts, small).tolist())


def _steps(gpu, L, Q):
    """name -> call that runs one entry point on the current operator context and compares it with its reference"""
    import adaptivesurfacereconstruction as asr
    pts = L["pts"]
    r24 = np.array(L["knn"][24])
    tree = asr.KDTree(pts)

    def k_radius():
        r = tree.compute_k_radius(24)
        assert r.dtype == np.float32 and np.array_equal(r, L["knn"][24])

    def inlier():
        inl = tree.compute_inlier(r24, radius_fraction=0.9, k=24, outlier_threshold=3)
        votes = (r24[L["order"]] < (r24 * np.float32(0.9))[:, None]).sum(1)
        assert np.array_equal(inl, votes < 3)

    def radius_neighbors():
        assert tree.compute_radius_neighbors(Q["small"]) == Q["small_counts"]

    def nearest():
        check_nearest(gpu, pts, Q["q"], frame=Q["frame"], what="shared index")

    def attributes():
        tp, tr, ta, tq, ts = (_t(a, gpu) for a in (pts, L["rad"], Q["attr"], Q["qa"], Q["sizes"]))
        out, weight, widen = ops.point_attributes_at(Q["frame"], tp, tr, ta, tq, ts, 3, MIN_WEIGHT, -7.0, return_info=True)
        _check_against_reference(out.cpu().numpy(), weight.cpu().numpy(), widen.cpu().numpy(), Q["ref"],
                                 float(np.abs(Q["attr"]).max()), MIN_WEIGHT, -7.0, "shared index")

    return dict(k_radius=k_radius, inlier=inlier, radius_neighbors=radius_neighbors, nearest=nearest, attributes=attributes)


ORDERS = {"k_radius-first": ["k_radius", "inlier", "radius_neighbors", "nearest", "attributes"],
          "nearest-first": ["nearest", "attributes", "radius_neighbors", "inlier", "k_radius"]}


@pytest.mark.parametrize("which", list(ORDERS))
def test_growth_of_one_entry_point_serves_the_others(gpu, lattice9, lattice9_queries, which):  # noqa: F811
    """the first entry point on a fresh context regrows the table twice (both orders start with a search that hashes the
    levels 0..5); every later one builds a table that holds at once, and each result still equals its reference"""
    order = ORDERS[which]
    with ops.fresh_context(gpu) as ctx:
        steps = _steps(gpu, lattice9, lattice9_queries)
        seen = []
        for name in order:
            before = _regrows(ctx)
            steps[name]()
            seen.append(_regrows(ctx) - before)
        print("regrows: " + ", ".join("%s %d" % p for p in zip(order, seen)))
        assert seen[0] >= 2
        assert seen[1:] == [0] * (len(order) - 1)
