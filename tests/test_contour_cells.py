"""CPU tests of tests/contour_cells.py: the generators against the plain restatement and the oracle, what the oracle must
give on rings whatever libstdc++ does, and the coverage that tests/test_gpu_contour_cells.py relies on.  No GPU."""
import numpy as np
import pytest

import contour_cells as C
from oracle import oracle as O


def _oracle(values, duals, positions, thr=1.0):
    """-> (vertices, triangles), or None where the oracle ends in "cannot sort duals\""""
    try:
        return O.create_triangle_mesh(values, duals, positions, thr)
    except RuntimeError as e:
        assert "cannot sort duals" in str(e)
        return None


def _agrees(r, mesh):
    v, t = mesh
    na = int(r.active.sum())
    assert (v.shape[0], t.shape[0]) == (r.num_vertices, r.num_triangles)
    assert np.array_equal(v[:na].view(np.uint32), r.vertices.view(np.uint32))
    assert t.shape[0] == 0 or (t.min() >= 0 and t.max() < v.shape[0])


def _ring_inputs():
    for n in C.RING_N + (30,):
        for pad in C.RING_PADS:
            yield "ring%d-pad%d" % (n, pad), C.ring(n, pad=pad), n
    for n, gap in C.OPEN_RINGS:
        yield "open%d-%d" % (n, gap), C.ring(n, missing=(gap,), pad=2), n - 1
    for n, own in C.ONCE_RINGS:
        yield "once%d-%d" % (n, own), C.ring(n, owner=own, pad=2), n


def test_rings_against_restatement_and_oracle():
    reached = set()
    for name, (v, d, p), n in _ring_inputs():
        r = C.Restatement(v, d, p)
        assert n in r.n_histogram, name
        reached.update(r.n_histogram)
        _agrees(r, _oracle(v, d, p))
    assert reached >= {1, 2, 3, 4, 5, 8, 9, 13, 14, 15, 28, 29, 30}
    for n, own in C.ONCE_RINGS:  # emitted once: one fan, not n
        v, d, p = C.ring(n, owner=own, pad=2)
        r = C.Restatement(v, d, p)
        assert r.n_histogram[n] == 1 and r.num_triangles == n


def _turns(wedges, n):
    """steps from each entry of a cyclic sequence of wedge numbers to the next, counted downwards mod n"""
    w = np.asarray(wedges)
    return (w - np.roll(w, -1)) % n


@pytest.mark.parametrize("n,missing,owner", [(3, (), None), (4, (), None), (5, (), None), (9, (), None),
                                              (14, (), None), (29, (), None), (30, (), None), (6, (0,), None),
                                              (6, (3,), None), (12, (11,), None), (20, (7,), None), (29, (13,), None),
                                              (8, (), 3), (29, (), 7), (4, (2,), None), (5, (0,), None)])
def test_ring_fans_are_discs_with_one_winding(n, missing, owner):
    """The edge is oriented from a (negative) to b, and the only face of wedge i that holds the directed edge (a, b) is
    {a, b, s_i}, which wedge i - 1 alone shares (contouring.cpp:229-245): whatever cell the walk starts from, the cells
    come out in descending cyclic wedge order.  So every fan is a closed disc -- each ring vertex the first corner of
    one triangle and the second of another, the centre in all -- every triangle turns downwards once, and an open ring
    gives the same fan with the missing sector spanned by one triangle."""
    pad = 3
    v, d, p = C.ring(n, missing=missing, pad=pad, owner=owner)
    r = C.Restatement(v, d, p)
    vtx, tri = _oracle(v, d, p)
    wedge = C.ring_wedges(n, missing, pad)
    k = n - len(missing)
    na = len(wedge)
    present = set(int(w) for w in wedge[pad:])
    emitted = k if owner is None else 1
    if k >= 5:
        assert tri.shape[0] == emitted * k and vtx.shape[0] == na + emitted
        for f in range(emitted):
            fan = tri[f * k:(f + 1) * k]
            assert np.all(fan[:, 2] == na + f)
            assert np.array_equal(fan[:, 1], np.roll(fan[:, 0], -1))  # a closed cycle
            assert set(wedge[fan[:, 0]].tolist()) == present and len(set(fan[:, 0].tolist())) == k
            steps = _turns(wedge[fan[:, 0]], n)
            assert steps.sum() == n and np.all(steps >= 1) and np.all(steps <= 1 + len(missing))
            centre = vtx[fan[:, 0]].astype(np.float32)
            acc = np.zeros(3, np.float32)
            for row in centre:  # f32 sum in fan order, one division
                acc = acc + row
            assert np.array_equal((acc / np.float32(k)).view(np.uint32), vtx[na + f].view(np.uint32))
    else:
        assert tri.shape[0] == emitted * (k - 2) and vtx.shape[0] == na
        for f in range(emitted):
            part = tri[f * (k - 2):(f + 1) * (k - 2)]
            assert set(wedge[part.ravel()].tolist()) == present
            for t in part:
                assert _turns(wedge[t], n).sum() == n  # one downward turn: the same winding as the fans


def test_two_arcs_cannot_be_sorted_from_any_start():
    n, gaps = C.TWO_GAPS
    v, d, p = C.ring(n, missing=gaps)
    r = C.Restatement(v, d, p)
    assert r.n_histogram == {n - 2: n - 2}
    for e in r.edges:
        reversals, sorts = r.min_reversals(e)
        assert reversals >= 2 and not sorts
    assert _oracle(v, d, p) is None
    # one gap: some start needs the reversal, none needs two, all sort
    v, d, p = C.ring(12, missing=(11,))
    r = C.Restatement(v, d, p)
    e = next(e for e in r.edges if e[4] == 11)
    assert r.min_reversals(e) == (0, True)


def test_two_cells_without_a_common_face():
    """n == 2 emits no triangle, but the reference sorts the cells before it looks at n (contouring.cpp:360-369)"""
    v, d, p = C.ring(4, missing=(1, 3))
    r = C.Restatement(v, d, p)
    assert r.n_histogram == {2: 2} and r.num_triangles == 0
    assert all(not r.min_reversals(e)[1] for e in r.edges)
    assert _oracle(v, d, p) is None
    v, d, p = C.ring(4, missing=(2, 3))  # two neighbours: sorted, nothing emitted
    vtx, tri = _oracle(v, d, p)
    assert vtx.shape[0] == 2 and tri.shape[0] == 0


def test_merged_lattices():
    meshes, failures, distinct, ns = 0, 0, set(), set()
    for m, frac, seed in C.LATTICES:
        v, d, p = C.merged_lattice(m, frac, seed)
        assert d.shape == ((m - 1) ** 3, 8) and d.min() >= 0 and d.max() < len(v)
        r = C.Restatement(v, d, p)
        distinct.update(len(set(c.tolist())) for c in r.cells)
        ns.update(r.n_histogram)
        mesh = _oracle(v, d, p)
        if mesh is None:
            failures += 1
            assert any(not r.min_reversals(e)[1] for e in r.edges if e[4] > 1)
        else:
            meshes += 1
            _agrees(r, mesh)
            assert np.isfinite(mesh[0]).all()
    assert meshes * 4 >= 3 * len(C.LATTICES) and failures >= 1
    assert distinct >= {4, 5, 6, 7, 8} and ns >= {1, 2, 3, 4, 5, 6, 7}
    v, d, p = C.merged_lattice(2, 0.0, 0)
    assert d.shape == (1, 8)


def test_special_values_decide_crossings():
    seen = {}
    for name, v, d, p, thr in C.special_cases():
        r = C.Restatement(v, d, p, thr)
        mesh = _oracle(v, d, p, thr)
        assert mesh is not None, name
        _agrees(r, mesh)
        assert np.isfinite(mesh[0]).all(), name  # a vertex that is not finite could not be compared on bits
        kinds = C.deciding_classes(v, d, thr)
        if name.startswith("lattice"):
            assert all(c >= 1 for c in kinds.values()), (name, kinds)
        for k, c in kinds.items():
            seen[k] = seen.get(k, 0) + c
    assert set(seen) == {"zero", "negative zero", "nan", "infinity", "denormal"} and all(seen.values())
    v = C.with_special_values(C.merged_lattice(7, 0.0, 5)[0], 0, 1.0)
    assert (v[:, 1] == np.float32(1)).any() and (v[:, 1] == np.nextafter(np.float32(1), np.float32(2))).any()


def test_zero_and_denormal_crossings_in_the_restatement():
    """what the odd values must do, stated on single cells: a zero of either sign and a NaN cross nothing, a denormal
    crosses like any number and puts the vertex on its own voxel, two infinities put it halfway (t is NaN)"""
    v, d, p = C.ring(1)
    for a, b, active, t in ((0.0, 1.0, False, None), (-0.0, 1.0, False, None), (np.nan, 1.0, False, None),
                            (-1e-45, 1.0, True, 0.0), (-1.0, 1e-45, True, 1.0), (-np.inf, 1.0, True, None),
                            (-1.0, np.inf, True, None), (-np.inf, np.inf, True, 0.5), (-3.4e38, 3.4e38, True, 0.5)):
        w = v.copy()
        w[:, 0] = np.float32(b)
        w[0, 0] = np.float32(a)
        w = w[[0, 1, 2]]
        cell = np.array([[0, 1, 1, 1, 1, 1, 1, 1]], np.int64)  # crossings: (0,1), (2,0), (0,4), all between voxels 0 and 1
        r = C.Restatement(w, cell, p[:3])
        assert bool(r.active[0]) == active
        mesh = _oracle(w, cell, p[:3])
        assert mesh[0].shape[0] == int(active)
        if active:
            assert np.array_equal(mesh[0].view(np.uint32), r.vertices.view(np.uint32))
            p0, p1 = p[0].astype(np.float64), p[1].astype(np.float64)
            if t is None:  # one infinite end: t is NaN (halfway) walking one way along the edge, 0 walking the other
                assert np.isfinite(mesh[0]).all()
            elif t == 0.5:  # the same midpoint from all three crossings
                at = 0.5 * p0 + 0.5 * p1
                want = ((at + at + at) / 3).astype(np.float32)
                assert np.array_equal(mesh[0][0].view(np.uint32), want.view(np.uint32))
            else:  # t is 0 or 1 but for a denormal: the vertex rounds to the voxel whose value is next to nothing
                assert np.array_equal(mesh[0][0].view(np.uint32), p[int(t)].view(np.uint32))


def test_threshold_gate_is_strict():
    """u > thr on both ends closes an edge: equality leaves it open, a NaN unsigned value or threshold leaves it open"""
    v, d, p = C.ring(5)
    for u, thr, open_ in ((1.0, 1.0, True), (np.nextafter(np.float32(1), np.float32(2)), 1.0, False),
                          (np.nan, 1.0, True), (5.0, np.nan, True), (5.0, np.inf, True), (np.inf, np.inf, True),
                          (np.inf, 3.0e38, False), (0.0, -1.0, False), (0.0, 0.0, True)):
        w = v.copy()
        w[:, 1] = np.float32(u)
        r = C.Restatement(w, d, p, thr)
        mesh = _oracle(w, d, p, thr)
        assert bool(r.active.any()) == open_ and (mesh[0].shape[0] > 0) == open_, (u, thr)
        _agrees(r, mesh)


def test_plane_field_reaches_the_rims():
    hist = {}
    for noise in (0.0, 0.5):
        v, d, p = C.plane_field(5000, 0, noise)
        r = C.Restatement(v, d, p)
        _agrees(r, _oracle(v, d, p))
        for k, c in r.n_histogram.items():
            hist[k] = hist.get(k, 0) + c
    assert all(hist.get(k, 0) >= 2 for k in (1, 2, 3, 4, 5, 6, 7)) and max(hist) <= 8
