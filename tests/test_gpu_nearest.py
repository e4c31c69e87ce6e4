"""GPU tests of the surface comparison: asr_hip_nearest_point bit for bit against a numpy brute-force
search, asr_hip_mesh_sample on meshes whose areas are exact in binary, and the metrics built on both
(asr_hip.metrics, adaptivesurfacereconstruction.evaluate_mesh, asrtool --compare).

Nearest point: the reference is d2 = (dx*dx + dy*dy) + dz*dz in float32 and argmin, which takes the first minimum, i.e.
the smallest index; indices and squared distances must be array_equal, every row, no tolerance.

Sampling: axis-aligned right triangles with power-of-two legs, so areas, prefix sums and S * A_t / A are exact.
  - containment: with delta = 16 * 2^-24 * max|coordinate| (the point is three rounded multiply-adds of values of that
    magnitude) the float64 barycentric coordinates of a sample in ITS triangle lie in [-delta, 1 + delta] and its
    distance to the triangle's plane is at most delta;
  - counts: |count_t - S A_t / A| <= 2: sample s owns the stratum [s, s + 1) A / S, and a parameter interval of length
    L (in strata) meets at most ceil(L) + 1 strata and contains at least floor(L) - 1;
  - uniformity inside a triangle: each barycentric coordinate has mean 1/3 and variance 1/18, so the mean of S = 90 000
    samples has sigma = sqrt(1 / 18 / S) = 7.9e-4; the bound 4e-3 is five sigma (a missing sqrt gives a mean of 1/2).

Metrics: two unit squares at z = 0 and z = 0.25 sampled with S = 20 000: every distance is at least 0.25 exactly, and
chamfer_l1 <= 0.26 as soon as the samples' covering radius is at most 0.07 (sqrt(0.0625 + 0.0049) = 0.2596), which for
20 000 uniform points fails with probability below e^-300.
"""
import json
import os

import numpy as np
import pytest
import torch

import asrtool
from asr_hip import _lib, metrics, ops, ply, synth
from asr_hip._lib import AsrHipError

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# nearest point
# ---------------------------------------------------------------------------------------------------------------------
def brute_nearest(points, queries):
    """(index int32 [M], sqdist f32 [M]) of the float32 formula; a non-finite query row gives -1 and +inf"""
    points, queries = np.asarray(points, np.float32), np.asarray(queries, np.float32)
    idx = np.full(len(queries), -1, np.int32)
    sq = np.full(len(queries), np.inf, np.float32)
    ok = np.flatnonzero(np.isfinite(queries).all(1))
    px, py, pz = (np.ascontiguousarray(points[:, c])[None, :] for c in range(3))
    step = max(1, (1 << 22) // max(1, len(points)))
    for s in range(0, len(ok), step):
        rows = ok[s:s + step]
        q = queries[rows]
        dx, dy, dz = px - q[:, 0:1], py - q[:, 1:2], pz - q[:, 2:3]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        i = d2.argmin(1)
        idx[rows] = i
        sq[rows] = d2[np.arange(len(rows)), i]
    return idx, sq


def frame_of(points, margin=0.1):
    return _lib.frame_init(*synth.bounding_box(np.asarray(points, np.float32), margin))


def check_nearest(gpu, points, queries, frame=None, what=""):
    frame = frame or frame_of(points)
    idx, sq = ops.nearest_point(frame, torch.from_numpy(points).to(gpu), torch.from_numpy(queries).to(gpu))
    assert idx.dtype == torch.int32 and sq.dtype == torch.float32
    assert tuple(idx.shape) == (len(queries),) and tuple(sq.shape) == (len(queries),)
    ref_idx, ref_sq = brute_nearest(points, queries)
    idx, sq = idx.cpu().numpy(), sq.cpu().numpy()
    bad = np.flatnonzero((idx != ref_idx) | (sq.view(np.uint32) != ref_sq.view(np.uint32)))
    print("%s: n=%d m=%d, %d rows differ%s" % (what, len(points), len(queries), len(bad),
                                                 "" if not len(bad) else " (first: row %d, got %d / %r, want %d / %r)"
                                                 % (bad[0], idx[bad[0]], sq[bad[0]], ref_idx[bad[0]], ref_sq[bad[0]])))
    assert np.array_equal(idx, ref_idx), what
    assert np.array_equal(sq.view(np.uint32), ref_sq.view(np.uint32)), what
    return idx, sq


@pytest.mark.parametrize("n", [1, 5, 64, 65])
def test_nearest_small_clouds(gpu, n):
    rng = np.random.default_rng(n)
    pts = rng.normal(size=(n, 3)).astype(np.float32)
    check_nearest(gpu, pts, rng.normal(size=(300, 3)).astype(np.float32), what="small n=%d" % n)


def test_nearest_lattice_ties(gpu):
    """12^3 lattice in a shuffled order: distance 0 at the points, 8-way ties at the cell centres, 4-way at the face centres"""
    g = np.arange(12, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts = np.ascontiguousarray(pts[np.random.default_rng(0).permutation(len(pts))])
    h = g[:-1] + np.float32(0.5)
    cells = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3)
    faces = np.concatenate([np.stack(np.meshgrid(*[g if a == ax else h for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
                            for ax in range(3)])
    idx, sq = check_nearest(gpu, pts, pts.copy(), what="lattice points")
    assert np.all(sq == 0) and np.array_equal(idx, np.arange(len(pts)))
    _, sq = check_nearest(gpu, pts, cells.astype(np.float32), what="lattice cell centres")
    assert np.all(sq == np.float32(0.75))
    _, sq = check_nearest(gpu, pts, faces.astype(np.float32), what="lattice face centres")
    assert np.all(sq == np.float32(0.5))


def test_nearest_duplicates_pick_the_smaller_index(gpu):
    pts, _ = synth.sphere_cloud(3000, 1)
    pts[:50] = pts[50:100]
    rng = np.random.default_rng(2)
    idx, sq = check_nearest(gpu, pts, pts.copy(), what="duplicates, the points themselves")
    assert np.all(sq == 0) and np.array_equal(idx[50:100], np.arange(50)) and np.array_equal(idx[:50], np.arange(50))
    check_nearest(gpu, pts, (pts + rng.normal(size=pts.shape) * 1e-3).astype(np.float32), what="duplicates, jittered")


def _scan_queries(pts, frame, seed):
    rng = np.random.default_rng(seed)
    lo, hi = pts.min(0), pts.max(0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    corners = np.array([[(frame.bb_min, frame.bb_max)[(c >> d) & 1][d] for d in range(3)] for c in range(8)], np.float32)
    weird = np.array([[np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    return np.concatenate([pts + rng.normal(size=pts.shape) * 1e-3,          # next to the points
                           rng.uniform(lo, hi, size=(2000, 3)),              # in the box, far from the surface
                           rng.uniform(mid - 3 * half, mid + 3 * half, size=(500, 3)),  # mostly outside the frame
                           corners, weird]).astype(np.float32)


def test_nearest_scan_cloud(gpu):
    p, _ = synth.scan_cloud(6000, seed=5, device="cpu")
    pts = np.ascontiguousarray(p.numpy())
    frame = frame_of(pts)
    q = _scan_queries(pts, frame, 6)
    idx, sq = check_nearest(gpu, pts, q, frame, what="scan cloud")
    assert np.all(idx[-2:] == -1) and np.all(np.isposinf(sq[-2:]))
    assert np.all(idx[:-2] >= 0) and np.all(np.isfinite(sq[:-2]))


def test_nearest_mixed_density_with_a_crowded_cell(gpu):
    """3000 points within 2e-5 of one point: that cell exceeds the crowd limit of the search (1024) and its queries
    start on a finer level; 100 isolated points far away stretch the frame so that the scene itself is a few cells"""
    p, _ = synth.scan_cloud(6000, seed=7, device="cpu", density_variance=10.0)
    rng = np.random.default_rng(8)
    base = p.numpy()
    clump = base[123] + rng.uniform(-2e-5, 2e-5, size=(3000, 3))
    far = rng.uniform(-1, 1, size=(100, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(20, 40, size=(100, 1))
    pts = np.ascontiguousarray(np.concatenate([base, clump, far]).astype(np.float32))
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    frame = frame_of(pts)
    idx, sq = check_nearest(gpu, pts, _scan_queries(pts, frame, 9), frame, what="mixed density + crowded cell")
    assert np.all(idx[-2:] == -1) and np.all(np.isposinf(sq[-2:]))


def test_nearest_sizes_determinism_and_kdtree(gpu):
    import adaptivesurfacereconstruction as asr
    pts, _ = synth.sphere_cloud(2000, 3)
    frame = frame_of(pts)
    dp = torch.from_numpy(pts).to(gpu)
    idx, sq = ops.nearest_point(frame, dp, torch.zeros((0, 3), device=gpu))
    assert tuple(idx.shape) == (0,) and tuple(sq.shape) == (0,) and idx.dtype == torch.int32
    q = np.random.default_rng(4).normal(size=(257, 3)).astype(np.float32)
    idx, sq = check_nearest(gpu, pts, q, frame, what="m = 257")
    idx2, sq2 = ops.nearest_point(frame, dp, torch.from_numpy(q).to(gpu))
    assert np.array_equal(idx2.cpu().numpy(), idx) and np.array_equal(sq2.cpu().numpy().view(np.uint32), sq.view(np.uint32))
    kidx, kdist = asr.KDTree(pts).nearest(q)
    assert kidx.dtype == np.int32 and kdist.dtype == np.float32
    assert np.array_equal(kidx, idx) and np.array_equal(kdist, np.sqrt(sq))


def test_nearest_rejects_bad_input(gpu):
    import adaptivesurfacereconstruction as asr
    pts = torch.zeros((4, 3), device=gpu)
    frame = _lib.frame_init([-1, -1, -1], [1, 1, 1])
    with pytest.raises(ValueError):
        ops.nearest_point(frame, pts, torch.zeros((5, 2), device=gpu))
    with pytest.raises(ValueError):
        ops.nearest_point(frame, torch.zeros(12, device=gpu), pts)
    with pytest.raises(ValueError):
        asr.KDTree(np.zeros((4, 3), np.float32)).nearest(np.zeros(3, np.float32))
    with pytest.raises(AsrHipError):
        ops.nearest_point(frame, pts.cpu(), pts)
    with pytest.raises(AsrHipError):
        ops.nearest_point(frame, pts, pts.cpu())
    with pytest.raises(AsrHipError):
        ops.nearest_point(frame, torch.zeros((0, 3), device=gpu), pts)


# ---------------------------------------------------------------------------------------------------------------------
# mesh sampling
# ---------------------------------------------------------------------------------------------------------------------
def _right_triangles():
    """right triangles with legs 1, 2 and 8 (areas 0.5 : 2 : 32 = 1 : 4 : 64) in the three coordinate planes at integer
    offsets, plus three triangles without area (a repeated corner, three collinear corners, three equal corners)"""
    vertices, triangles, areas = [], [], []

    def add(origin, leg, plane):
        a, b = [(0, 1), (1, 2), (2, 0)][plane]
        v0 = np.array(origin, np.float64)
        v1, v2 = v0.copy(), v0.copy()
        v1[a] += leg
        v2[b] += leg
        base = len(vertices)
        vertices.extend([v0, v1, v2])
        triangles.append([base, base + 1, base + 2])
        areas.append(leg * leg / 2.0)

    for i in range(5):
        add((4 * i, -3, 2), 1, i % 3)
    for i in range(3):
        add((-8, 16 * i, -4), 2, (i + 1) % 3)
    add((32, 32, 0), 8, 0)
    add((-64, 8, 16), 8, 2)
    base = len(vertices)
    vertices.extend([np.array(v, np.float64) for v in ((1, 1, 1), (2, 3, 4), (3, 5, 7))])
    for t in ([base, base, base + 1], [base, base + 1, base + 2], [base + 2, base + 2, base + 2]):
        triangles.insert(len(triangles) // 2, t)  # in the middle of the list
        areas.insert(len(areas) // 2, 0.0)
    return np.array(vertices, np.float32), np.array(triangles, np.int32), np.array(areas, np.float64)


@pytest.fixture(scope="module")
def sampled(gpu):
    v, t, areas = _right_triangles()
    S = 20000
    p, n, tri = ops.mesh_sample(torch.from_numpy(v).to(gpu), torch.from_numpy(t).to(gpu), S, seed=11, normals=True,
                                return_triangle=True)
    assert p.dtype == torch.float32 and tuple(p.shape) == (S, 3) and tuple(n.shape) == (S, 3)
    assert tri.dtype == torch.int32 and tuple(tri.shape) == (S,)
    return v, t, areas, p.cpu().numpy(), n.cpu().numpy(), tri.cpu().numpy()


def _barycentrics(v, t, p, tri):
    """float64 (b0, b1, b2) of p in its triangle (least squares in the plane) and the distance to the plane"""
    v = v.astype(np.float64)
    v0, e1, e2 = v[t[tri, 0]], v[t[tri, 1]] - v[t[tri, 0]], v[t[tri, 2]] - v[t[tri, 0]]
    d = p.astype(np.float64) - v0
    a11, a12, a22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (d * e1).sum(1), (d * e2).sum(1)
    det = a11 * a22 - a12 * a12
    b1, b2 = (r1 * a22 - r2 * a12) / det, (r2 * a11 - r1 * a12) / det
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.stack([1 - b1 - b2, b1, b2], 1), np.abs((d * nrm).sum(1)), nrm


def test_samples_lie_in_their_triangles(sampled):
    v, t, areas, p, n, tri = sampled
    assert tri.min() >= 0 and tri.max() < len(t)
    assert np.all(areas[tri] > 0), "a triangle without area was chosen"
    bary, plane, nrm = _barycentrics(v, t, p, tri)
    delta = 16 * EPS * np.abs(v).max()
    print("barycentric range [%.3g, %.3g], plane residual %.3g, delta %.3g" % (bary.min(), bary.max(), plane.max(), delta))
    assert bary.min() >= -delta and bary.max() <= 1 + delta
    assert plane.max() <= delta
    # unit face normals in corner order
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() <= 4 * EPS
    assert np.abs(n.astype(np.float64) - nrm).max() <= 4 * EPS


def test_sample_counts_follow_the_areas(sampled):
    v, t, areas, p, n, tri = sampled
    counts = np.bincount(tri, minlength=len(t))
    expect = len(tri) * areas / areas.sum()
    print("count - expectation:", np.round(counts - expect, 3).tolist())
    assert np.all(counts[areas == 0] == 0)
    assert np.abs(counts - expect).max() <= 2
    assert np.all(np.diff(tri) >= 0)  # stratified: sample s lies in stratum s of the prefix sums


def test_samples_are_uniform_inside_a_triangle(gpu):
    v = torch.tensor([[0, 0, 0.25], [4, 0, 0.25], [0, 2, 0.25]], dtype=torch.float32, device=gpu)
    t = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=gpu)
    p = ops.mesh_sample(v, t, 90000, seed=5)
    assert isinstance(p, torch.Tensor)
    p = p.cpu().numpy()
    assert np.all(p[:, 2] == np.float32(0.25))  # a triangle in a coordinate plane: points exactly in that plane
    bary, _, _ = _barycentrics(v.cpu().numpy(), t.cpu().numpy(), p, np.zeros(len(p), np.int64))
    print("mean barycentric coordinates:", bary.mean(0))
    assert np.abs(bary.mean(0) - 1 / 3).max() <= 4e-3
    # and of the right joint law: P(b0 > 1/2) = 1/4 for a uniform point
    assert abs((bary[:, 0] > 0.5).mean() - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / len(p))


def test_sampling_is_a_function_of_its_arguments(gpu, sampled):
    v, t, areas, p, n, tri = sampled
    dv, dt = torch.from_numpy(v).to(gpu), torch.from_numpy(t).to(gpu)
    p2, n2, tri2 = ops.mesh_sample(dv, dt, len(p), seed=11, normals=True, return_triangle=True)
    assert np.array_equal(p2.cpu().numpy().view(np.uint32), p.view(np.uint32))
    assert np.array_equal(n2.cpu().numpy().view(np.uint32), n.view(np.uint32)) and np.array_equal(tri2.cpu().numpy(), tri)
    p3 = ops.mesh_sample(dv, dt, len(p), seed=12).cpu().numpy()
    assert (p3 != p).any(1).mean() > 0.99
    big = ops.mesh_sample(dv, dt, 100, seed=2 ** 64 - 1)
    assert tuple(big.shape) == (100, 3) and bool(torch.isfinite(big).all())


def test_sampling_errors(gpu):
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=torch.float32, device=gpu)
    t = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=gpu)
    assert tuple(ops.mesh_sample(v, t, 0).shape) == (0, 3)
    none = torch.zeros((0, 3), dtype=torch.int32, device=gpu)
    assert tuple(ops.mesh_sample(v, none, 0).shape) == (0, 3)
    for bad in ([[0, 1, 3]], [[-1, 1, 2]]):
        with pytest.raises(AsrHipError, match="out of range"):
            ops.mesh_sample(v, torch.tensor(bad, dtype=torch.int32, device=gpu), 10)
    with pytest.raises(AsrHipError, match="no triangles"):
        ops.mesh_sample(v, none, 10)
    with pytest.raises(AsrHipError, match="area"):
        ops.mesh_sample(v, torch.tensor([[0, 0, 1], [2, 2, 2]], dtype=torch.int32, device=gpu), 10)
    with pytest.raises(ValueError):
        ops.mesh_sample(v[:, :2], t, 10)
    with pytest.raises(ValueError):
        ops.mesh_sample(v, t.reshape(-1), 10)
    with pytest.raises(ValueError):
        ops.mesh_sample(v, t, -1)
    with pytest.raises(AsrHipError):
        ops.mesh_sample(v.cpu(), t, 10)
    assert tuple(ops.mesh_sample(v, t, 10).shape) == (10, 3)  # the context is fine after the errors


# ---------------------------------------------------------------------------------------------------------------------
# metrics end to end
# ---------------------------------------------------------------------------------------------------------------------
def _square(z):
    v = np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def test_two_parallel_squares(gpu):
    (va, ta), (vb, tb) = _square(0.0), _square(0.25)
    dev = lambda x: torch.from_numpy(x).to(gpu)  # noqa: E731
    m = metrics.mesh_metrics(dev(va), dev(ta), (dev(vb), dev(tb)), 20000, (0.2, 0.5), seed=1)
    print(m)
    assert 0.25 <= m["chamfer_l1"] <= 0.26
    assert 0.25 <= m["accuracy"] <= 0.26 and 0.25 <= m["completeness"] <= 0.26
    assert m["fscore"] == [0.0, 1.0] and m["precision"] == [0.0, 1.0] and m["recall"] == [0.0, 1.0]
    assert m["normal_consistency"] == 1.0
    assert 0.0625 <= m["chamfer_l2"] <= 0.26 ** 2 and 0.25 <= m["hausdorff"] <= 0.27
    # no distance below 0.25, in either direction
    pa, pb = ops.mesh_sample(dev(va), dev(ta), 20000, seed=1), ops.mesh_sample(dev(vb), dev(tb), 20000, seed=2)
    for x, y in ((pa, pb), (pb, pa)):
        _, sq = ops.nearest_point(metrics.search_frame(y), y, x)
        assert float(sq.min()) >= 0.0625
    # a reference given as points (no normals): the same distances, no normal consistency
    m2 = metrics.mesh_metrics(dev(va), dev(ta), pb, 20000, (0.2, 0.5), seed=1)
    assert "normal_consistency" not in m2
    assert {k: v for k, v in m.items() if k != "normal_consistency"} == m2


def test_a_mesh_against_itself(gpu):
    v, t, _ = _right_triangles()
    p, n = ops.mesh_sample(torch.from_numpy(v).to(gpu), torch.from_numpy(t).to(gpu), 5000, seed=3, normals=True)
    m = metrics.point_set_metrics(p, p.clone(), (1e-3,), n, n.clone())
    assert m["accuracy"] == 0 and m["completeness"] == 0 and m["chamfer_l1"] == 0 and m["chamfer_l2"] == 0
    assert m["hausdorff"] == 0 and m["fscore"] == [1.0]
    assert abs(m["normal_consistency"] - 1) <= 4 * EPS


def test_point_set_metrics_match_brute_force(gpu):
    rng = np.random.default_rng(21)
    a = rng.normal(size=(3000, 3)).astype(np.float32)
    b = (rng.normal(size=(4000, 3)) * 1.1 + 0.05).astype(np.float32)
    thr = (0.05, 0.1, 0.3)
    got = metrics.point_set_metrics(torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu), thr)
    _, sq_ab = brute_nearest(b, a)
    _, sq_ba = brute_nearest(a, b)
    want = metrics.from_distances(sq_ab, sq_ba, thr)
    for k in ("precision", "recall", "fscore", "thresholds"):
        assert got[k] == want[k], k
    for k in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "hausdorff"):
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), k
    with pytest.raises(ValueError):
        metrics.point_set_metrics(torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu), thr, normals_a=torch.from_numpy(a).to(gpu))
    with pytest.raises(AsrHipError):
        metrics.point_set_metrics(torch.from_numpy(a), torch.from_numpy(b), thr)


def test_evaluate_mesh_and_the_command_line_agree_with_mesh_metrics(gpu, tmp_path, capsys):
    import adaptivesurfacereconstruction as asr
    va, ta, _ = _right_triangles()
    vb, tb = va + np.float32(0.125), ta
    dev = lambda x: torch.from_numpy(x).to(gpu)  # noqa: E731
    thr = (0.1, 0.25)
    want = metrics.mesh_metrics(dev(va), dev(ta), (dev(vb), dev(tb)), 5000, thr, seed=4)
    assert asr.evaluate_mesh(va, ta, reference_mesh=(vb, tb), num_samples=5000, thresholds=thr, seed=4) == want
    mesh, ref = str(tmp_path / "mesh.ply"), str(tmp_path / "ref.ply")
    ply.write_mesh(mesh, va, ta)
    ply.write_mesh(ref, vb, tb)
    assert asrtool.main(["--compare", mesh, ref, "--samples", "5000", "--thresholds", "0.1,0.25", "--seed", "4"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and json.loads(lines[0]) == want
    # a reference without faces is a point cloud; its normals are used
    pb, nb = ops.mesh_sample(dev(vb), dev(tb), 3000, seed=9, normals=True)
    cloud = str(tmp_path / "cloud.ply")
    ply.write_points(cloud, pb.cpu().numpy(), nb.cpu().numpy())
    want = metrics.mesh_metrics(dev(va), dev(ta), (pb, nb), 5000, thr, seed=4)
    assert "normal_consistency" in want
    assert asr.evaluate_mesh(va, ta, reference_points=pb.cpu().numpy(), reference_normals=nb.cpu().numpy(),
                             num_samples=5000, thresholds=thr, seed=4) == want
    assert asrtool.main(["--compare", mesh, cloud, "--samples", "5000", "--thresholds", "0.1,0.25", "--seed", "4"]) == 0
    assert json.loads(capsys.readouterr().out.strip()) == want
    # default thresholds: 0.5 % and 1 % of the diagonal of the reference's bounding box
    got = asr.evaluate_mesh(va, ta, reference_mesh=(vb, tb), num_samples=1000)
    diag = float(np.linalg.norm(vb.astype(np.float64).max(0) - vb.astype(np.float64).min(0)))
    assert got["thresholds"] == [0.005 * diag, 0.01 * diag]
    with pytest.raises(ValueError):
        asr.evaluate_mesh(va, ta)
    assert os.path.exists(mesh)
