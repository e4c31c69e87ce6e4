"""Mesh adjacency without a GPU: the numpy restatement of the edge table, the topology report and Taubin smoothing
(tests/mesh_adjacency_ref.py, the yardstick of tests/test_gpu_mesh_adjacency.py) on shapes with known answers, the new
exports and the struct size in the built library, and the argument checks that must come before any GPU work.

Measured with the restatement:
  UV sphere 30 x 60: V = 1 802, E = 5 400, F = 3 600, euler 2, every edge used twice, once forward; genus 0.
  33 x 33 plane without the triangles whose centroid has |x|, |y| < 0.1: 152 boundary edges in 2 loops, 25 unused
    vertices, euler 0 (a disc with one hole).
  Sphere with radial noise of sigma 0.01 (default_rng(0)), 10 iterations: rms distance from the unit sphere
    0.0100 -> 0.0040 with the defaults (lambda 0.5, mu -0.53); mean radius 1.0012 against 0.974 with mu = 0 (Laplacian).
  Summing the rows in descending instead of ascending neighbour order: the same f32 bits at 1, 10 and 20 iterations.
  Plane with in-plane jitter: z stays 0.25f bit for bit in all three boundary modes."""
import ctypes

import numpy as np
import pytest

import mesh_adjacency_ref as A
import mesh_simplify_ref as S
from asr_hip import _lib, ops, ply

NEW_EXPORTS = ("asr_hip_mesh_edges_count", "asr_hip_mesh_edges_fill", "asr_hip_mesh_topology", "asr_hip_mesh_smooth")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _radius(v):
    return np.sqrt((v.astype(np.float64) ** 2).sum(1))


# ---- the restatement on shapes with known answers -----------------------------------------------------------------
def test_sphere_is_a_closed_oriented_surface_of_genus_0():
    v, t = S.uv_sphere()
    edges, uses, forward = A.edge_table(t, len(v))
    assert len(v) == 1802 and edges.shape == (5400, 2) and len(t) == 3600
    assert (uses == 2).all() and (forward == 1).all() and (edges[:, 0] < edges[:, 1]).all()
    key = edges[:, 0].astype(np.int64) * len(v) + edges[:, 1]
    assert (np.diff(key) > 0).all()
    topo = A.topology(t, len(v))
    assert topo["euler"] == 2 and topo["watertight"] and topo["genus"] == 0 and topo["components"] == 1
    assert topo["used_vertices"] == 1802 and topo["boundary_loops"] == 0 and topo["edge_manifold"] and topo["oriented"]


def test_plane_with_a_hole():
    v, t = A.holed_plane()
    topo = A.topology(t, len(v))
    assert topo["boundary_edges"] == 152 and topo["nonmanifold_edges"] == 0
    assert topo["num_vertices"] - topo["used_vertices"] == 25
    assert topo["boundary_loops"] == 2 and topo["euler"] == 0 and topo["components"] == 1
    assert not topo["watertight"] and topo["genus"] is None and topo["edge_manifold"] and topo["oriented"]


def test_torus_two_spheres_and_the_crafted_meshes():
    v, t = A.torus()
    topo = A.topology(t, len(v))
    assert topo["euler"] == 0 and topo["watertight"] and topo["genus"] == 1
    v, t = A.two_spheres()
    topo = A.topology(t, len(v))
    assert topo["components"] == 2 and topo["euler"] == 4 and topo["watertight"] and topo["genus"] == 0
    v, t = A.three_on_one_edge()
    edges, uses, forward = A.edge_table(t, len(v))
    topo = A.topology(t, len(v))
    assert topo["nonmanifold_edges"] == 1 and not topo["edge_manifold"] and topo["boundary_edges"] == 6
    assert edges[uses == 3].tolist() == [[0, 1]] and forward[uses == 3].tolist() == [2]
    v, t = A.flipped_sphere()
    topo = A.topology(t, len(v))
    assert topo["inconsistent_edges"] == 3 and not topo["oriented"] and not topo["watertight"]
    assert topo["boundary_edges"] == 0 and topo["euler"] == 2
    v, t = A.duplicate_and_degenerate()
    topo = A.topology(t, len(v))
    assert topo["degenerate_triangles"] == 2 and topo["triangles"] == 3601 and topo["edges"] == 5400
    assert topo["nonmanifold_edges"] == 3 and topo["inconsistent_edges"] == 0 and topo["used_vertices"] == 1802
    v, t = A.renumbered_sphere()
    ref = A.topology(S.uv_sphere()[1], 1802)
    assert A.topology(t, len(v)) == ref
    # no triangles, one triangle, out of range
    assert A.edge_table(np.zeros((0, 3), np.int32), 7)[0].shape == (0, 2)
    topo = A.topology(np.zeros((0, 3), np.int32), 7)
    assert topo["num_vertices"] == 7 and topo["euler"] == 0 and topo["components"] == 0 and not topo["watertight"]
    edges, uses, forward = A.edge_table([[2, 0, 1]], 3)
    assert edges.tolist() == [[0, 1], [0, 2], [1, 2]] and uses.tolist() == [1, 1, 1] and forward.tolist() == [1, 0, 1]
    for bad in ([[0, 1, 3]], [[0, -1, 2]]):
        with pytest.raises(ValueError):
            A.edge_table(bad, 3)


def test_fans_have_rows_on_both_sides_of_the_cut():
    v, t = A.fans_around_the_cut()
    src, dst, _ = A.neighbour_rows(t, len(v))
    rows = np.bincount(src, minlength=len(v))
    for n in (A.SMOOTH_CUT - 1, A.SMOOTH_CUT, A.SMOOTH_CUT + 1, 5000):
        assert (rows == n).sum() == 1, n
    assert (rows == 0).sum() == 3 and (np.diff(src * len(v) + dst) > 0).all()


# ---- smoothing properties of the restatement ------------------------------------------------------------------------
def test_taubin_removes_noise_and_keeps_the_size():
    v, t = A.noisy_sphere()
    rms = lambda x: float(np.sqrt(((_radius(x) - 1) ** 2).mean()))  # noqa: E731
    taubin = A.smooth(v, t, 10)
    laplace = A.smooth(v, t, 10, mu=0.0)
    print("rms %.4f -> %.4f; mean radius %.4f (Taubin) %.4f (Laplacian)"
          % (rms(v), rms(taubin), _radius(taubin).mean(), _radius(laplace).mean()))
    assert rms(taubin) < rms(v)
    assert abs(_radius(taubin).mean() - 1) < abs(_radius(laplace).mean() - 1)
    for it in (1, 10, 20):
        assert np.array_equal(_bits(A.smooth(v, t, it)), _bits(A.smooth(v, t, it, descending=True)))
    assert np.array_equal(_bits(A.smooth(v, t, 0)), _bits(v))


def test_planarity_and_the_boundary_modes():
    v, t = A.jittered_holed_plane()
    edges, uses, _ = A.edge_table(t, len(v))
    rim = np.zeros(len(v), bool)
    rim[edges[uses == 1].reshape(-1)] = True
    unused = np.ones(len(v), bool)
    unused[t.reshape(-1)] = False
    out = {}
    for mode in A.BOUNDARY_MODES:
        out[mode] = A.smooth(v, t, 10, boundary=mode)
        assert np.all(out[mode][:, 2] == np.float32(0.25)), mode
        assert np.array_equal(_bits(out[mode][unused]), _bits(v[unused])), mode
    assert np.array_equal(_bits(out["pinned"][rim]), _bits(v[rim]))
    assert not np.array_equal(_bits(out["free"][rim]), _bits(v[rim]))
    assert not np.array_equal(_bits(out["along"][rim]), _bits(v[rim]))
    # "along": a rim vertex on a straight side stays on that side's line, "free" pulls it inwards
    side = rim & (v[:, 0] < -0.45) & (np.abs(v[:, 1]) < 0.4)
    spread = lambda a: float(a[side, 0].astype(np.float64).std())  # noqa: E731
    assert spread(out["along"]) <= spread(v) and out["free"][side, 0].mean() > v[side, 0].mean()
    with pytest.raises(ValueError):
        A.smooth(np.where(np.arange(len(v))[:, None] == 5, np.nan, v), t, 1)


# ---- these fail without the feature and need no GPU --------------------------------------------------------------------
def test_library_has_the_new_exports_and_the_struct():
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert lib.asr_hip_struct_size(b"asr_mesh_topology") == 8 * 11 == ctypes.sizeof(_lib.MeshTopology)


def test_smooth_arguments_are_checked_before_the_device():
    """CPU tensors: the argument errors must come first (a good call would fail on the tensors' device)"""
    import torch
    v, t = S.uv_sphere()
    tv, tt = torch.from_numpy(v), torch.from_numpy(t)
    for kw in (dict(lam=0), dict(lam=1.5), dict(lam=float("nan")), dict(mu=0.1), dict(mu=float("-inf")), dict(mu=float("nan")),
               dict(iterations=-1), dict(iterations=1001), dict(iterations=2.5), dict(boundary="nope"), dict(boundary=1)):
        with pytest.raises(ValueError):
            ops.mesh_smooth(tv, tt, **kw)
    with pytest.raises(_lib.AsrHipError, match="GPU tensor"):
        ops.mesh_smooth(tv, tt)
    summary = ops.topology_summary({k: v for k, v in A.topology(t, len(v)).items() if isinstance(v, int) and not isinstance(v, bool)})
    assert summary == A.topology(t, len(v))


def test_reconstruct_surface_refuses_a_negative_smooth_before_the_gpu():
    import adaptivesurfacereconstruction as asr
    v, _ = S.uv_sphere()
    for bad in (-1, 1001):
        with pytest.raises(ValueError, match="smooth"):
            asr.reconstruct_surface(v, v, weights={}, smooth=bad)
    with pytest.raises(ValueError):
        asr.smooth_mesh(v, S.uv_sphere()[1], boundary="nope")
    with pytest.raises(ValueError):
        asr.smooth_mesh(v, S.uv_sphere()[1], lam=0.0)


def test_asrtool_refuses_bad_smooth_and_topology_arguments(tmp_path, capsys):
    """exit status 1 and a message, before any GPU work (this test runs without a GPU)"""
    import asrtool
    v, t = S.plane_mesh()
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    ply.write_mesh(a, v, t)
    cloud = str(tmp_path / "c.ply")
    ply.write_points(cloud, v, np.tile(np.float32([0, 0, 1]), (len(v), 1)))
    cases = [
        (["--smooth-mesh", a], "two files"),
        (["--smooth-mesh", a, "--iterations", "3"], "two files"),
        (["--smooth-mesh", a, b, "--boundary", "nope"], "--boundary"),
        (["--smooth-mesh", a, b, "--boundary"], "--boundary"),
        (["--smooth-mesh", a, b, "--iterations", "-1"], "--iterations"),
        (["--smooth-mesh", a, b, "--iterations", "many"], "--iterations"),
        (["--smooth-mesh", a, b, "--iterations", "1001"], "--iterations"),
        (["--smooth-mesh", str(tmp_path / "missing.ply"), b], "no such file"),
        (["--smooth-mesh", cloud, b], "cannot read"),
        (["--topology", str(tmp_path / "missing.ply")], "no such file"),
        (["--topology"], "needs a file"),
        (["--topology", cloud], "cannot read"),
        (["--in", cloud, "--out", b, "--smooth"], "--smooth"),
        (["--in", cloud, "--out", b, "--smooth", "0"], "--smooth"),
        (["--in", cloud, "--out", b, "--smooth", "-2"], "--smooth"),
        (["--in", cloud, "--out", b, "--smooth", "lots"], "--smooth"),
    ]
    for argv, word in cases:
        assert asrtool.main(list(argv)) == 1, argv
        err = capsys.readouterr().err
        assert err.startswith("asrtool: ") and word in err, (argv, err)
    assert not (tmp_path / "b.ply").exists()
    assert "--smooth-mesh" in asrtool.HELP and "--topology" in asrtool.HELP and "--smooth N" in asrtool.HELP
