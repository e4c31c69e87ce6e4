"""Hole filling without a GPU: the numpy restatement of asr_hip_mesh_fill_holes_* (tests/mesh_fill_ref.py, the yardstick
of tests/test_gpu_mesh_fill_holes.py) on shapes with known answers, the new exports and the struct size in the built
library, and the argument checks that must come before any GPU work.

Known answers:
  tetrahedron without a face: one rim of 3 edges -> one triangle, no hub; closed, genus 0.
  cube without its top: one rim of 4 edges -> a hub at the top's centre and 4 triangles; closed, genus 0.
  tube of 4 rings of 12: two rims of 12 edges -> 2 hubs, 24 triangles; closed, genus 0.
  33 x 33 plane with the hole of tests/mesh_adjacency_ref.py: the hole has 24 edges, the border 128; a cap in 24..127
    fills the hole alone and leaves a disc (euler 1, one loop of 128 edges).
  two square holes that share a corner are ONE rim of 8 edges through a vertex that is left twice: not simple.
  a triangle turned over on the hole's rim: a rim vertex is entered twice and never left: not simple."""
import ctypes

import numpy as np
import pytest

import mesh_adjacency_ref as A
import mesh_fill_ref as F
import mesh_simplify_ref as S
from asr_hip import _lib, ops, ply

NEW_EXPORTS = ("asr_hip_mesh_fill_holes_count", "asr_hip_mesh_fill_holes_fill")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _fill(v, t, max_edges):
    """the restatement, with the properties every result has -> (v2, t2, report, topology before, topology after)"""
    before = A.topology(t, len(v))
    v2, t2, rep = F.fill_holes(v, t, max_edges)
    after = A.topology(t2, len(v2))
    assert v2.dtype == np.float32 and t2.dtype == np.int32
    assert np.array_equal(_bits(v2[:len(v)]), _bits(v)) and np.array_equal(t2[:len(t)], t)
    assert len(v2) == len(v) + rep["new_vertices"] and len(t2) == len(t) + rep["new_triangles"]
    assert rep["rims"] == before["boundary_loops"] == rep["filled"] + rep["too_long"] + rep["not_simple"]
    assert after["euler"] == before["euler"] + rep["filled"]
    assert after["boundary_loops"] == before["boundary_loops"] - rep["filled"]
    assert after["inconsistent_edges"] == before["inconsistent_edges"] and after["nonmanifold_edges"] == before["nonmanifold_edges"]
    return v2, t2, rep, before, after


def test_open_tetrahedron_gets_one_triangle_and_no_hub():
    v, t = F.open_tetrahedron()
    v2, t2, rep, _, after = _fill(v, t, 3)
    assert rep == dict(rims=1, filled=1, too_long=0, not_simple=0, new_vertices=0, new_triangles=1)
    assert t2[-1].tolist() == [0, 2, 1]  # m = 0, p -> m is 2 -> 0, m -> s is 0 -> 1
    assert after["watertight"] and after["genus"] == 0 and after["euler"] == 2 and after["triangles"] == 4


def test_open_cube_gets_a_hub_at_the_centre_of_its_top():
    v, t = F.open_cube()
    v2, t2, rep, before, after = _fill(v, t, 4)
    assert before["oriented"] and before["boundary_edges"] == 4
    assert rep == dict(rims=1, filled=1, too_long=0, not_simple=0, new_vertices=1, new_triangles=4)
    assert v2[8].tolist() == [0.5, 0.5, 1.0]
    assert t2[-4:, 1].tolist() == [4, 5, 6, 7] and (t2[-4:, 2] == 8).all()  # ascending tail, (b, a, hub)
    assert after["watertight"] and after["genus"] == 0 and after["euler"] == 2
    # one below the rim's length: nothing happens
    v3, t3, rep3, _, _ = _fill(v, t, 3)
    assert rep3 == dict(rims=1, filled=0, too_long=1, not_simple=0, new_vertices=0, new_triangles=0)
    assert len(v3) == len(v) and np.array_equal(t3, t)


def test_open_cylinder_closes_at_both_ends():
    v, t = F.open_cylinder()
    v2, t2, rep, before, after = _fill(v, t, 12)
    assert before["boundary_loops"] == 2 and before["euler"] == 0
    assert rep == dict(rims=2, filled=2, too_long=0, not_simple=0, new_vertices=2, new_triangles=24)
    assert after["watertight"] and after["genus"] == 0
    assert np.allclose(v2[-2:], [[0, 0, 0], [0, 0, 1.5]], atol=1e-6)  # rim ids 0 and 36: the bottom ring, then the top
    assert _fill(v, t, 11)[2]["too_long"] == 2


def test_holed_plane_with_a_cap_between_the_hole_and_the_border():
    v, t = A.holed_plane()
    for cap in (24, 127):
        v2, t2, rep, _, after = _fill(v, t, cap)
        assert rep == dict(rims=2, filled=1, too_long=1, not_simple=0, new_vertices=1, new_triangles=24)
        assert after["boundary_loops"] == 1 and after["boundary_edges"] == 128 and after["euler"] == 1 and not after["watertight"]
        assert np.allclose(v2[-1], [0, 0, 0.25], atol=1e-6)
    assert _fill(v, t, 23)[2]["filled"] == 0
    _, _, rep, _, after = _fill(v, t, 128)  # the border too: a closed (flat) surface
    assert rep["filled"] == 2 and after["watertight"] and after["genus"] == 0


def test_bow_tie_and_flipped_rim_are_not_simple_and_untouched():
    v, t = F.bow_tie()
    v2, t2, rep, before, _ = _fill(v, t, 8)
    assert before["boundary_loops"] == 2 and before["boundary_edges"] == 28
    assert rep == dict(rims=2, filled=0, too_long=1, not_simple=1, new_vertices=0, new_triangles=0)
    assert np.array_equal(t2, t) and len(v2) == len(v)
    assert _fill(v, t, 3)[2]["not_simple"] == 1  # whatever its length
    v, t = F.flipped_rim_plane()
    v2, t2, rep, before, _ = _fill(v, t, 127)
    assert before["inconsistent_edges"] == 2 and before["boundary_edges"] == 152
    assert rep == dict(rims=2, filled=0, too_long=1, not_simple=1, new_vertices=0, new_triangles=0)
    assert np.array_equal(t2, t)


def test_disks_on_both_sides_of_the_summation_cut():
    v, t = F.disks_around_the_cut()
    v2, t2, rep, _, after = _fill(v, t, 200)
    assert rep == dict(rims=4, filled=4, too_long=0, not_simple=0, new_vertices=4, new_triangles=127 + 128 + 129 + 200)
    assert after["watertight"] and after["components"] == 4
    # the long shape and a sequential sum agree to a rounding of the f32 result
    rims = [np.arange(b + 1, b + 1 + n) for b, n in zip(np.cumsum([0, 128, 129, 130]), (127, 128, 129, 200))]
    for hub, rim in zip(v2[-4:], rims):
        seq = (v[rim].astype(np.float64).sum(0) / len(rim)).astype(np.float32)
        assert np.all(np.abs(hub.astype(np.float64) - seq) <= 2.0 ** -22 * np.abs(v[rim]).max())
    assert _fill(v, t, 128)[2] == dict(rims=4, filled=2, too_long=2, not_simple=0, new_vertices=2, new_triangles=255)


def test_renumbered_vertices_are_summed_and_emitted_in_ascending_index():
    v, t = F.renumbered_holes()
    v2, t2, rep, before, after = _fill(v, t, 12)
    assert before["used_vertices"] == len(v) - 9
    assert rep == dict(rims=3, filled=3, too_long=0, not_simple=0, new_vertices=3, new_triangles=28)
    assert after["watertight"] and after["components"] == 2
    new = t2[len(t):]
    hubs = new[:, 2]
    assert (np.diff(hubs) >= 0).all()
    for h in np.unique(hubs):
        tails = new[hubs == h, 1]
        assert (np.diff(tails) > 0).all()
    first = [new[hubs == h, 1][0] for h in np.unique(hubs)]
    assert first == sorted(first)  # ascending rim id = ascending smallest vertex
    assert set(_fill(v, t, 4)[2].items()) >= {("filled", 1), ("too_long", 2)}


def test_single_triangle_becomes_a_pillow_and_a_second_pass_fills_nothing():
    v, t = F.single_triangle()
    v2, t2, rep, _, after = _fill(v, t, 3)
    assert t2.tolist() == [[2, 0, 1], [0, 2, 1]] and rep["filled"] == 1 and after["watertight"] and after["euler"] == 2
    for make, cap in ((F.open_cube, 4), (A.holed_plane, 100), (F.bow_tie, 8), (A.fans_around_the_cut, 1 << 20)):
        v, t = make()
        v2, t2, rep, _, _ = _fill(v, t, cap)
        v3, t3, rep3, _, _ = _fill(v2, t2, cap)
        assert rep3["filled"] == 0 and rep3["rims"] == rep["rims"] - rep["filled"]
        assert np.array_equal(_bits(v3), _bits(v2)) and np.array_equal(t3, t2)


def test_restatement_errors_and_empty_inputs():
    v, t = F.open_cube()
    for bad in (2, (1 << 20) + 1, 0, -1, 4.5, True):
        with pytest.raises(ValueError, match="max_edges"):
            F.fill_holes(v, t, bad)
    worse = t.copy()
    worse[3, 1] = 8
    with pytest.raises(ValueError, match="out of range"):
        F.fill_holes(v, worse, 4)
    nan = v.copy()
    nan[5, 0] = np.nan  # on the rim
    with pytest.raises(ValueError, match="not finite"):
        F.fill_holes(nan, t, 4)
    assert F.fill_holes(nan, t, 3)[2]["filled"] == 0  # ... which is not filled
    nan = v.copy()
    nan[0, 2] = np.inf  # off the rim: never read
    v2, _, rep = F.fill_holes(nan, t, 4)
    assert rep["filled"] == 1 and np.array_equal(_bits(v2[:8]), _bits(nan)) and v2[8].tolist() == [0.5, 0.5, 1.0]
    v2, t2, rep = F.fill_holes(v, t[:0], 4)
    assert np.array_equal(v2, v) and t2.shape == (0, 3) and not any(rep.values())
    sv, st = S.uv_sphere()
    v2, t2, rep = F.fill_holes(sv, st, 1 << 20)
    assert np.array_equal(_bits(v2), _bits(sv)) and np.array_equal(t2, st) and not any(rep.values())


# ---- these fail without the feature and need no GPU --------------------------------------------------------------------
def test_library_has_the_new_exports_and_the_struct():
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert lib.asr_hip_struct_size(b"asr_mesh_fill_report") == 8 * 6 == ctypes.sizeof(_lib.MeshFillReport)
    assert tuple(name for name, _ in _lib.MeshFillReport._fields_) == F.REPORT_FIELDS


def test_fill_arguments_are_checked_before_the_device():
    """CPU tensors: the argument errors must come first (a good call would fail on the tensors' device)"""
    import torch
    import adaptivesurfacereconstruction as asr
    v, t = F.open_cube()
    tv, tt = torch.from_numpy(v), torch.from_numpy(t)
    for bad in (2, (1 << 20) + 1, 0, -3, 4.5, True):
        with pytest.raises(ValueError, match="max_edges"):
            ops.mesh_fill_holes(tv, tt, bad)
        with pytest.raises(ValueError, match="max_edges"):
            asr.fill_mesh_holes(v, t, bad)
    assert ops.check_fill_arguments(3) == 3 and ops.check_fill_arguments(1 << 20) == 1 << 20
    with pytest.raises(_lib.AsrHipError, match="GPU tensor"):
        ops.mesh_fill_holes(tv, tt, 4)
    for bad in (2, -1, (1 << 20) + 1):
        with pytest.raises(ValueError, match="max_edges"):
            asr.reconstruct_surface(v, v, weights={}, fill_holes=bad)
    with pytest.raises(ValueError):
        asr.fill_mesh_holes(v, t.reshape(-1), 4)


def test_hub_attributes_are_the_mean_of_the_rim():
    v, t = F.open_cube()
    v2, t2, _ = F.fill_holes(v, t, 4)
    col = (np.arange(24).reshape(8, 3) * 10).astype(np.uint8)
    got = ply.hub_attributes(col, t2, 8, 9)
    assert got.dtype == np.uint8 and np.array_equal(got[:8], col) and got[8].tolist() == [165, 175, 185]
    nrm = np.tile(np.float32([0, 0, 1]), (8, 1))
    nrm[4] = [1, 0, 0]
    got = ply.hub_attributes(nrm, t2, 8, 9)
    assert got.dtype == np.float32 and got[8].tolist() == [0.25, 0.0, 0.75]
    tv, tt = F.open_tetrahedron()  # no hub: nothing is added
    assert np.array_equal(ply.hub_attributes(col[:4], F.fill_holes(tv, tt, 3)[1], 4, 4), col[:4])


def test_asrtool_refuses_bad_fill_arguments(tmp_path, capsys):
    """exit status 1 and a message, before any GPU work (this test runs without a GPU)"""
    import asrtool
    v, t = F.open_cube()
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    ply.write_mesh(a, v, t)
    cloud = str(tmp_path / "c.ply")
    ply.write_points(cloud, v, np.tile(np.float32([0, 0, 1]), (len(v), 1)))
    cases = [
        (["--fill-mesh", a], "two files"),
        (["--fill-mesh", a, "--max-edges", "8"], "two files"),
        (["--fill-mesh", a, b], "--max-edges"),
        (["--fill-mesh", a, b, "--max-edges"], "--max-edges"),
        (["--fill-mesh", a, b, "--max-edges", "2"], "--max-edges"),
        (["--fill-mesh", a, b, "--max-edges", "1048577"], "--max-edges"),
        (["--fill-mesh", a, b, "--max-edges", "few"], "--max-edges"),
        (["--fill-mesh", str(tmp_path / "missing.ply"), b, "--max-edges", "8"], "no such file"),
        (["--fill-mesh", cloud, b, "--max-edges", "8"], "cannot read"),
        (["--in", cloud, "--out", b, "--fill-holes"], "--fill-holes"),
        (["--in", cloud, "--out", b, "--fill-holes", "0"], "--fill-holes"),
        (["--in", cloud, "--out", b, "--fill-holes", "2"], "--fill-holes"),
        (["--in", cloud, "--out", b, "--fill-holes", "1048577"], "--fill-holes"),
        (["--in", cloud, "--out", b, "--fill-holes", "all"], "--fill-holes"),
    ]
    for argv, word in cases:
        assert asrtool.main(list(argv)) == 1, argv
        err = capsys.readouterr().err
        assert err.startswith("asrtool: ") and word in err, (argv, err)
    assert not (tmp_path / "b.ply").exists()
    assert "--fill-mesh" in asrtool.HELP and "--fill-holes N" in asrtool.HELP and "--max-edges N" in asrtool.HELP
    assert asrtool.HELP.startswith("usage: asrtool --in point_cloud.ply --out mesh.ply")
