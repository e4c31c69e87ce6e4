"""Mesh simplification without a GPU: the numpy float64 restatement of the contract (tests/mesh_simplify_ref.py, the
yardstick of tests/test_gpu_mesh_simplify.py) has the properties the feature is built for, asrtool refuses bad
--simplify / --decimate arguments before any GPU work, and colours follow a vertex_map on the host.

Measured with the restatement (the GPU test's property bounds stay well inside these):
  UV sphere 30 x 60 (1 802 vertices, 3 600 triangles), frame over [-1.3,-1.2,-1.25]..[1.3,1.2,1.35]:
    level  cell size h  vertices  triangles  smallest radius (quadric)  (plain mean)
      3      0.325         152       300        1 - 2.8e-8                0.9875
      4      0.1625        552      1100        1 - 2.8e-8                0.9960
      5      0.08125      1372      2740        1 - 3.7e-8                0.9983
     21                   1802      3600        every vertex keeps its bits
    summing the corners in a random order changes no output bit at levels 3, 4 and 5.
  33 x 33 grid in the plane z = 0.25, frame over [-0.65, 0.65]^3, level 3: every output z is exactly 0.25f.
  65 x 65 roof z = 0.25 - |x - 3/32| (the crease on a grid line), same frame, level 3 (h = 0.1625): largest vertical
    distance of an output vertex from the roof 1.2e-4 h with the quadric, 0.19 h with the plain mean."""
import numpy as np
import pytest

import mesh_simplify_ref as R
from asr_hip import _lib, ply


@pytest.fixture(scope="module")
def sphere():
    v, t = R.uv_sphere()
    assert v.shape == (1802, 3) and t.shape == (3600, 3)
    return _lib.frame_init(*R.SPHERE_BOX), v, t


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("level,nv,nt,mean_radius", [(3, 152, 300, 0.9875), (4, 552, 1100, 0.9960), (5, 1372, 2740, 0.9983)])
def test_sphere_sizes_radius_and_order_independence(sphere, level, nv, nt, mean_radius):
    frame, v, t = sphere
    vo, to, vm = R.simplify(frame, v, t, level=level)
    assert vo.shape == (nv, 3) and to.shape == (nt, 3) and vm.shape == (len(v),)
    assert to.min() == 0 and to.max() == nv - 1 and (vm >= 0).all() and vm.max() == nv - 1
    radius = np.sqrt((vo.astype(np.float64) ** 2).sum(1))
    plain = R.simplify(frame, v, t, level=level, mean_only=True)[0]
    print("level %d: smallest radius %.9f (plain mean %.4f)" % (level, radius.min(), np.sqrt((plain.astype(np.float64) ** 2).sum(1)).min()))
    assert radius.min() >= 1 - 1e-7  # (the planes of an inscribed mesh meet on or outside the sphere)
    assert abs(np.sqrt((plain.astype(np.float64) ** 2).sum(1)).min() - mean_radius) < 1e-4
    # every output vertex lies in the cell its inputs lie in
    lo, hi = R.cluster_boxes(frame, v, np.full(len(v), level), vm, nv)
    tol = 2.0 ** -22 * np.maximum(np.abs(lo), np.abs(hi))
    assert np.all(vo >= lo - tol) and np.all(vo <= hi + tol)
    shuffled = R.simplify(frame, v, t, level=level, corner_order=np.random.default_rng(level).permutation(3 * len(t)))
    assert np.array_equal(_bits(shuffled[0]), _bits(vo)) and np.array_equal(shuffled[1], to)


def test_level_21_is_the_identity_and_level_0_is_empty(sphere):
    frame, v, t = sphere
    vo, to, vm = R.simplify(frame, v, t, level=21)
    # vertices in ascending key order: the map is a permutation, and through it everything is the input
    assert sorted(vm.tolist()) == list(range(len(v)))
    assert np.array_equal(_bits(vo[vm]), _bits(v)) and np.array_equal(to, vm[t])
    vo, to, vm = R.simplify(frame, v, t, level=0)
    assert vo.shape == (0, 3) and to.shape == (0, 3) and (vm == -1).all()
    # per-vertex levels: cells of different levels are different clusters
    lv = np.where(v[:, 2] > 0, 5, 3)
    vo, to, vm = R.simplify(frame, v, t, levels=lv)
    up, down = np.unique(vm[lv == 5]), np.unique(vm[lv == 3])
    assert len(np.intersect1d(up, down)) == 0 and len(up) + len(down) == len(vo)


def test_plane_and_roof():
    frame = _lib.frame_init(*R.GRID_BOX)
    h = float(frame.voxel_size[3])
    v, t = R.plane_mesh()
    vo, to, _ = R.simplify(frame, v, t, level=3)
    assert len(vo) > 16 and len(to) > 16 and np.all(vo[:, 2] == np.float32(0.25))
    v, t = R.roof_mesh()
    assert np.any(v[:, 0] == np.float32(R.ROOF_X))  # the crease is a grid line
    vo, to, _ = R.simplify(frame, v, t, level=3)
    quadric = R.roof_distance(vo).max() / h
    mean = R.roof_distance(R.simplify(frame, v, t, level=3, mean_only=True)[0]).max() / h
    print("roof: %d vertices, %d triangles, distance %.3g h (plain mean %.3g h)" % (len(vo), len(to), quadric, mean))
    assert quadric <= 1e-3 and mean > 0.05


def test_restatement_refuses_what_the_contract_refuses(sphere):
    frame, v, t = sphere
    bad_t = t.copy()
    bad_t[7, 1] = len(v)
    bad_v = v.copy()
    bad_v[3, 0] = np.nan
    far = v.copy()
    far[5] = [0, 0, 1e3]
    for kw in (dict(level=-1), dict(level=22), dict(), dict(level=3, levels=np.zeros(len(v))), dict(levels=np.zeros(5)),
               dict(levels=np.full(len(v), 22))):
        with pytest.raises(ValueError):
            R.simplify(frame, v, t, **kw)
    for vv, tt in ((v, bad_t), (v, -t), (bad_v, t), (far, t), (v[:0], t)):
        with pytest.raises(ValueError):
            R.simplify(frame, vv, tt, level=3)
    for vv, tt in ((v[:0], t[:0]), (v, t[:0])):
        vo, to, vm = R.simplify(frame, vv, tt, level=3)
        assert len(vo) == 0 and len(to) == 0 and len(vm) == len(vv) and (vm == -1).all()


def test_asrtool_refuses_bad_simplify_and_decimate_arguments(tmp_path, capsys):
    """exit status 1 and a message, before any GPU work (this test runs without a GPU)"""
    import asrtool
    v, t = R.plane_mesh()
    mesh = str(tmp_path / "m.ply")
    ply.write_mesh(mesh, v, t)
    out = str(tmp_path / "o.ply")
    cloud = str(tmp_path / "c.ply")
    ply.write_points(cloud, v, np.tile(np.float32([0, 0, 1]), (len(v), 1)))
    cases = [
        (["--in", cloud, "--out", out, "--simplify"], "--simplify"),
        (["--in", cloud, "--out", out, "--simplify", "two"], "--simplify"),
        (["--in", cloud, "--out", out, "--simplify", "0"], "--simplify"),
        (["--in", cloud, "--out", out, "--simplify", "-1"], "--simplify"),
        (["--in", cloud, "--out", out, "--simplify", "1.5"], "--simplify"),
        (["--in", cloud, "--out", out, "--simplify", "22"], "--simplify"),
        (["--decimate", mesh], "two files"),
        (["--decimate", mesh, "--cell", "0.1"], "two files"),
        (["--decimate", mesh, out], "--cell"),
        (["--decimate", mesh, out, "--cell"], "--cell"),
        (["--decimate", mesh, out, "--cell", "big"], "--cell"),
        (["--decimate", mesh, out, "--cell", "0"], "--cell"),
        (["--decimate", mesh, out, "--cell", "-0.1"], "--cell"),
        (["--decimate", mesh, out, "--cell", "nan"], "--cell"),
        (["--decimate", mesh, out, "--cell", "inf"], "--cell"),
        (["--decimate", str(tmp_path / "none.ply"), out, "--cell", "0.1"], "no such file"),
        (["--decimate", cloud, out, "--cell", "0.1"], "cannot read"),
        (["--in", cloud, "--out", out, "--precision", "f8"], "precision"),
        (["--in", cloud, "--out", out, "--colors"], "--colors"),
    ]
    for argv, word in cases:
        assert asrtool.main(list(argv)) == 1, argv
        err = capsys.readouterr().err
        assert err.startswith("asrtool: ") and word in err, (argv, err)
    assert not (tmp_path / "o.ply").exists()


def test_colours_follow_a_vertex_map(tmp_path):
    col = np.array([[10, 20, 30], [20, 40, 31], [0, 0, 0], [255, 255, 255], [255, 254, 0], [7, 7, 7]], np.uint8)
    vmap = np.array([1, 1, -1, 0, 0, 2])
    out = ply.average_colors(col, vmap, 4)
    # means 15 30 30.5 / 255 254.5 127.5 / 7 7 7 / nothing; round half to even
    assert out.dtype == np.uint8 and out.tolist() == [[255, 254, 128], [15, 30, 30], [7, 7, 7], [0, 0, 0]]
    with pytest.raises(ValueError):
        ply.average_colors(col, vmap, 2)
    with pytest.raises(ValueError):
        ply.average_colors(col[:5], vmap, 4)
    with pytest.raises(ValueError):
        ply.average_colors(col.astype(np.float32), vmap, 4)
    # through a simplification and a PLY file: a colour that depends on x alone stays within the cell's range of it
    frame = _lib.frame_init(*R.GRID_BOX)
    v, t = R.plane_mesh()
    vo, to, vm = R.simplify(frame, v, t, level=3)
    col = np.stack([np.rint((v[:, 0] + 0.5) * 255), np.full(len(v), 90), np.zeros(len(v))], 1).astype(np.uint8)
    out = ply.average_colors(col, vm, len(vo))
    for o in range(len(vo)):
        members = col[vm == o, 0]
        assert members.min() <= out[o, 0] <= members.max()
    assert np.all(out[:, 1] == 90) and np.all(out[:, 2] == 0)
    path = str(tmp_path / "s.ply")
    ply.write_mesh(path, vo, to, colors=out)
    v2, t2, c2 = ply.read_mesh(path, with_colors=True)
    assert np.array_equal(v2, vo) and np.array_equal(t2, to) and np.array_equal(c2, out)
