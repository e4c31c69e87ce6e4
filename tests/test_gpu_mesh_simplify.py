"""GPU tests of mesh simplification (asr_hip_mesh_simplify_count / _fill) against the numpy float64
restatement of its contract (tests/mesh_simplify_ref.py; what that restatement itself achieves is recorded and checked in
tests/test_mesh_simplify.py), and of its users: ImplicitPipeline.mesh(simplify=), reconstruct_surface(simplify=),
simplify_mesh and asrtool --decimate.

Structure (triangles, vertex_map, sizes) must equal the restatement exactly.  Positions, per component:
    |got - ref| <= 2^-22 * max(|coordinate|, h)
The 3x3 system is solved in f64 and has a condition number of at most about 3e3 (eps = 1e-3 tr(A) / 3), so its error
(1e-16 * 3e3 relative to h) can only flip the final rounding to f32; the bound is four half-ulps of the larger of the
coordinate and the cell size."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_simplify_ref as R
from asr_hip import _lib, ops, ply, synth
from asr_hip._lib import AsrHipError
from asr_hip.pipeline import ImplicitPipeline

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "adaptive-surface-reconstruction_amd", "asrtool.py")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _run(gpu, frame, v, t, level=None, levels=None):
    """the op, twice (the same bits on every run) -> numpy (vertices, triangles, vertex_map)"""
    tv, tt = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(gpu), torch.from_numpy(np.ascontiguousarray(t, np.int32)).to(gpu)
    tl = None if levels is None else torch.from_numpy(np.asarray(levels, np.int8)).to(gpu)
    a = ops.mesh_simplify(frame, tv, tt, level=level, levels=tl, return_map=True)
    b = ops.mesh_simplify(frame, tv, tt, level=level, levels=tl, return_map=True)
    assert a[0].dtype == torch.float32 and a[1].dtype == torch.int32 and a[2].dtype == torch.int32
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
    two = ops.mesh_simplify(frame, tv, tt, level=level, levels=tl)
    assert len(two) == 2 and torch.equal(two[0].view(torch.int32), a[0].view(torch.int32)) and torch.equal(two[1], a[1])
    return tuple(x.cpu().numpy() for x in a)


def _check(gpu, frame, v, t, what, level=None, levels=None):
    """the op against the restatement -> (got, ref)"""
    got = _run(gpu, frame, v, t, level, levels)
    ref = R.simplify(frame, v, t, level=level, levels=levels)
    assert got[0].shape == ref[0].shape and got[1].shape == ref[1].shape and got[2].shape == ref[2].shape, what
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), what
    lv = np.full(len(v), level, np.int64) if levels is None else np.asarray(levels, np.int64)
    vs = np.array(frame.voxel_size[:], np.float64)
    h = np.zeros(len(ref[0]))
    h[ref[2][ref[2] >= 0]] = vs[lv[ref[2] >= 0]]
    diff = np.abs(got[0].astype(np.float64) - ref[0].astype(np.float64))
    bound = 2.0 ** -22 * np.maximum(np.abs(ref[0].astype(np.float64)), h[:, None])
    print("%s: %d -> %d vertices, %d -> %d triangles, max |got - ref| = %.3g, largest share of the bound %.3g, %d of %d "
          "coordinates differ" % (what, len(v), len(got[0]), len(t), len(got[1]), diff.max() if diff.size else 0,
                                  (diff / bound).max() if diff.size else 0, int((diff > 0).sum()), diff.size))
    assert np.all(diff <= bound), what
    # every output vertex lies in the box of its cell
    lo, hi = R.cluster_boxes(frame, v, lv, ref[2], len(ref[0]))
    tol = 2.0 ** -22 * np.maximum(np.abs(lo), np.abs(hi))
    assert np.all(got[0] >= lo - tol) and np.all(got[0] <= hi + tol), what
    return got, ref


@pytest.fixture(scope="module")
def sphere():
    v, t = R.uv_sphere()
    return _lib.frame_init(*R.SPHERE_BOX), v, t


# ---- 1. exact structure and the properties the restatement stays within --------------------------------------------
@pytest.mark.parametrize("level,nv,nt", [(3, 152, 300), (4, 552, 1100), (5, 1372, 2740)])
def test_sphere_equals_the_restatement(gpu, sphere, level, nv, nt):
    frame, v, t = sphere
    got, _ = _check(gpu, frame, v, t, "sphere level %d" % level, level=level)
    assert got[0].shape == (nv, 3) and got[1].shape == (nt, 3)
    radius = np.sqrt((got[0].astype(np.float64) ** 2).sum(1))
    print("sphere level %d: smallest radius %.9f" % (level, radius.min()))
    if level in (3, 4):
        assert radius.min() >= 0.9999


def test_per_vertex_levels(gpu, sphere):
    frame, v, t = sphere
    lv = np.where(v[:, 2] > 0, 5, 3)
    got, _ = _check(gpu, frame, v, t, "sphere levels 5 / 3", levels=lv)
    up, down = np.unique(got[2][lv == 5]), np.unique(got[2][lv == 3])
    assert len(np.intersect1d(up, down)) == 0 and len(up) + len(down) == len(got[0])


def test_plane_and_roof(gpu):
    frame = _lib.frame_init(*R.GRID_BOX)
    h = float(frame.voxel_size[3])
    v, t = R.plane_mesh()
    got, _ = _check(gpu, frame, v, t, "plane level 3", level=3)
    assert len(got[0]) > 16 and np.all(got[0][:, 2] == np.float32(0.25))
    v, t = R.roof_mesh()
    got, _ = _check(gpu, frame, v, t, "roof level 3", level=3)
    dist = R.roof_distance(got[0]).max() / h
    print("roof level 3: largest distance from the roof %.3g h" % dist)
    assert dist <= 1e-3
    _check(gpu, frame, v, t, "roof level 4", level=4)  # (clusters limited by the clamp: no crease bound here)


# ---- 2. sizes where a kernel can go wrong ---------------------------------------------------------------------------
def test_level_0_one_cluster_and_level_21_all_singletons(gpu, sphere):
    frame, v, t = sphere
    got = _run(gpu, frame, v, t, level=0)  # one cluster holding all 10 800 corners
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (len(v),) and (got[2] == -1).all()
    # level 21 with two vertices no triangle references: the rest keeps its bits
    v2 = np.concatenate([v[:100], [[0.5, 0.5, 0.5]], v[100:], [[-0.25, 0.125, 0.0]]]).astype(np.float32)
    t2 = np.where(t >= 100, t + 1, t).astype(np.int32)
    got, ref = _check(gpu, frame, v2, t2, "sphere level 21", level=21)
    vm = got[2]
    assert vm[100] == -1 and vm[-1] == -1 and len(got[0]) == len(v)
    used = vm >= 0
    assert sorted(vm[used].tolist()) == list(range(len(v)))
    assert np.array_equal(_bits(got[0][vm[used]]), _bits(v2[used])) and np.array_equal(got[1], vm[t2])
    assert np.array_equal(_bits(got[0]), _bits(ref[0]))


def _fan(hub, n_first, n_second, phase):
    """two vertices 0.01 apart (one cluster at level 3) with n_first and n_second triangles to a ring of radius 0.3"""
    n = max(n_first, n_second)
    th = 2 * np.pi * np.arange(n) / n + phase
    ring = hub + np.stack([0.3 * np.cos(th), 0.3 * np.sin(th), 0.1 * np.sin(3 * th) - 0.05], 1)
    v = np.concatenate([[hub, hub + 0.01], ring]).astype(np.float32)
    tri = [(0, 2 + i, 2 + (i + 1) % n) for i in range(n_first)] + [(1, 2 + i, 2 + (i + 1) % n) for i in range(n_second)]
    return v, np.array(tri, np.int32)


def test_clusters_of_64_and_65_corners(gpu):
    frame = _lib.frame_init(*R.GRID_BOX)
    va, ta = _fan(np.array([-0.3, -0.3, 0.0]), 63, 1, 0.1)   # 64 corners in the hub's cluster
    vb, tb = _fan(np.array([0.3, 0.3, 0.1]), 63, 2, 0.2)     # 65
    v = np.concatenate([va, vb, [[0.0, 0.6, -0.6]]]).astype(np.float32)  # ... and a vertex no triangle references
    t = np.concatenate([ta, tb + len(va)]).astype(np.int32)
    _, key = R.vertex_cells(frame, v, np.full(len(v), 3))
    assert key[0] == key[1] and key[len(va)] == key[len(va) + 1]
    corners = key[t.reshape(-1)]
    assert (corners == key[0]).sum() == 64 and (corners == key[len(va)]).sum() == 65
    got, _ = _check(gpu, frame, v, t, "fans of 64 and 65 corners", level=3)
    assert got[2][-1] == -1 and got[2][0] == got[2][1] >= 0


def test_duplicate_and_degenerate_triangles(gpu):
    frame = _lib.frame_init(*R.GRID_BOX)
    # four clusters at level 3 (h = 0.1625), two vertices each: x x' y y' z z' w w'
    base = np.array([[-0.40625, -0.40625, 0.0], [0.09375, -0.40625, 0.0625], [-0.1, 0.1, 0.4], [0.4, 0.3, -0.2]])
    v = np.repeat(base, 2, axis=0)
    v[1::2] += [0.02, 0.01, 0.015]
    x, y, z, w = 0, 2, 4, 6
    mid = len(v)
    v = np.concatenate([v, [(v[x] + v[y]) / 2], [[0.2, 0.2, 0.2]]]).astype(np.float32)
    v[mid] = (v[x].astype(np.float64) + v[y].astype(np.float64)) / 2  # exactly on the edge in f32: a triangle without area
    assert np.array_equal(v[mid].astype(np.float64) * 2, v[x].astype(np.float64) + v[y])
    t = np.array([
        (x, y, z),              # 0 survives
        (x, mid, y),            # 1 no area (three clusters all the same: x, mid's own, y -- survives as a triangle)
        (z + 1, y + 1, x + 1),  # 2 = 0 in the opposite orientation: dropped
        (w, y, z),              # 3 survives
        (z, w + 1, y + 1),      # 4 = 3
        (y + 1, z + 1, w),      # 5 = 3
        (x, x + 1, y),          # 6 two corners in one cluster: dropped
        (x, x, z),              # 7 two equal corners, no area: dropped
        (x, w, z),              # 8 survives
        (w + 1, x + 1, z),      # 9 = 8
    ], np.int32)
    _, key = R.vertex_cells(frame, v, np.full(len(v), 3))
    assert len(np.unique(key)) == 6 and all(key[i] == key[i + 1] for i in (x, y, z, w))
    got, ref = _check(gpu, frame, v, t, "duplicates", level=3)
    vm = got[2]
    assert np.array_equal(got[1], vm[t[[0, 1, 3, 8]]])  # the earlier one, with its own corner order, in input order
    assert vm[-1] == -1 and (vm[:-1] >= 0).all() and len(got[0]) == 5
    # three triangles with the same triple in the middle of a longer list, a fourth at its end
    sv, st = R.uv_sphere(6, 8)
    sv = (sv * 0.12 + [0.3, -0.3, 0.3]).astype(np.float32)
    t2 = np.concatenate([st[:40] + len(v), t[3:6], st[40:] + len(v), t[[4]]]).astype(np.int32)
    v2 = np.concatenate([v, sv]).astype(np.float32)
    got, _ = _check(gpu, frame, v2, t2, "duplicates in the middle", level=3)
    same = [i for i, tri in enumerate(got[1]) if sorted(tri) == sorted(got[2][[w, y, z]])]
    assert len(same) == 1 and np.array_equal(got[1][same[0]], got[2][t[3]])


def test_empty_inputs(gpu):
    frame = _lib.frame_init(*R.GRID_BOX)
    v, t = R.plane_mesh()
    for vv, tt in ((v[:0], t[:0]), (v, t[:0])):
        got = _run(gpu, frame, vv, tt, level=3)
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (len(vv),) and (got[2] == -1).all()
        got = _run(gpu, frame, vv, tt, levels=np.full(len(vv), 3))
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and (got[2] == -1).all()


# ---- 3. errors ----------------------------------------------------------------------------------------------------
def test_errors_and_a_good_call_afterwards(gpu, sphere):
    frame, v, t = sphere
    tv, tt = torch.from_numpy(v).to(gpu), torch.from_numpy(t).to(gpu)
    ctx = ops.context(gpu)

    def corrupt(a, where, value):
        a = a.clone()
        a[where] = value
        return a

    lv = torch.full((len(v),), 3, dtype=torch.int8, device=gpu)
    library = [
        (dict(triangles=corrupt(tt, (17, 1), -1), level=3), "out of range"),
        (dict(triangles=corrupt(tt, (3599, 2), len(v)), level=3), "out of range"),
        (dict(level=-1), "level"),
        (dict(level=22), "level"),
        (dict(levels=corrupt(lv, 5, -1)), "level"),
        (dict(levels=corrupt(lv, 1801, 22)), "level"),
        (dict(vertices=corrupt(tv, (7, 1), float("nan")), level=3), "outside the frame"),
        (dict(vertices=corrupt(tv, (7, 1), float("inf")), level=3), "outside the frame"),
        (dict(vertices=corrupt(tv, (1000, 2), 1.5), level=3), "outside the frame"),   # the cube ends at 1.35
        (dict(vertices=corrupt(tv, (0, 0), -1e30), levels=lv), "outside the frame"),
        (dict(vertices=tv[:0], level=3), "out of range"),                             # triangles without vertices
    ]
    for kw, word in library:
        args = dict(vertices=tv, triangles=tt)
        args.update(kw)
        with pytest.raises(AsrHipError, match=word):
            ops.mesh_simplify(frame, ctx=ctx, **args)
    for kw in (dict(vertices=tv.cpu(), level=3), dict(triangles=tt.cpu(), level=3), dict(levels=lv.cpu())):
        args = dict(vertices=tv, triangles=tt)
        args.update(kw)
        with pytest.raises(AsrHipError, match="GPU tensor"):
            ops.mesh_simplify(frame, ctx=ctx, **args)
    for kw in (dict(), dict(level=3, levels=lv), dict(levels=lv[:-1]), dict(levels=lv[:, None]),
               dict(vertices=tv[:, :2], level=3), dict(triangles=tt.reshape(-1), level=3), dict(vertices=tv.reshape(-1), level=3)):
        args = dict(vertices=tv, triangles=tt)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.mesh_simplify(frame, ctx=ctx, **args)
    # a fill without its count is refused, and the context still works
    with pytest.raises(AsrHipError, match="must follow"):
        ctx.call("asr_hip_mesh_simplify_fill", _lib.ptr(tv), _lib.ptr(tt), _lib.ptr(None))
    got = ops.mesh_simplify(frame, tv, tt, level=3, return_map=True, ctx=ctx)
    ref = R.simplify(frame, v, t, level=3)
    assert np.array_equal(got[1].cpu().numpy(), ref[1]) and np.array_equal(got[2].cpu().numpy(), ref[2])


# ---- 4. end to end ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(gpu):
    p, q = synth.scan_cloud(6000, seed=31, device="cpu")
    pts, nrm = p.numpy(), q.numpy()
    return pts, nrm, synth.knn_radii(pts, 24), synth.bounding_box(pts, 0.1), synth.make_weights(4, seed=31)


def _levels_by_hand(frame, pipe, v, k):
    keys = pipe.get("voxel_keys0")
    rows = ops.leaf_locate(frame, keys, v).cpu().numpy()
    leaf_level = np.array([(int(key).bit_length() - 1) // 3 for key in keys.cpu().numpy().view(np.uint64)])
    return np.where(rows >= 0, np.maximum(0, leaf_level[np.maximum(rows, 0)] - k), 21).astype(np.int8)


def test_pipeline_mesh_simplify(gpu, scene):
    pts, nrm, rad, bb, weights = scene
    pipe = ImplicitPipeline(weights, device=gpu)
    tp, tn, tr = (torch.from_numpy(a).to(gpu) for a in (pts, nrm, rad))
    pipe.forward(tp, tn, tr, *bb)
    v, t = pipe.mesh()
    v0, t0 = pipe.mesh(simplify=0)
    assert torch.equal(v0.view(torch.int32), v.view(torch.int32)) and torch.equal(t0, t) and len(t) > 500
    frame = _lib.frame_init(*bb)
    previous = len(t)
    for k in (1, 2):
        vk, tk = pipe.mesh(simplify=k)
        lv = _levels_by_hand(frame, pipe, v, k)
        assert np.array_equal(pipe.simplify_levels(v, k).cpu().numpy(), lv)
        want = ops.mesh_simplify(frame, v, t, levels=torch.from_numpy(lv).to(gpu))
        assert torch.equal(vk.view(torch.int32), want[0].view(torch.int32)) and torch.equal(tk, want[1])
        print("pipeline simplify=%d: %d -> %d vertices, %d -> %d triangles" % (k, len(v), len(vk), len(t), len(tk)))
        assert 0 < len(tk) < previous and len(vk) < len(v)
        previous = len(tk)
        _check(gpu, frame, v.cpu().numpy(), t.cpu().numpy(), "pipeline mesh k=%d" % k, levels=lv)
    with pytest.raises(ValueError):
        pipe.mesh(simplify=-1)


def test_reconstruct_surface_simplify(gpu, scene, tmp_path):
    import adaptivesurfacereconstruction as asr
    import asrtool
    pts, nrm, _, _, weights = scene
    plain = asr.reconstruct_surface(pts, nrm, weights=weights)
    zero = asr.reconstruct_surface(pts, nrm, weights=weights, simplify=0)
    assert sorted(zero) == sorted(plain) == ["triangles", "vertices"]
    assert np.array_equal(_bits(zero["vertices"]), _bits(plain["vertices"])) and np.array_equal(zero["triangles"], plain["triangles"])
    res = asr.reconstruct_surface(pts, nrm, weights=weights, simplify=1, vertex_normals=True, point_attributes=pts)
    n = len(res["vertices"])
    assert 0 < n < len(plain["vertices"]) and 0 < len(res["triangles"]) < len(plain["triangles"])
    assert res["vertex_normals"].shape == (n, 3) and res["vertex_attributes"].shape == (n, 3)
    assert res["triangles"].min() == 0 and res["triangles"].max() == n - 1
    with pytest.raises(ValueError):
        asr.reconstruct_surface(pts, nrm, weights=weights, simplify=-1)
    # asrtool --simplify is that call (in this process: the tool's own start is not what is tested)
    np.savez(str(tmp_path / "w.npz"), **weights)
    ply.write_points(str(tmp_path / "in.ply"), pts, nrm)
    assert asrtool.main(["--in", str(tmp_path / "in.ply"), "--out", str(tmp_path / "out.ply"), "--weights",
                         str(tmp_path / "w.npz"), "--simplify", "1", "--normals"]) == 0
    v, t, n = ply.read_mesh(str(tmp_path / "out.ply"), with_normals=True)
    assert np.array_equal(_bits(v), _bits(res["vertices"])) and np.array_equal(t, res["triangles"])
    assert np.array_equal(_bits(n), _bits(res["vertex_normals"]))


def test_simplify_mesh_and_asrtool_decimate(gpu, sphere, tmp_path):
    import adaptivesurfacereconstruction as asr
    _, v, t = sphere
    cell = 0.2
    res = asr.simplify_mesh(v, t, cell, return_map=True)
    # KDTree's margin, and the deepest level whose voxel size is >= cell
    lo, hi = v.min(0), v.max(0)
    m = max(1e-3, 1e-3 * float((hi - lo).max()))
    frame = _lib.frame_init(lo - np.float32(m), hi + np.float32(m))
    vs = np.array(frame.voxel_size[:])
    level = int(np.flatnonzero(vs >= cell).max())
    assert res["level"] == level and res["cell_size"] == float(vs[level]) and cell <= res["cell_size"] < 2 * cell
    want = _run(gpu, frame, v, t, level=level)
    assert np.array_equal(_bits(res["vertices"]), _bits(want[0])) and np.array_equal(res["triangles"], want[1])
    assert np.array_equal(res["vertex_map"], want[2]) and 0 < len(want[1]) < len(t)
    assert sorted(asr.simplify_mesh(v, t, cell)) == ["cell_size", "level", "triangles", "vertices"]
    assert asr.simplify_mesh(v, t, 100.0)["level"] == 0  # larger than the root cube: one cell, nothing left
    for wrong in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            asr.simplify_mesh(v, t, wrong)
    with pytest.raises(ValueError):
        asr.simplify_mesh(v[:0], t[:0], cell)
    # the command line, with colours
    col = np.stack([np.rint((v[:, 0] + 1) * 127), np.full(len(v), 90), np.rint((v[:, 2] + 1) * 100)], 1).astype(np.uint8)
    ply.write_mesh(str(tmp_path / "in.ply"), v, t, colors=col, normals=v)
    r = subprocess.run([sys.executable, TOOL, "--decimate", str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "--cell",
                        str(cell)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "%d -> %d vertices" % (len(v), len(want[0])) in r.stdout
    v2, t2, n2, c2 = ply.read_mesh(str(tmp_path / "out.ply"), with_normals=True, with_colors=True)
    assert np.array_equal(_bits(v2), _bits(want[0])) and np.array_equal(t2, want[1]) and n2 is None
    assert np.array_equal(c2, ply.average_colors(col, want[2], len(want[0]))) and np.all(c2[:, 1] == 90)
