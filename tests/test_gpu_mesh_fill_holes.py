"""GPU tests of asr_hip_mesh_fill_holes_count / _fill against the numpy restatement of their contract
(tests/mesh_fill_ref.py; what the restatement itself gives on shapes with known answers is checked in
tests/test_mesh_fill_holes.py), and of their users: ImplicitPipeline.mesh(fill_holes=), reconstruct_surface(fill_holes=),
fill_mesh_holes and the two asrtool forms.

Triangles, report and sizes are integers and must equal the restatement exactly; the input vertices must keep their bits.
Hub positions, per coordinate:
    |got - ref| <= 2^-22 * max |input coordinate|
the bound derived in the docstring of tests/test_gpu_mesh_adjacency.py: both sides sum in f64 and round once to f32, so
only a flipped final rounding, one ulp of a coordinate (at most 2^-23 of the largest), can differ; the bound is twice
that.  The hubs of rims of up to 128 vertices, which both sides sum sequentially, must agree bit for bit.  Every call
runs twice and must give the same bits."""
import json

import numpy as np
import pytest
import torch

import mesh_adjacency_ref as A
import mesh_fill_ref as F
from asr_hip import _lib, ops, ply, synth
from asr_hip._lib import AsrHipError
from asr_hip.pipeline import ImplicitPipeline
from stream_helpers import late
from test_gpu_mesh_adjacency import MESHES

pytestmark = pytest.mark.gpu

ALL = 1 << 20
MAKERS = dict(MESHES, **F.FILL_MESHES)
# (mesh, max_edges): every mesh with the largest cap; the caps one below / at a rim's length and the two sides of the cut
CASES = [(name, ALL) for name in MAKERS] + [
    ("open tetrahedron", 3), ("open cube", 3), ("open cube", 4), ("open cylinder", 11), ("open cylinder", 12),
    ("holed plane", 23), ("holed plane", 24), ("holed plane", 127), ("disks around the cut", 128),
    ("disks around the cut", 129), ("bow tie", 8), ("flipped rim", 127), ("renumbered holes", 4), ("fans", 128),
]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def meshes():
    return {name: make() for name, make in MAKERS.items()}


def _fill(gpu, v, t, cap, what):
    """the op twice (equal bits) -> (vertices, triangles, report) as numpy"""
    tv, tt = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(gpu), torch.from_numpy(np.ascontiguousarray(t, np.int32)).to(gpu)
    a = ops.mesh_fill_holes(tv, tt, cap, return_report=True)
    b = ops.mesh_fill_holes(tv, tt, cap, return_report=True)
    assert a[0].dtype == torch.float32 and a[1].dtype == torch.int32 and a[0].ndim == a[1].ndim == 2, what
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and a[2] == b[2], what
    assert torch.equal(tv.view(torch.int32), torch.from_numpy(_bits(v)).to(gpu)) and torch.equal(tt, torch.from_numpy(t).to(gpu))
    plain = ops.mesh_fill_holes(tv, tt, cap)
    assert len(plain) == 2 and torch.equal(plain[1], a[1])
    return a[0].cpu().numpy(), a[1].cpu().numpy(), a[2]


def _compare(v, t, got, ref, what):
    gv, gt, grep = got
    rv, rt, rrep = ref
    assert grep == rrep and all(type(x) is int for x in grep.values()), what
    assert gv.shape == rv.shape and gt.shape == rt.shape, what
    assert np.array_equal(gt, rt), what
    nv = len(v)
    assert np.array_equal(_bits(gv[:nv]), _bits(v)), what
    if len(gv) == nv:
        return
    length = np.bincount(rt[len(t):, 2][rt[len(t):, 2] >= nv] - nv, minlength=len(rv) - nv)  # rim length of every hub
    diff = np.abs(gv[nv:].astype(np.float64) - rv[nv:].astype(np.float64))
    bound = 2.0 ** -22 * float(np.abs(v).max())
    print("%s: %d hubs (%d of rims longer than %d), max |got - ref| = %.3g, share of the bound %.3g, %d coordinates differ"
          % (what, len(length), int((length > F.FILL_CUT).sum()), F.FILL_CUT, diff.max(), diff.max() / bound, int((diff > 0).sum())))
    assert np.all(diff <= bound), what
    short = length <= F.FILL_CUT
    assert np.array_equal(_bits(gv[nv:][short]), _bits(rv[nv:][short])), what


# ---- 1. the op against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cap", CASES, ids=["%s-%d" % c for c in CASES])
def test_fill_equals_the_restatement(gpu, meshes, name, cap):
    v, t = meshes[name]
    got = _fill(gpu, v, t, cap, name)
    _compare(v, t, got, F.fill_holes(v, t, cap), "%s, max_edges %d" % (name, cap))
    print(name, cap, got[2])
    topo = ops.mesh_topology(torch.from_numpy(got[1]).to(gpu), len(got[0]))
    assert topo == A.topology(got[1], len(got[0])), name
    before = A.topology(t, len(v))
    assert got[2]["rims"] == before["boundary_loops"] and topo["euler"] == before["euler"] + got[2]["filled"]


def test_fill_known_answers(gpu, meshes):
    for name, cap, want, watertight in (
            ("open tetrahedron", 3, dict(rims=1, filled=1, too_long=0, not_simple=0, new_vertices=0, new_triangles=1), True),
            ("open cube", 4, dict(rims=1, filled=1, too_long=0, not_simple=0, new_vertices=1, new_triangles=4), True),
            ("open cylinder", 12, dict(rims=2, filled=2, too_long=0, not_simple=0, new_vertices=2, new_triangles=24), True),
            ("holed plane", 100, dict(rims=2, filled=1, too_long=1, not_simple=0, new_vertices=1, new_triangles=24), False),
            ("bow tie", 8, dict(rims=2, filled=0, too_long=1, not_simple=1, new_vertices=0, new_triangles=0), False),
            ("flipped rim", 127, dict(rims=2, filled=0, too_long=1, not_simple=1, new_vertices=0, new_triangles=0), False),
            ("single triangle", 3, dict(rims=1, filled=1, too_long=0, not_simple=0, new_vertices=0, new_triangles=1), True),
            ("sphere", ALL, dict.fromkeys(F.REPORT_FIELDS, 0), True),
            ("no triangles", ALL, dict.fromkeys(F.REPORT_FIELDS, 0), False)):
        v, t = meshes[name]
        gv, gt, rep = _fill(gpu, v, t, cap, name)
        assert rep == want, name
        assert ops.mesh_topology(torch.from_numpy(gt).to(gpu), len(gv))["watertight"] == watertight, name
        if not rep["filled"]:
            assert np.array_equal(_bits(gv), _bits(v)) and np.array_equal(gt, t), name
    v, t = meshes["single triangle"]
    assert _fill(gpu, v, t, 3, "pillow")[1].tolist() == [[2, 0, 1], [0, 2, 1]]
    v, t = meshes["open cube"]
    gv, gt, _ = _fill(gpu, v, t, 4, "cube")
    assert gv[8].tolist() == [0.5, 0.5, 1.0] and gt[-4:].tolist() == [[6, 4, 8], [4, 5, 8], [7, 6, 8], [5, 7, 8]]
    again = _fill(gpu, gv, gt, 4, "cube again")  # filling twice fills nothing the second time
    assert not any(again[2].values()) and np.array_equal(again[1], gt) and np.array_equal(_bits(again[0]), _bits(gv))


def test_fill_errors(gpu, meshes):
    v, t = meshes["open cube"]
    tv, tt = torch.from_numpy(v).to(gpu), torch.from_numpy(t).to(gpu)
    ctx = ops.context(gpu)
    want = ops.mesh_fill_holes(tv, tt, 4)
    for bad in (2, ALL + 1):
        with pytest.raises(ValueError, match="max_edges"):
            ops.mesh_fill_holes(tv, tt, bad)
        # the library's own check (ops.mesh_fill_holes makes it first, in Python)
        nvo, nto, rep = ops.i64(0), ops.i64(0), _lib.MeshFillReport()
        with pytest.raises(AsrHipError, match="max_edges"):
            ctx.call("asr_hip_mesh_fill_holes_count", _lib.ptr(tv), ops.i64(len(v)), _lib.ptr(tt), ops.i64(len(t)), ops.i64(bad),
                     ops.ctypes.byref(nvo), ops.ctypes.byref(nto), ops.ctypes.byref(rep))
    for where, value in (((3, 1), -1), ((9, 2), len(v)), ((0, 0), 2 ** 31 - 1)):
        bad = tt.clone()
        bad[where] = value
        with pytest.raises(AsrHipError, match="out of range"):
            ops.mesh_fill_holes(tv, bad, 4)
    with pytest.raises(AsrHipError, match="out of range"):
        ops.mesh_fill_holes(tv[:0], tt, 4)
    for value in (float("nan"), float("inf")):
        bad = tv.clone()
        bad[5, 1] = value  # on the rim
        with pytest.raises(AsrHipError, match="not finite"):
            ops.mesh_fill_holes(bad, tt, 4)
        got = ops.mesh_fill_holes(bad, tt, 3, return_report=True)  # the rim stays open: its vertices are not read
        assert got[2]["filled"] == 0 and torch.equal(got[0].view(torch.int32), bad.view(torch.int32))
        bad = tv.clone()
        bad[0, 2] = value  # off the rim
        got = ops.mesh_fill_holes(bad, tt, 4, return_report=True)
        assert got[2]["filled"] == 1 and torch.equal(got[0][:8].view(torch.int32), bad.view(torch.int32))
        assert torch.equal(got[0][8:].view(torch.int32), want[0][8:].view(torch.int32)) and torch.equal(got[1], want[1])
    with pytest.raises(AsrHipError, match="must follow"):
        ctx.call("asr_hip_mesh_fill_holes_fill", _lib.ptr(want[0]), _lib.ptr(want[1]))
    ops.mesh_topology(tt, len(v))  # another mesh call between the two
    nvo, nto, rep = ops.i64(0), ops.i64(0), _lib.MeshFillReport()
    ctx.call("asr_hip_mesh_fill_holes_count", _lib.ptr(tv), ops.i64(len(v)), _lib.ptr(tt), ops.i64(len(t)), ops.i64(4),
             ops.ctypes.byref(nvo), ops.ctypes.byref(nto), ops.ctypes.byref(rep))
    assert (nvo.value, nto.value, rep.filled) == (9, 14, 1)
    ops.mesh_topology(tt, len(v))
    with pytest.raises(AsrHipError, match="must follow"):
        ctx.call("asr_hip_mesh_fill_holes_fill", _lib.ptr(want[0]), _lib.ptr(want[1]))
    with pytest.raises(AsrHipError, match="GPU tensor"):
        ops.mesh_fill_holes(tv.cpu(), tt, 4)
    for call in (lambda: ops.mesh_fill_holes(tv[:, :2], tt, 4), lambda: ops.mesh_fill_holes(tv, tt.reshape(-1), 4)):
        with pytest.raises(ValueError):
            call()
    # ... and the context still works
    got = ops.mesh_fill_holes(tv, tt, 4)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
    # no triangles, no vertices
    got = ops.mesh_fill_holes(tv, tt[:0], 4, return_report=True)
    assert torch.equal(got[0].view(torch.int32), tv.view(torch.int32)) and got[1].shape == (0, 3) and not any(got[2].values())
    got = ops.mesh_fill_holes(tv[:0], tt[:0], 4)
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3)


def test_fill_on_a_side_stream(gpu, meshes):
    """the inputs arrive late on a side stream (all-zero bytes until then: degenerate triangles, nothing to fill); the call
    on that stream must wait for them"""
    v, t = meshes["renumbered holes"]
    tv, tt = torch.from_numpy(v).to(gpu), torch.from_numpy(t).to(gpu)
    ref = ops.mesh_fill_holes(tv, tt, 12, return_report=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    (lv, lt), _ = late(side, tv, tt)
    with torch.cuda.stream(side):
        got = ops.mesh_fill_holes(lv, lt, 12, return_report=True)
    side.synchronize()
    assert got[2] == ref[2] and ref[2]["filled"] == 3
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1])
    torch.cuda.synchronize()
    back = ops.mesh_fill_holes(tv, tt, 12)  # and the default stream again
    assert torch.equal(back[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(back[1], ref[1])


# ---- 2. the layers above -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(gpu):
    p, q = synth.scan_cloud(6000, seed=31, device="cpu")
    pts, nrm = p.numpy(), q.numpy()
    return pts, nrm, synth.knn_radii(pts, 24), synth.bounding_box(pts, 0.1), synth.make_weights(4, seed=31)


def _rim_lengths(v, t):
    tail, head = F.directed_boundary(t, len(v))
    rim_of = F.rim_ids(tail, head, len(v))
    return np.sort(np.bincount(rim_of[tail])[np.unique(rim_of[rim_of >= 0])])


def test_pipeline_mesh_fill_holes(gpu, scene):
    pts, nrm, rad, bb, weights = scene
    pipe = ImplicitPipeline(weights, device=gpu)
    pipe.forward(*(torch.from_numpy(a).to(gpu) for a in (pts, nrm, rad)), *bb)
    v, t = pipe.mesh()
    v0, t0 = pipe.mesh(fill_holes=0)
    assert torch.equal(v0.view(torch.int32), v.view(torch.int32)) and torch.equal(t0, t) and len(t) > 500
    lengths = _rim_lengths(v.cpu().numpy(), t.cpu().numpy())
    print("pipeline mesh: rim lengths", lengths.tolist())
    cap = int(lengths.max()) if len(lengths) else 3  # every simple rim of this mesh
    vf, tf = pipe.mesh(fill_holes=cap)
    want = ops.mesh_fill_holes(v, t, cap, return_report=True)
    print("pipeline mesh:", want[2])
    assert torch.equal(vf.view(torch.int32), want[0].view(torch.int32)) and torch.equal(tf, want[1])
    ref = F.fill_holes(v.cpu().numpy(), t.cpu().numpy(), cap)
    _compare(v.cpu().numpy(), t.cpu().numpy(), (want[0].cpu().numpy(), want[1].cpu().numpy(), want[2]), ref, "pipeline mesh")
    assert want[2]["rims"] == ops.mesh_topology(t, len(v))["boundary_loops"]
    assert want[2]["filled"] >= 1 and len(vf) > len(v)  # (the seeded cloud's mesh has simple rims: the checks below bite)
    # before smooth: the smoother moves the hubs too
    got = pipe.mesh(fill_holes=cap, smooth=2)
    hand = ops.mesh_smooth(want[0], want[1], iterations=2)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), hand.view(torch.int32))
    assert not torch.equal(hand[len(v):].view(torch.int32), want[0][len(v):].view(torch.int32))
    # between simplify and smooth
    vs, ts = pipe.mesh(simplify=1)
    caps = _rim_lengths(vs.cpu().numpy(), ts.cpu().numpy())
    cap = int(caps.max()) if len(caps) else 3
    got = pipe.mesh(simplify=1, fill_holes=cap, smooth=2)
    filled = ops.mesh_fill_holes(vs, ts, cap, return_report=True)
    print("simplified pipeline mesh:", filled[2])
    hand = ops.mesh_smooth(filled[0], filled[1], iterations=2)
    assert torch.equal(got[1], filled[1]) and torch.equal(got[0].view(torch.int32), hand.view(torch.int32))
    assert torch.equal(pipe.mesh(simplify=1, smooth=2, fill_holes=0)[0].view(torch.int32),
                       ops.mesh_smooth(vs, ts, iterations=2).view(torch.int32))
    for bad in (2, -1, ALL + 1):
        with pytest.raises(ValueError):
            pipe.mesh(fill_holes=bad)


def test_reconstruct_surface_fill_mesh_holes_and_asrtool(gpu, scene, tmp_path):
    import adaptivesurfacereconstruction as asr
    import asrtool
    pts, nrm, _, _, weights = scene
    plain = asr.reconstruct_surface(pts, nrm, weights=weights)
    zero = asr.reconstruct_surface(pts, nrm, weights=weights, fill_holes=0)
    assert sorted(zero) == ["triangles", "vertices"]
    assert np.array_equal(_bits(zero["vertices"]), _bits(plain["vertices"])) and np.array_equal(zero["triangles"], plain["triangles"])
    lengths = _rim_lengths(plain["vertices"], plain["triangles"])
    cap = int(lengths.max()) if len(lengths) else 3
    res = asr.reconstruct_surface(pts, nrm, weights=weights, fill_holes=cap, vertex_normals=True)
    hand = asr.fill_mesh_holes(plain["vertices"], plain["triangles"].astype(np.int64), cap)
    print("reconstructed mesh: rim lengths", lengths.tolist(), {k: hand[k] for k in F.REPORT_FIELDS})
    assert sorted(hand) == sorted(("vertices", "triangles") + F.REPORT_FIELDS)
    assert hand["vertices"].dtype == np.float32 and hand["triangles"].dtype == np.int32
    assert np.array_equal(_bits(res["vertices"]), _bits(hand["vertices"])) and np.array_equal(res["triangles"], hand["triangles"])
    assert res["vertex_normals"].shape == res["vertices"].shape
    ref = F.fill_holes(plain["vertices"], plain["triangles"], cap)
    _compare(plain["vertices"], plain["triangles"], (hand["vertices"], hand["triangles"], {k: hand[k] for k in F.REPORT_FIELDS}),
             ref, "reconstructed mesh")
    # asrtool --fill-holes is that call (in this process: the tool's own start is not what is tested)
    np.savez(str(tmp_path / "w.npz"), **weights)
    ply.write_points(str(tmp_path / "in.ply"), pts, nrm)
    assert asrtool.main(["--in", str(tmp_path / "in.ply"), "--out", str(tmp_path / "out.ply"), "--weights",
                         str(tmp_path / "w.npz"), "--fill-holes", str(cap), "--normals"]) == 0
    v, t, n = ply.read_mesh(str(tmp_path / "out.ply"), with_normals=True)
    assert np.array_equal(_bits(v), _bits(res["vertices"])) and np.array_equal(t, res["triangles"])
    assert np.array_equal(_bits(n), _bits(res["vertex_normals"]))


def test_fill_mesh_holes_and_asrtool_fill_mesh(gpu, tmp_path, capsys):
    import adaptivesurfacereconstruction as asr
    import asrtool
    v, t = F.renumbered_holes()
    res = asr.fill_mesh_holes(v, t, 12)
    ref = F.fill_holes(v, t, 12)
    _compare(v, t, (res["vertices"], res["triangles"], {k: res[k] for k in F.REPORT_FIELDS}), ref, "renumbered holes")
    assert res["filled"] == 3 and asr.mesh_topology(res["triangles"], len(res["vertices"]))["watertight"]
    col = np.stack([np.arange(len(v)) % 256, np.full(len(v), 90), (7 * np.arange(len(v))) % 251], 1).astype(np.uint8)
    nrm = (v / np.maximum(np.sqrt((v.astype(np.float64) ** 2).sum(1, keepdims=True)), 1e-9)).astype(np.float32)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    ply.write_mesh(src, v, t, colors=col, normals=nrm)
    capsys.readouterr()
    assert asrtool.main(["--fill-mesh", src, dst, "--max-edges", "12"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == ref[2]
    v2, t2, n2, c2 = ply.read_mesh(dst, with_normals=True, with_colors=True)
    assert np.array_equal(_bits(v2), _bits(res["vertices"])) and np.array_equal(t2, res["triangles"])
    assert np.array_equal(c2[:len(v)], col) and np.array_equal(_bits(n2[:len(v)]), _bits(nrm))
    new = t2[len(t):]
    for hub in range(len(v), len(v2)):  # the mean over the rim vertices its triangles name
        rim = new[new[:, 2] == hub, 1]
        assert len(rim) in (4, 12)
        assert np.array_equal(c2[hub], np.rint(col[rim].astype(np.float64).mean(0)).astype(np.uint8))
        assert np.allclose(n2[hub], nrm[rim].astype(np.float64).mean(0), rtol=0, atol=1e-6)
    # a mesh without normals and colours, and a cap that fills one rim only
    ply.write_mesh(src, v, t)
    assert asrtool.main(["--fill-mesh", src, dst, "--max-edges", "4"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == F.fill_holes(v, t, 4)[2]
    v3, t3, n3, c3 = ply.read_mesh(dst, with_normals=True, with_colors=True)
    assert n3 is None and c3 is None and len(v3) == len(v) + 1 and len(t3) == len(t) + 4
