"""GPU tests of asr_hip_points_merge_count / _fill against the numpy restatement of their contract
(tests/points_merge_ref.py; what the restatement itself gives on clouds with known answers is checked in
tests/test_points_merge.py), and of their users: merge_points, reconstruct_surface(thin=) and the two asrtool forms.

Counts, map, order (through the map) and report are integers and must equal the restatement.  Every value must lie
within 1 f32 ulp of the restatement's: both sides sum in f64 and round once to f32, a cluster of up to
ASR_MERGE_LONG_CLUSTER members even in the same order (those are also required to agree bit for bit).  Normals are
compared where |sum n| >= 1e-3 sum |n| (or where the sum has no finite positive length and the first member's normal is
copied); at most 1 % of the clusters may be left out, which tests/test_points_merge.py shows for the restatement alone.
The clouds keep every mean away from zero (positive coordinates, radii and attributes where long clusters occur), since
an ulp of a cancelled mean is not what the f64 sums promise.  Every call runs twice and must give the same bits."""
import numpy as np
import pytest
import torch

import points_merge_ref as P
from asr_hip import _lib, ops, ply, synth
from stream_helpers import late

pytestmark = pytest.mark.gpu

T = _lib.ASR_MERGE_LONG_CLUSTER
VALUES = ("points", "normals", "radii", "attributes")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _t(gpu, a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu).to(dtype)


def _merge(gpu, frame, pts, nrm=None, rad=None, att=None, level=None, levels=None, split_sides=False):
    """the op twice (equal bits) -> dict of numpy arrays like the restatement's"""
    args = (frame, _t(gpu, pts), _t(gpu, nrm), _t(gpu, rad), _t(gpu, att))
    kwargs = dict(level=level, levels=_t(gpu, levels, torch.int8), split_sides=split_sides, return_map=True,
                  return_counts=True, return_report=True)
    a = ops.points_merge(*args, **kwargs)
    b = ops.points_merge(*args, **kwargs)
    assert len(a) == 7 and a[6] == b[6] and all(type(x) is int for x in a[6].values())
    for x, y in zip(a[:6], b[:6]):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert a[4].dtype == torch.int32 and a[5].dtype == torch.int32
    plain = ops.points_merge(*args, level=level, levels=kwargs["levels"], split_sides=split_sides)
    assert len(plain) == 4 and torch.equal(plain[0].view(torch.int32), a[0].view(torch.int32))
    host = lambda x: None if x is None else x.cpu().numpy()  # noqa: E731
    return dict(points=host(a[0]), normals=host(a[1]), radii=host(a[2]), attributes=host(a[3]), cluster=host(a[4]),
                counts=host(a[5]), report=a[6])


def _compare(got, ref, what):
    assert got["report"] == ref["report"], what
    assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["cluster"], ref["cluster"]), what
    short = ref["counts"] <= T
    for name in VALUES:
        assert (got[name] is None) == (ref[name] is None), (what, name)
        if ref[name] is None:
            continue
        assert got[name].shape == ref[name].shape and got[name].dtype == np.float32, (what, name)
        rows = ref["normal_ok"] if name == "normals" else np.ones(len(ref["counts"]), bool)
        d = P.ulp_distance(got[name][rows], ref[name][rows])
        print("%s %s: %d clusters (%d long, %d left out), %d values differ, largest distance %d ulp"
              % (what, name, len(rows), int((~short).sum()), int((~rows).sum()), int((d > 0).sum()), int(d.max()) if d.size else 0))
        assert np.all(d <= 1), (what, name)
        same = _bits(got[name][rows & short]) == _bits(ref[name][rows & short])
        nan = np.isnan(ref[name][rows & short]) & np.isnan(got[name][rows & short])
        assert np.all(same | nan), (what, name)
    assert (~ref["normal_ok"]).mean() <= 0.01 if len(ref["counts"]) else True, what


@pytest.fixture(scope="module")
def scan():
    return P.scan_case()


# ---- 1. the operator --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_scan_cloud_at_one_level(gpu, scan, split):  # (a)
    frame, pts, nrm, rad, att, level = scan
    got = _merge(gpu, frame, pts, nrm, rad, att, level=level, split_sides=split)
    ref = P.merge(frame, pts, nrm, rad, att, level=level, split_sides=split)
    _compare(got, ref, "scan, level %d, split %d" % (level, split))
    assert np.isin(ref["counts"], np.arange(2, 11)).mean() > 0.5
    lo, hi = P.boxes(frame, pts, level, ref)
    tol = 2.0 ** -22 * np.maximum(np.abs(lo), np.abs(hi))
    assert np.all(got["points"] >= lo - tol) and np.all(got["points"] <= hi + tol)


def test_scan_cloud_with_levels_from_the_radii(gpu, scan):  # (b)
    frame, pts, nrm, rad, att, _ = scan
    keys = ops.point_keys(frame, _t(gpu, pts), _t(gpu, rad) * 0.5, 1.0, 21).cpu().numpy().view(np.uint64)
    levels = np.zeros(len(pts), np.int64)
    for l in range(1, 22):
        levels[keys >= np.uint64(1 << (3 * l))] = l
    assert np.array_equal(levels, P.radius_levels(frame, rad, 0.5)) and len(np.unique(levels)) >= 2
    for split in (False, True):
        got = _merge(gpu, frame, pts, nrm, rad, att, levels=levels, split_sides=split)
        _compare(got, P.merge(frame, pts, nrm, rad, att, levels=levels, split_sides=split), "scan, levels, split %d" % split)
    bad = levels.copy()
    bad[77] = 22
    with pytest.raises(_lib.AsrHipError, match="level"):
        ops.points_merge(frame, _t(gpu, pts), levels=_t(gpu, bad, torch.int8))
    bad[77] = -1
    with pytest.raises(_lib.AsrHipError, match="level"):
        ops.points_merge(frame, _t(gpu, pts), levels=_t(gpu, bad, torch.int8))
    with pytest.raises(_lib.AsrHipError, match="must follow"):  # a refused count leaves nothing to fill
        ops.context(gpu).call("asr_hip_points_merge_fill", None, None, None, None, None, None)
    again = _merge(gpu, frame, pts, nrm, rad, att, levels=levels, split_sides=True)
    assert again["report"] == got["report"] and np.array_equal(_bits(again["points"]), _bits(got["points"]))


def test_cluster_sizes_round_the_threshold_and_one_cell(gpu):  # (c)
    sizes = [1, 2, T - 1, T, T + 1, 4 * T + 3]
    frame, pts, nrm, rad, att = P.sized_clusters(sizes)
    for split in (False, True):
        got = _merge(gpu, frame, pts, nrm, rad, att, level=4, split_sides=split)
        ref = P.merge(frame, pts, nrm, rad, att, level=4, split_sides=split)
        assert sorted(ref["counts"].tolist()) == sizes
        _compare(got, ref, "sizes round %d, split %d" % (T, split))
    frame, pts, nrm, rad, att = P.one_cell_cloud(50000)
    got = _merge(gpu, frame, pts, nrm, rad, att, level=0, split_sides=True)
    ref = P.merge(frame, pts, nrm, rad, att, level=0, split_sides=True)
    assert ref["report"] == dict(clusters=1, dropped=0, largest_cluster=50000, split_cells=0)
    _compare(got, ref, "50000 points in one cell")


@pytest.mark.parametrize("zero_first", [False, True])
def test_thin_wall(gpu, zero_first):  # (d)
    frame, pts, nrm, level = P.thin_wall(zero_first=zero_first)
    rad = np.linspace(0.01, 0.02, len(pts)).astype(np.float32)
    for split in (True, False):
        got = _merge(gpu, frame, pts, nrm, rad, level=level, split_sides=split)
        ref = P.merge(frame, pts, nrm, rad, level=level, split_sides=split)
        _compare(got, ref, "thin wall, zero_first %d, split %d" % (zero_first, split))
        assert ref["report"]["split_cells"] == ((35 if zero_first else 36) if split else 0)


def test_dropped_points(gpu, scan):  # (e)
    frame, pts, nrm, rad, att, level = scan
    rng = np.random.default_rng(3)
    bad = pts.copy()
    pick = rng.permutation(len(pts))[:430]  # the first 400 are dropped, the last 40 get non-finite values
    bad[pick[:100]] = np.nan
    bad[pick[100:200], 1] = np.inf
    bad[pick[200:300], 2] = -np.inf
    bad[pick[300:350]] *= np.float32(1e6)   # finite, outside the root cube
    bad[pick[350:400], 0] = np.float32(3e38)
    rad2, att2, nrm2 = rad.copy(), att.copy(), nrm.copy()
    rad2[pick[390:410]] = np.nan            # non-finite values propagate and drop nothing
    att2[pick[395:420], 1] = np.inf
    nrm2[pick[398:430], 0] = np.inf
    for split in (False, True):
        got = _merge(gpu, frame, bad, nrm2, rad2, att2, level=level, split_sides=split)
        ref = P.merge(frame, bad, nrm2, rad2, att2, level=level, split_sides=split)
        assert ref["report"]["dropped"] == 400 and np.array_equal(np.sort(pick[:400]), np.nonzero(ref["cluster"] < 0)[0])
        _compare(got, ref, "scan with dropped points, split %d" % split)
        assert np.isnan(got["radii"]).any() and np.isinf(got["attributes"]).any()
    nothing = np.full((300, 3), np.nan, np.float32)
    nothing[::3] = 1e30
    got = _merge(gpu, frame, nothing, nrm[:300], rad[:300], att[:300], level=level, split_sides=True)
    assert got["report"] == dict(clusters=0, dropped=300, largest_cluster=0, split_cells=0)
    assert got["points"].shape == (0, 3) and got["attributes"].shape == (0, 3) and np.all(got["cluster"] == -1)
    _compare(got, P.merge(frame, nothing, nrm[:300], rad[:300], att[:300], level=level, split_sides=True), "all dropped")


def test_empty_and_single_point(gpu):  # (f)
    frame = P.unit_frame()
    z = np.zeros((0, 3), np.float32)
    got = _merge(gpu, frame, z, z, np.zeros(0, np.float32), np.zeros((0, 2), np.float32), level=5, split_sides=True)
    assert got["report"] == dict(clusters=0, dropped=0, largest_cluster=0, split_cells=0)
    assert got["points"].shape == (0, 3) and got["attributes"].shape == (0, 2) and got["cluster"].shape == (0,)
    one = np.array([[0.25, 0.5, 0.75]], np.float32)
    nrm, rad, att = np.array([[0, 0, 0]], np.float32), np.array([np.nan], np.float32), np.array([[1.5, -0.0]], np.float32)
    for level in (0, 9, 21):
        got = _merge(gpu, frame, one, nrm, rad, att, level=level, split_sides=True)
        assert got["report"] == dict(clusters=1, dropped=0, largest_cluster=1, split_cells=0)
        assert np.array_equal(_bits(got["points"]), _bits(one)) and np.array_equal(_bits(got["normals"]), _bits(nrm))
        assert np.array_equal(_bits(got["radii"]), _bits(rad)) and np.array_equal(_bits(got["attributes"]), _bits(att))
        assert got["counts"].tolist() == [1] and got["cluster"].tolist() == [0]
    got = _merge(gpu, frame, np.array([[np.nan, 0, 0]], np.float32), level=3)
    assert got["report"]["dropped"] == 1 and got["cluster"].tolist() == [-1] and len(got["points"]) == 0


def test_exact_duplicates(gpu, scan):  # (g)
    frame, pts, nrm, rad, att, level = scan
    pts, nrm, rad, att = pts[:3000].copy(), nrm[:3000].copy(), rad[:3000].copy(), att[:3000].copy()
    pts[100:200], nrm[100:200] = pts[0:100], nrm[0:100]
    for kwargs in (dict(level=level), dict(level=21), dict(level=21, split_sides=True)):
        got = _merge(gpu, frame, pts, nrm, rad, att, **kwargs)
        ref = P.merge(frame, pts, nrm, rad, att, **kwargs)
        _compare(got, ref, "duplicates %s" % sorted(kwargs.items()))
        assert np.array_equal(got["cluster"][100:200], got["cluster"][0:100])
    assert ref["report"]["largest_cluster"] >= 2 and np.all(ref["counts"][ref["cluster"][0:100]] >= 2)
    # the mean of two equal points is that point
    two = ref["counts"][ref["cluster"][0:100]] == 2
    assert np.array_equal(_bits(got["points"][got["cluster"][0:100]][two]), _bits(pts[0:100][two]))


def test_channel_counts_and_null_arguments(gpu, scan):  # (h)
    frame, pts, nrm, rad, _, level = scan
    pts, nrm, rad = pts[:5000], nrm[:5000], rad[:5000]
    rng = np.random.default_rng(8)
    for c in (1, 16):
        att = rng.uniform(1.0, 2.0, (len(pts), c)).astype(np.float32)
        got = _merge(gpu, frame, pts, nrm, rad, att, level=level, split_sides=True)
        _compare(got, P.merge(frame, pts, nrm, rad, att, level=level, split_sides=True), "%d channels" % c)
    flat = _merge(gpu, frame, pts, att=att[:, 0], level=level)  # [N] is one channel
    assert flat["attributes"].shape == (len(flat["points"]), 1)
    full = P.merge(frame, pts, nrm, rad, att, level=level)
    tp, tn, tr, ta = (_t(gpu, a) for a in (pts, nrm, rad, att))
    for keep in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)):  # every optional input absent in turn
        a = ops.points_merge(frame, tp, tn if keep[0] else None, tr if keep[1] else None, ta if keep[2] else None, level=level)
        assert [x is not None for x in a[1:]] == [bool(k) for k in keep]
        assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(full["points"]))
        for x, name in zip(a[1:], VALUES[1:]):
            if x is not None:
                rows = full["normal_ok"] if name == "normals" else slice(None)
                assert np.array_equal(_bits(x.cpu().numpy()[rows]), _bits(full[name][rows])), name
    # every output pointer NULL in turn, at the C ABI
    ctx = ops.context(gpu)
    m, c = len(full["points"]), att.shape[1]
    import ctypes
    for skip in range(7):
        outs = [torch.full((m, 3), 7.0, device=gpu), torch.full((m, 3), 7.0, device=gpu), torch.full((m,), 7.0, device=gpu),
                torch.full((m, c), 7.0, device=gpu), torch.full((m,), -7, dtype=torch.int32, device=gpu),
                torch.full((len(pts),), -7, dtype=torch.int32, device=gpu)]
        n_out = ctypes.c_int64(0)
        ctx.call("asr_hip_points_merge_count", ctypes.byref(frame), _lib.ptr(tp), ctypes.c_int64(len(pts)), _lib.ptr(tn),
                 _lib.ptr(tr), _lib.ptr(ta), c, None, level, 0, ctypes.byref(n_out), None)
        assert n_out.value == m
        ctx.call("asr_hip_points_merge_fill", *[_lib.ptr(None if i == skip else o) for i, o in enumerate(outs)])
        for i, (o, want) in enumerate(zip(outs, [full[k] for k in VALUES] + [full["counts"], full["cluster"]])):
            o = o.cpu().numpy()
            if i == skip:
                assert np.all(o == (7.0 if i < 4 else -7))
            elif i == 1:
                assert np.array_equal(_bits(o[full["normal_ok"]]), _bits(want[full["normal_ok"]]))
            elif i < 4:
                assert np.array_equal(_bits(o), _bits(want))
            else:
                assert np.array_equal(o, want)
    with pytest.raises(_lib.AsrHipError, match="must follow"):
        ctx.call("asr_hip_points_merge_fill", None, None, None, None, None, None)
    with pytest.raises(_lib.AsrHipError):  # no CPU fallback
        ops.points_merge(frame, torch.from_numpy(pts), level=level)


def test_inputs_arriving_late_on_a_side_stream(gpu, scan):  # (i)
    frame, pts, nrm, rad, att, level = scan
    tensors = [_t(gpu, a) for a in (pts, nrm, rad, att)]
    ref = ops.points_merge(frame, *tensors, level=level, split_sides=True, return_map=True, return_counts=True,
                           return_report=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    lt, _ = late(side, *tensors)
    with torch.cuda.stream(side):
        got = ops.points_merge(frame, *lt, level=level, split_sides=True, return_map=True, return_counts=True,
                               return_report=True)
    side.synchronize()
    assert got[6] == ref[6] and ref[6]["clusters"] > 1000
    for x, y in zip(got[:6], ref[:6]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    torch.cuda.synchronize()
    back = ops.points_merge(frame, *tensors, level=level, split_sides=True)  # and the default stream again
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(back, ref[:4]))


# ---- 2. the layers above (j) ------------------------------------------------------------------------------------------
def test_merge_points_is_the_operator(gpu, scan):
    import adaptivesurfacereconstruction as asr
    frame, pts, nrm, rad, att, level = scan
    cell = 1.5 * float(frame.voxel_size[level + 1])  # the level whose voxel size lies in [cell, 2 cell)
    res = asr.merge_points(pts, nrm, rad, att, cell_size=cell)
    assert sorted(res) == sorted(("points", "normals", "radii", "attributes", "counts", "cluster", "report", "cell_size"))
    assert res["cell_size"] == float(frame.voxel_size[level]) and cell <= res["cell_size"] < 2 * cell
    want = _merge(gpu, frame, pts, nrm, rad, att, level=level, split_sides=True)
    for name in VALUES:
        assert np.array_equal(_bits(res[name]), _bits(want[name])), name
    assert np.array_equal(res["counts"], want["counts"]) and np.array_equal(res["cluster"], want["cluster"])
    assert res["report"] == want["report"]
    # split_sides is ignored without normals; NaN points are dropped and do not stretch the frame
    bad = pts.copy()
    bad[5] = np.nan
    res = asr.merge_points(bad, radii=rad, cell_size=cell, split_sides=True)
    assert res["normals"] is None and res["attributes"] is None and res["report"]["dropped"] == 1 and res["cluster"][5] == -1
    # radius_factor: the levels of the octree build
    res = asr.merge_points(pts, nrm, rad, att, radius_factor=0.5, split_sides=False)
    want = _merge(gpu, frame, pts, nrm, rad, att, levels=P.radius_levels(frame, rad, 0.5))
    assert res["cell_size"] is None and res["report"] == want["report"]
    for name in VALUES:
        assert np.array_equal(_bits(res[name]), _bits(want[name])), name


@pytest.fixture(scope="module")
def scene():
    p, q = synth.scan_cloud(6000, seed=31, device="cpu")
    return p.numpy(), q.numpy(), synth.make_weights(4, seed=31)


def test_reconstruct_surface_thin(gpu, scene):
    import adaptivesurfacereconstruction as asr
    pts, nrm, weights = scene
    plain = asr.reconstruct_surface(pts, nrm, weights=weights)
    zero = asr.reconstruct_surface(pts, nrm, weights=weights, thin=0)
    assert sorted(zero) == ["triangles", "vertices"]
    assert np.array_equal(_bits(zero["vertices"]), _bits(plain["vertices"])) and np.array_equal(zero["triangles"], plain["triangles"])
    cell = 0.3 * float(synth.knn_radii(pts, 24).mean())
    col = np.random.default_rng(4).uniform(0, 255, (len(pts), 3)).astype(np.float32)
    merged = asr.merge_points(pts, nrm, attributes=col, cell_size=cell)
    print("thin: %d -> %d points at cell size %g" % (len(pts), len(merged["points"]), merged["cell_size"]))
    assert 0.2 * len(pts) < len(merged["points"]) < 0.95 * len(pts)
    res = asr.reconstruct_surface(pts, nrm, weights=weights, thin=cell, point_attributes=col)
    hand = asr.reconstruct_surface(merged["points"], merged["normals"], weights=weights, point_attributes=merged["attributes"])
    assert len(res["triangles"]) > 500 and sorted(res) == ["triangles", "vertex_attributes", "vertices"]
    assert np.array_equal(_bits(res["vertices"]), _bits(hand["vertices"])) and np.array_equal(res["triangles"], hand["triangles"])
    assert np.array_equal(_bits(res["vertex_attributes"]), _bits(hand["vertex_attributes"]))
    assert not np.array_equal(res["triangles"], plain["triangles"])
    # given radii are merged alike
    rad = synth.knn_radii(pts, 24)
    merged = asr.merge_points(pts, nrm, rad, cell_size=cell)
    res = asr.reconstruct_surface(pts, nrm, rad, weights=weights, thin=cell)
    hand = asr.reconstruct_surface(merged["points"], merged["normals"], merged["radii"], weights=weights)
    assert np.array_equal(_bits(res["vertices"]), _bits(hand["vertices"])) and np.array_equal(res["triangles"], hand["triangles"])


def test_asrtool_thin_cloud_round_trip(gpu, scan, tmp_path, capsys):
    import adaptivesurfacereconstruction as asr
    import asrtool
    _, pts, nrm, rad, _, _ = scan
    pts, nrm, rad = pts[:4000], nrm[:4000], rad[:4000]
    col = np.random.default_rng(9).integers(0, 256, (len(pts), 3)).astype(np.uint8)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    cell = 2.0 * float(rad.mean())
    ply.write_points(src, pts, nrm, rad, colors=col)
    capsys.readouterr()
    assert asrtool.main(["--thin-cloud", src, dst, "--cell", repr(cell)]) == 0
    want = asr.merge_points(pts, nrm, rad, col.astype(np.float32), cell_size=cell)
    assert ("%d -> %d points" % (len(pts), len(want["points"]))) in capsys.readouterr().out
    p2, n2, r2 = ply.read_points(dst)
    assert len(p2) < len(pts)
    assert np.array_equal(_bits(p2), _bits(want["points"])) and np.array_equal(_bits(n2), _bits(want["normals"]))
    assert np.array_equal(_bits(r2), _bits(want["radii"]))
    assert np.array_equal(ply.read_point_colors(dst), np.rint(np.clip(want["attributes"], 0, 255)).astype(np.uint8))
    # a cloud without radii and colours
    ply.write_points(src, pts, nrm)
    assert asrtool.main(["--thin-cloud", src, dst, "--cell", repr(cell)]) == 0
    p3, n3, r3 = ply.read_points(dst)
    assert np.array_equal(_bits(p3), _bits(want["points"])) and len(r3) == 0 and ply.read_point_colors(dst) is None
