"""Point merge without a GPU: the ABI of asr_hip_points_merge_count / _fill, the argument checks of every layer above it
that need no device, and what the numpy restatement of the contract (tests/points_merge_ref.py) gives on clouds with
known answers.  The restatement is what tests/test_gpu_points_merge.py holds the kernels to; here it is also shown that on
the clouds of those tests at most 1 % of the clusters have a normal sum too short to be compared."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_simplify_ref as R
import points_merge_ref as P
from asr_hip import _lib, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _lib.ASR_MERGE_LONG_CLUSTER


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- 1. the ABI -------------------------------------------------------------------------------------------------------
def test_exports_and_threshold():
    header = open(os.path.join(REPO, "include", "asr_hip.h")).read()
    lib = _lib.load()
    for name in ("asr_hip_points_merge_count", "asr_hip_points_merge_fill"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert int(re.search(r"#define ASR_MERGE_LONG_CLUSTER (\d+)", header).group(1)) == T
    assert int(re.search(r"#define ASR_MAX_ATTRIBUTE_CHANNELS (\d+)", header).group(1)) == _lib.ASR_MAX_ATTRIBUTE_CHANNELS
    assert lib.asr_hip_struct_size(b"asr_points_merge_report") == 8 * 4 == ctypes.sizeof(_lib.PointsMergeReport)
    assert tuple(n for n, _ in _lib.PointsMergeReport._fields_) == P.REPORT_FIELDS
    assert lib.asr_hip_version().decode().startswith("0.2.0")
    # without a context nothing runs
    assert lib.asr_hip_points_merge_fill(None, None, None, None, None, None, None) == 1


# ---- 2. argument checks that need no device ---------------------------------------------------------------------------
def test_ops_argument_checks():
    frame = P.unit_frame()
    pts = torch.full((5, 3), 0.5)
    nrm = torch.ones((5, 3))
    for kwargs in (dict(level=-1), dict(level=22), dict(level=1.5), dict(level=True), dict(), dict(level=3, levels=torch.zeros(5)),
                   dict(levels=torch.zeros(4)), dict(level=3, split_sides=True),
                   dict(level=3, attributes=torch.zeros((5, 17))), dict(level=3, attributes=torch.zeros((5, 0))),
                   dict(level=3, attributes=torch.zeros((4, 3))), dict(level=3, radii=torch.zeros(4)),
                   dict(level=3, normals=torch.zeros((5, 2)))):
        with pytest.raises(ValueError):
            ops.points_merge(frame, pts, **kwargs)
    with pytest.raises(ValueError):
        ops.points_merge(frame, torch.zeros((5, 2)), level=3)
    # valid arguments reach the device check: CPU tensors are refused, nothing else is computed instead
    with pytest.raises(_lib.AsrHipError):
        ops.points_merge(frame, pts, nrm, level=3, split_sides=True)


def test_module_argument_checks():
    import adaptivesurfacereconstruction as asr
    pts = np.full((5, 3), 0.5, np.float32)
    nrm = np.ones((5, 3), np.float32)
    rad = np.full(5, 0.1, np.float32)
    for kwargs in (dict(), dict(cell_size=0.1, radius_factor=0.5, radii=rad), dict(cell_size=0.0), dict(cell_size=-1.0),
                   dict(cell_size=float("nan")), dict(radius_factor=0.5), dict(radius_factor=0.0, radii=rad),
                   dict(cell_size=0.1, attributes=np.zeros((5, 17))), dict(cell_size=0.1, attributes=np.zeros((4, 3))),
                   dict(cell_size=0.1, radii=rad[:4]), dict(cell_size=0.1, normals=nrm[:4])):
        with pytest.raises(ValueError):
            asr.merge_points(pts, **kwargs)
    with pytest.raises(ValueError):
        asr.merge_points(np.full((5, 3), np.nan, np.float32), cell_size=0.1)
    for thin in (-1, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            asr.reconstruct_surface(pts, nrm, thin=thin)


def test_asrtool_refuses_bad_thin_arguments(tmp_path, capsys):
    import asrtool
    src = str(tmp_path / "in.ply")
    open(src, "wb").write(b"not a ply file")  # never read: the options are refused first
    for bad in ("x", "0", "-1", "inf", "nan"):
        assert asrtool.main(["--in", src, "--out", str(tmp_path / "out.ply"), "--thin", bad]) == 1
        assert "--thin" in capsys.readouterr().err
    assert asrtool.main(["--in", src, "--out", str(tmp_path / "out.ply"), "--thin"]) == 1
    assert asrtool.main(["--thin-cloud", src, str(tmp_path / "out.ply")]) == 1
    assert "--cell" in capsys.readouterr().err
    assert asrtool.main(["--thin-cloud", src, str(tmp_path / "out.ply"), "--cell", "0"]) == 1
    assert asrtool.main(["--thin-cloud", src, "--cell", "0.1"]) == 1
    assert asrtool.main(["--thin-cloud", str(tmp_path / "missing.ply"), str(tmp_path / "out.ply"), "--cell", "0.1"]) == 1
    assert "no such file" in capsys.readouterr().err
    assert asrtool.main(["--thin-cloud", src, str(tmp_path / "out.ply"), "--cell", "0.1"]) == 1  # not a PLY file
    assert not os.path.exists(str(tmp_path / "out.ply"))
    assert asrtool.HELP.startswith("usage: asrtool --in point_cloud.ply --out mesh.ply\n")
    assert "--thin SIZE" in asrtool.HELP and "--thin-cloud IN.ply OUT.ply --cell SIZE" in asrtool.HELP


# ---- 3. the restatement -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan():
    return P.scan_case()


def _check_sums(n, res):
    m = len(res["points"])
    assert res["report"]["clusters"] == m == len(res["counts"]) == len(res["keys"])
    assert int(res["counts"].sum()) == n - res["report"]["dropped"] == int((res["cluster"] >= 0).sum())
    assert res["report"]["largest_cluster"] == (int(res["counts"].max()) if m else 0)
    assert np.array_equal(np.bincount(res["cluster"][res["cluster"] >= 0], minlength=m), res["counts"])
    order = res["keys"].astype(np.float64) * 2 + res["sides"]  # (keys of these frames stay far below 2^52)
    assert np.all(np.diff(order) > 0)


def test_counts_order_and_boxes_on_the_scan(scan):
    frame, pts, nrm, rad, att, level = scan
    for kwargs in (dict(level=level), dict(level=level, split_sides=True),
                   dict(levels=P.radius_levels(frame, rad, 0.5)), dict(levels=P.radius_levels(frame, rad, 0.5), split_sides=True)):
        res = P.merge(frame, pts, nrm, rad, att, **kwargs)
        _check_sums(len(pts), res)
        assert res["report"]["dropped"] == 0
        share = float(np.isin(res["counts"], np.arange(2, 11)).mean())
        print(sorted(kwargs), res["report"], "clusters of 2..10 members: %.0f %%" % (100 * share),
              "normals left out: %d" % int((~res["normal_ok"]).sum()))
        if "level" in kwargs:
            assert share > 0.5  # "most clusters have 2-10 members"
        assert (~res["normal_ok"]).mean() <= 0.01
        lo, hi = P.boxes(frame, pts, kwargs.get("level", kwargs.get("levels")), res)
        tol = 2.0 ** -22 * np.maximum(np.abs(lo), np.abs(hi))
        assert np.all(res["points"] >= lo - tol) and np.all(res["points"] <= hi + tol)
        assert np.all(res["radii"] >= rad.min()) and np.all(res["radii"] <= rad.max())
        assert res["attributes"].shape == (len(res["points"]), 3)
        length = np.sqrt((res["normals"].astype(np.float64) ** 2).sum(1))
        assert np.all(np.abs(length[res["normal_ok"]] - 1) < 1e-6)
    levels = P.radius_levels(frame, rad, 0.5)
    assert len(np.unique(levels)) >= 2 and np.array_equal(np.unique(res["levels"]), np.unique(levels))


def test_level_21_is_the_input_in_key_order(scan):
    frame, pts, nrm, rad, att, _ = scan
    lv = np.full(len(pts), 21)
    _, key = R.vertex_cells(frame, pts, lv)
    _, first = np.unique(key, return_index=True)  # one point per cell: distinct cells
    first = np.sort(first)
    p, q, r, a = pts[first], nrm[first], rad[first], att[first]
    for split in (False, True):
        res = P.merge(frame, p, q, r, a, level=21, split_sides=split)
        order = np.argsort(key[first], kind="stable")
        assert res["report"] == dict(clusters=len(p), dropped=0, largest_cluster=1, split_cells=0)
        assert np.array_equal(_bits(res["points"]), _bits(p[order])) and np.array_equal(_bits(res["normals"]), _bits(q[order]))
        assert np.array_equal(_bits(res["radii"]), _bits(r[order])) and np.array_equal(_bits(res["attributes"]), _bits(a[order]))
        assert np.array_equal(res["cluster"][order], np.arange(len(p)))


def test_thin_wall_sides():
    frame, pts, nrm, level = P.thin_wall()
    both = P.merge(frame, pts, nrm, level=level, split_sides=True)
    one = P.merge(frame, pts, nrm, level=level)
    _check_sums(len(pts), both)
    _check_sums(len(pts), one)
    assert one["report"] == dict(clusters=36, dropped=0, largest_cluster=13, split_cells=0)
    assert both["report"] == dict(clusters=72, dropped=0, largest_cluster=9, split_cells=36)
    assert np.array_equal(both["keys"][0::2], one["keys"]) and np.array_equal(both["keys"][1::2], one["keys"])
    assert np.array_equal(both["sides"], np.tile([0, 1], 36))
    assert sorted(np.unique(both["counts"]).tolist()) == [4, 9] and np.all(both["counts"][0::2] + both["counts"][1::2] == 13)
    # the two clusters of a cell are the two sheets: normals +-z, 0.2 cells apart
    up = both["normals"][:, 2] > 0
    assert np.all(np.abs(both["normals"][:, 2]) == 1) and up.sum() == 36
    assert np.all((both["counts"] == 9) == up)
    h = float(frame.voxel_size[level])
    gap = np.abs(both["points"][0::2, 2] - both["points"][1::2, 2])
    assert np.allclose(gap, 0.2 * h, rtol=1e-4)
    # unsplit, the sheets are averaged: the normal sum (9 - 4) z is kept, the position lies between them
    assert np.all(one["normals"][:, 2] == 1) and one["normal_ok"].all() and both["normal_ok"].all()
    # a zero normal in front: nothing of that cell is on side 1
    frame, pts, nrm, level = P.thin_wall(zero_first=True)
    res = P.merge(frame, pts, nrm, level=level, split_sides=True)
    assert res["report"] == dict(clusters=71, dropped=0, largest_cluster=13, split_cells=35)
    c = res["cluster"][0]
    assert res["counts"][c] == 13 and res["sides"][c] == 0 and res["normal_ok"].all()


def test_dropped_points_and_empty_results():
    frame, pts, nrm, rad, att = P.sized_clusters([1, 2, 5])
    bad = pts.copy()
    bad[1] = np.nan
    bad[3, 1] = np.inf
    bad[4] = [1e30, 0.5, 0.5]
    bad[6] = [-3.0, 0.5, 0.5]  # finite and outside the root cube of the unit box
    res = P.merge(frame, bad, nrm, rad, att, level=4)
    _check_sums(len(pts), res)
    assert res["report"]["dropped"] == 4 and np.array_equal(np.nonzero(res["cluster"] < 0)[0], [1, 3, 4, 6])
    nothing = P.merge(frame, np.full((7, 3), np.nan, np.float32), nrm[:7], rad[:7], att[:7], level=4, split_sides=True)
    assert nothing["report"] == dict(clusters=0, dropped=7, largest_cluster=0, split_cells=0)
    assert nothing["points"].shape == (0, 3) and nothing["attributes"].shape == (0, 3) and np.all(nothing["cluster"] == -1)
    empty = P.merge(frame, np.zeros((0, 3), np.float32), level=0)
    assert empty["report"] == dict(clusters=0, dropped=0, largest_cluster=0, split_cells=0) and len(empty["cluster"]) == 0
    # non-finite radii, normals and attributes propagate into their cluster and drop nothing
    rad2, att2, nrm2 = rad.copy(), att.copy(), nrm.copy()
    rad2[0], att2[2, 1], nrm2[5, 0] = np.nan, np.inf, np.inf
    res2 = P.merge(frame, pts, nrm2, rad2, att2, level=4)
    assert res2["report"]["dropped"] == 0
    assert np.isnan(res2["radii"][res2["cluster"][0]]) and np.isinf(res2["attributes"][res2["cluster"][2], 1])
    c = res2["cluster"][5]  # no finite length: the first member's normal, bit for bit
    first = int(np.nonzero(res2["cluster"] == c)[0][0])
    assert np.array_equal(_bits(res2["normals"][c]), _bits(nrm2[first]))


def test_sized_clusters_and_the_cap_on_left_out_normals():
    sizes = [1, 2, T - 1, T, T + 1, 4 * T + 3]
    frame, pts, nrm, rad, att = P.sized_clusters(sizes)
    res = P.merge(frame, pts, nrm, rad, att, level=4, split_sides=True)
    _check_sums(len(pts), res)
    assert sorted(res["counts"].tolist()) == sizes and res["report"]["split_cells"] == 0 and res["normal_ok"].all()
    one = P.one_cell_cloud(2000)
    res = P.merge(*one, level=0)
    assert res["report"] == dict(clusters=1, dropped=0, largest_cluster=2000, split_cells=0) and res["normal_ok"].all()
    exact = np.array([np.float32(np.sum(one[1][:, a].astype(np.longdouble)) / 2000) for a in range(3)])
    assert P.ulp_distance(res["points"][0], exact).max() <= 1
    # ulp_distance itself
    x = np.float32(1.0)
    assert P.ulp_distance([x, -0.0, np.nan, x], [np.nextafter(x, np.float32(2)), 0.0, np.nan, np.nan]).tolist()[:3] == [1, 0, 0]
    assert P.ulp_distance([x], [np.nan])[0] > 1 << 30
