"""Surface-comparison metrics without a GPU: the pure reduction asr_hip.metrics.from_distances on hand-made arrays, the
PLY reader of `asrtool --compare`, and the command line's argument handling.

Worked example (all values exact in binary):
    sq_ab = [0, 0.25, 1, 4]      d_ab = [0, 0.5, 1, 2]     accuracy     = 3.5 / 4 = 0.875
    sq_ba = [0.0625, 0.5625]     d_ba = [0.25, 0.75]       completeness = 1 / 2   = 0.5
    chamfer_l1 = (0.875 + 0.5) / 2 = 0.6875
    chamfer_l2 = (5.25 / 4 + 0.625 / 2) / 2 = (1.3125 + 0.3125) / 2 = 0.8125
    hausdorff  = 2
    t = 0.5   (t*t = 0.25):     sq_ab < 0.25 -> {0}: P = 1/4 (0.25 itself is NOT below: strict <);
                                sq_ba < 0.25 -> {0.0625}: R = 1/2;  F = 2 (1/4)(1/2) / (3/4) = 1/3
    t = 0.125 (t*t = 0.015625): P = 1/4, R = 0, F = 0
    t = 4:                      P = R = F = 1
    dots_ab = [1, -1, 0.5, -0.5], dots_ba = [0.25, -0.75]: normal_consistency = (0.75 + 0.5) / 2 = 0.625
"""
import json
import os

import numpy as np
import pytest
import torch

import asrtool
from asr_hip import metrics, ply


def test_from_distances_worked_example():
    sq_ab = np.array([0, 0.25, 1, 4], np.float32)
    sq_ba = np.array([0.0625, 0.5625], np.float32)
    m = metrics.from_distances(sq_ab, sq_ba, (0.5, 0.125, 4.0), dots_ab=[1, -1, 0.5, -0.5], dots_ba=[0.25, -0.75])
    assert m["accuracy"] == 0.875 and m["completeness"] == 0.5
    assert m["chamfer_l1"] == 0.6875 and m["chamfer_l2"] == 0.8125 and m["hausdorff"] == 2.0
    assert m["thresholds"] == [0.5, 0.125, 4.0]
    assert m["precision"] == [0.25, 0.25, 1.0]
    assert m["recall"] == [0.5, 0.0, 1.0]
    assert m["fscore"] == [2 * 0.25 * 0.5 / 0.75, 0.0, 1.0]
    assert m["normal_consistency"] == 0.625
    assert all(isinstance(v, float) for k, v in m.items() if not isinstance(v, list))
    json.dumps(m)  # plain Python numbers
    # torch tensors give the same numbers, and without normals there is no normal consistency
    m2 = metrics.from_distances(torch.from_numpy(sq_ab), torch.from_numpy(sq_ba), (0.5, 0.125, 4.0))
    assert "normal_consistency" not in m2
    assert {k: v for k, v in m.items() if k != "normal_consistency"} == m2


def test_fscore_is_zero_when_nothing_is_within_the_threshold():
    m = metrics.from_distances(np.array([1, 4], np.float32), np.array([9], np.float32), (0.5,))
    assert m["precision"] == [0.0] and m["recall"] == [0.0] and m["fscore"] == [0.0]


def test_threshold_is_the_f32_square_and_strict():
    """precision counts sq < f32(t) * f32(t): a squared distance equal to that f32 product is out, the next f32 below is in"""
    t2 = np.float32(0.1) * np.float32(0.1)
    assert float(t2) != 0.1 * 0.1  # the f32 product is not the double one
    below = np.nextafter(t2, np.float32(0))
    m = metrics.from_distances(np.array([t2, below, below], np.float32), np.array([t2], np.float32), (0.1,))
    assert m["precision"] == [2 / 3] and m["recall"] == [0.0]
    assert m["fscore"] == [0.0]


def test_means_are_taken_in_float64():
    """d = [2^24, 1, 1, 1]: a float32 running sum stays at 2^24; the float64 mean is (2^24 + 3) / 4"""
    sq = np.array([2.0 ** 48, 1, 1, 1], np.float32)
    m = metrics.from_distances(sq, sq, ())
    assert m["accuracy"] == (2.0 ** 24 + 3) / 4 == 4194304.75
    assert m["chamfer_l2"] == (2.0 ** 48 + 3) / 4
    assert m["hausdorff"] == 2.0 ** 24 and m["fscore"] == []


def test_from_distances_rejects_bad_input():
    one = np.ones(3, np.float32)
    with pytest.raises(ValueError):
        metrics.from_distances(np.zeros(0, np.float32), one, (1.0,))
    with pytest.raises(ValueError):
        metrics.from_distances(one, one, (1.0,), dots_ab=one)
    with pytest.raises(ValueError):
        metrics.from_distances(one, one, (1.0,), dots_ab=one, dots_ba=np.ones(2, np.float32))


def test_read_surface_tells_meshes_from_clouds(tmp_path):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32)
    t = np.array([[0, 1, 2]], np.int32)
    n = np.array([[0, 0, 1]] * 3, np.float32)
    for binary in (True, False):
        ply.write_mesh(str(tmp_path / "m.ply"), v, t, binary=binary)
        gv, gt, gn = ply.read_surface(str(tmp_path / "m.ply"))
        assert np.array_equal(gv, v) and np.array_equal(gt, t) and gn is None
        ply.write_points(str(tmp_path / "c.ply"), v, n, binary=binary)
        gv, gt, gn = ply.read_surface(str(tmp_path / "c.ply"))
        assert np.array_equal(gv, v) and gt is None and np.array_equal(gn, n)
    ply.write_mesh(str(tmp_path / "e.ply"), v, np.zeros((0, 3), np.int32))  # a mesh file without faces: a cloud
    gv, gt, gn = ply.read_surface(str(tmp_path / "e.ply"))
    assert np.array_equal(gv, v) and gt is None and gn is None


def test_default_thresholds_follow_the_reference_box():
    import adaptivesurfacereconstruction as asr
    box = np.array([[0, 0, 0], [3, 4, 12]], np.float32)  # diagonal 13
    assert asr.default_thresholds(box) == (0.005 * 13.0, 0.01 * 13.0)


def test_compare_with_a_missing_file_fails_with_a_message(tmp_path, capsys):
    ply.write_mesh(str(tmp_path / "m.ply"), np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32))
    missing = str(tmp_path / "nope.ply")
    for args in (["--compare", str(tmp_path / "m.ply"), missing], ["--compare", missing, str(tmp_path / "m.ply")]):
        assert asrtool.main(args) != 0
        err = capsys.readouterr().err
        assert "no such file" in err and missing in err
    assert asrtool.main(["--compare", str(tmp_path / "m.ply")]) != 0
    assert "two files" in capsys.readouterr().err
    assert asrtool.main(["--compare", str(tmp_path / "m.ply"), str(tmp_path / "m.ply"), "--samples", "many"]) != 0
    assert "--samples" in capsys.readouterr().err
    # the mode is looked at before --in / --out: their presence does not turn it into a reconstruction
    assert asrtool.main(["--compare", missing, missing, "--in", "a.ply", "--out", "b.ply"]) != 0
    assert "no such file" in capsys.readouterr().err


def test_help_lists_the_compare_mode(capsys):
    assert asrtool.main([]) == 1  # as before: no --in / --out prints the usage
    out = capsys.readouterr().out
    assert out == asrtool.HELP
    for word in ("--compare MESH.ply REFERENCE.ply", "--samples", "--thresholds", "--seed", "0.5 % and 1 %"):
        assert word in out
    assert os.path.basename(asrtool.__file__) == "asrtool.py"
