"""Global registration without a GPU: the ABI of asr_hip_point_fpfh / _feature_match / _ransac_transform, the numpy
restatement of their contracts (tests/global_register_ref.py) on inputs with a known answer -- it is what
tests/test_gpu_global_register.py holds the kernels to -- and the argument checks of every layer above that need no
device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import global_register_ref as G
import register_ref as R
from asr_hip import _lib, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the ABI -------------------------------------------------------------------------------------------------------
def test_exports_struct_sizes_and_the_theta_table():
    header = open(os.path.join(REPO, "include", "asr_hip.h")).read()
    lib = _lib.load()
    for name in ("asr_hip_point_fpfh", "asr_hip_feature_match", "asr_hip_ransac_transform"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.asr_hip_struct_size(b"asr_ransac_params") == 32 == ctypes.sizeof(_lib.RansacParams)
    assert lib.asr_hip_struct_size(b"asr_ransac_report") == 24 == ctypes.sizeof(_lib.RansacReport)
    assert tuple(n for n, _ in _lib.RansacReport._fields_) == ops.RANSAC_REPORT
    # without a context nothing runs
    assert lib.asr_hip_point_fpfh(None, None, None, 0, None, 3, None, None, None) == 1
    assert lib.asr_hip_feature_match(None, None, 0, None, 0, 1, None, None) == 1
    assert lib.asr_hip_ransac_transform(None, None, 0, None, 0, None, 0, None, None, None) == 1
    # the count/fill comment of the header names the entry points that recycle the scratch arena
    rule = header[:header.index("#ifndef ASR_HIP_H")]
    assert "point_fpfh" in rule and "feature_match" in rule and "ransac_transform" in rule
    # one table: the header's literals are the restatement's, and both are cos / sin of the borders to 17 digits
    body = header[header.index("#define ASR_FPFH_THETA_TABLE"):]
    body = body[:body.index("/*")]
    literals = re.findall(r"\{(-?[0-9.]+), (-?[0-9.]+)\}", body)
    assert len(literals) == 10
    for b, (c, s) in enumerate(literals, 1):
        assert (float(c), float(s)) == G.THETA_TABLE[b - 1]
        beta = -math.pi + 2.0 * math.pi * b / 11
        assert c == "%.17g" % math.cos(beta) and s == "%.17g" % math.sin(beta)
    assert ops.FPFH_DIM == G.FPFH_DIM == 33
    tile = re.search(r"#define ASR_FEATURE_MATCH_TILE (\d+)",
                     open(os.path.join(REPO, "adaptive-surface-reconstruction_amd", "csrc", "asr_common.h")).read())
    assert int(tile.group(1)) == ops.FEATURE_MATCH_TILE


FEATURES_OBJ = os.path.join(REPO, "adaptive-surface-reconstruction_amd", "csrc", "asr_features.o")


def test_kernels_use_no_scratch_memory():
    """no array indexed by a bin or a lane went to scratch memory, nothing spills; the match keeps its row in registers
    and four workgroups of it fit a CU (128 registers, 40 KB of LDS)"""
    import sys
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import kernel_regs
    _lib.load()  # (fails first when nothing has been built)
    assert os.path.exists(FEATURES_OBJ), "the library is there but asr_features.o, which this test reads, is not"
    ks = {k["demangled"]: k for k in kernel_regs.kernels(FEATURES_OBJ) if k["demangled"].startswith("k_")}
    assert {"k_spfh", "k_fpfh", "k_feature_match<33, true>", "k_feature_match<16, false>", "k_feature_match<64, false>",
            "k_ransac_gather", "k_ransac_survivors", "k_ransac_score", "k_ransac_best", "k_ransac_result"} <= set(ks)
    for name, k in ks.items():
        assert k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, (name, k)
        assert k.get("vgpr_count", 0) + k.get("agpr_count", 0) <= 128, (name, k)
        assert k.get("group_segment_fixed_size", 0) <= 40960, (name, k)
    assert ks["k_spfh"].get("group_segment_fixed_size", 0) == 0 and ks["k_fpfh"].get("group_segment_fixed_size", 0) == 0


# ---- 2. the restatement ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    return {partial: G.bumpy_pair(partial) for partial in (False, True)}


def test_theta_rule_equals_atan2_binning(pairs):
    cloud, normals, _, _, _ = pairs[False]  # the 3000-point cloud: 72 000 slots, 69 000 of them pairs
    f = G.pair_features(cloud, normals, G.knn_brute(cloud, 24))
    v = f["valid"]
    assert len(cloud) == 3000 and v.sum() > 68000
    angle = np.arctan2(f["y"][v], f["x"][v])
    want = np.clip(np.floor(11.0 * (angle + np.pi) / (2.0 * np.pi)), 0, 10).astype(np.int32)
    assert np.array_equal(G.theta_bin(f["x"][v], f["y"][v]), want)
    # the borders themselves, reached from inside a bin: beta_b belongs to bin b
    for b in range(1, 11):
        c, s = G.THETA_TABLE[b - 1]
        for eps, bin_ in ((1e-9, b), (-1e-9, b - 1)):
            beta = -math.pi + 2.0 * math.pi * b / 11 + eps
            assert G.theta_bin(np.array([math.cos(beta)]), np.array([math.sin(beta)]))[0] == bin_


def test_histograms_are_normalised_and_rigid_motion_keeps_them(pairs):
    source, sn, target, tn, truth = pairs[False]
    idx = G.knn_brute(target, 16)
    fpfh, spfh, ok = G.point_fpfh(target, tn, idx)
    assert ok.all() and fpfh.dtype == np.float32 and fpfh.shape == (len(target), 33)
    for part in range(3):
        assert np.abs(spfh[:, 11 * part:11 * part + 11].sum(1) - 100.0).max() < 1e-3
        assert np.abs(fpfh[:, 11 * part:11 * part + 11].sum(1) - 200.0).max() < 1e-3
    # a moved copy of the cloud has the same lists and, up to the rounding of the motion, the same descriptors
    moved = R.transform_f32(truth, target)
    n64 = tn.astype(np.float64)
    mn = ((truth[:, 0] * n64[:, 0:1] + truth[:, 1] * n64[:, 1:2]) + truth[:, 2] * n64[:, 2:3]).astype(np.float32)
    again = G.point_fpfh(moved, mn, idx)[0]
    assert np.median(np.abs(again - fpfh).max(1)) < 1e-3
    # degenerate rows: a zero normal, a NaN normal, a row of -1, a neighbour stacked along the normal
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 2]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 0], [np.nan, 0, 1], [0, 0, 1], [0, 0, 3]], np.float32)
    index = np.array([[1, 2, 3, 4], [0, 2, 3, 4], [-1, -1, -1, -1], [0, 4, -1, 3], [3, 0, 0, -1]], np.int32)
    fpfh, spfh, ok = G.point_fpfh(pts, nrm, index)
    assert not ok.any()  # points 1 and 2 have no normal; every other pair is stacked along the normals: |d x u| = 0
    assert not fpfh.any() and not spfh.any()
    with pytest.raises(ValueError):
        G.point_fpfh(pts, nrm, np.full((5, 3), 5, np.int32))


def test_feature_match_restatement():
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=(40, 7)).astype(np.float32), rng.normal(size=(90, 7)).astype(np.float32)
    b[50] = b[20]  # a duplicate: the smaller row wins
    a[3] = b[50]
    a[5, 2] = np.nan
    b[7, 0] = np.inf
    a[9] = b[7]
    index, sq = G.feature_match(a, b)
    with np.errstate(invalid="ignore"):
        d = ((a[:, None, :].astype(np.float64) - b[None].astype(np.float64)) ** 2).sum(2)
    d[:, 7] = np.inf
    want = np.where(np.isnan(d), np.inf, d).argmin(1)
    rows = np.array([r for r in range(40) if r not in (5, 9)])
    assert np.array_equal(index[rows], want[rows]) and index[3] == 20 and sq[3] == 0.0
    assert index[5] == -1 and sq[5] == np.inf and index[9] == -1
    assert np.abs(sq[rows] - d[rows, want[rows]]).max() < 1e-5
    none, far = G.feature_match(a, np.full((4, 7), np.nan, np.float32))
    assert (none == -1).all() and np.isinf(far).all()
    corr, every = G.mutual_pairs(b[:30], b[:30])
    assert np.array_equal(corr[:, 0], corr[:, 1]) and len(every) == 29  # row 7 is not finite


def test_ransac_restatement_on_exact_pairs():
    rng = np.random.default_rng(5)
    target = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    truth = R.motion(75, 0.4)
    source = R.transform_f32(R.inverse(truth), target)
    corr = np.stack([np.arange(200), np.arange(200)], 1).astype(np.int32)
    corr[100:, 1] = rng.permutation(200)[:100]  # half of them wrong
    # splitmix64's published sequence from seed 0: hypothesis 0 draws its first three values
    for r, z in enumerate((0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)):
        assert G.splitmix_draw(0, np.arange(1), r, 1 << 20)[0] == z >> 44
    t, report = G.ransac_transform(source, target, corr, 0.01, 0.9, 2000, 7)
    assert report["evaluated"] > 0 and report["inliers"] >= 100 and 0 <= report["best_hypothesis"] < 2000
    assert np.abs(t - truth).max() < 1e-4
    assert G.rotation_angle(t, truth) < 0.01
    again = G.ransac_transform(source, target, corr, 0.01, 0.9, 2000, 7)
    assert np.array_equal(again[0], t) and again[1] == report
    # source points in a cluster a thousand times smaller than the target's: no triple has edges within the ratio
    t, report = G.ransac_transform(source * np.float32(1e-3), target, corr, 0.01, 0.9, 500, 1)
    assert t is None and report == {"evaluated": 0, "best_hypothesis": -1, "inliers": 0}
    with pytest.raises(ValueError):
        G.ransac_transform(source, target, np.array([[0, 0], [1, 1], [2, 200]]), 0.01)


@pytest.mark.parametrize("partial", (False, True), ids=("full", "partial"))
def test_reference_chain_recovers_the_motion(pairs, partial):
    """140 degrees about (0.3, 0.5, 0.8) plus (1, -0.5, 0.33): far outside ICP's basin.  The search's result is inside it:
    refined by the ICP restatement it arrives where that arrives from the true motion.  No angle is fixed in advance."""
    source, sn, target, tn, truth = pairs[partial]
    start, _ = R.driver(target, tn, source, np.zeros(3), 0.1, 5)
    assert G.rotation_angle(start, truth) > 90.0  # the local method alone does not get there
    t, report, corr = G.global_search(source, sn, target, tn, 48, 0.08, 50000, 1)
    print("partial %s: %s, angle to the truth %.3f deg" % (partial, report, G.rotation_angle(t, truth)))
    assert report["mutual_used"] and report["evaluated"] > 0 and report["inliers"] >= 3
    refined, rep = R.driver(target, tn, source, np.zeros(3), 0.1, 50, init=t)
    want, wrep = R.driver(target, tn, source, np.zeros(3), 0.1, 50, init=truth)
    print("refined %s\nfrom the truth %s\nmax |difference| %.3e" % (rep, wrep, np.abs(refined - want).max()))
    assert rep["converged"] and wrep["converged"]
    # both runs stop after an update below 1e-7 (radians, and units of a cloud of extent 2), and a point-to-plane step
    # near its fixed point leaves at most a tenth of the update it made: each run ends within 1e-8 of the fixed point,
    # two runs within 2e-8 of each other
    assert np.abs(refined - want).max() < 2e-8
    assert rep["pairs"] == wrep["pairs"]


# ---- 3. argument checks ----------------------------------------------------------------------------------------------
def test_argument_checks_need_no_device():
    p, nrm = torch.zeros((10, 3)), torch.ones((10, 3))
    idx = torch.zeros((10, 8), dtype=torch.int32)
    assert ops.check_point_fpfh_arguments(p, nrm, idx) == (10, 8)
    for args in ((torch.zeros((10, 2)), nrm, idx), (p, torch.ones((9, 3)), idx), (p, nrm, torch.zeros((9, 8))),
                 (p, nrm, torch.zeros((10, 2))), (p, nrm, torch.zeros((10, 65))), (p, nrm, torch.zeros(80)),
                 (p, torch.ones(30), idx)):
        with pytest.raises(ValueError):
            ops.check_point_fpfh_arguments(*args)
        with pytest.raises(ValueError):
            ops.point_fpfh(*args)
    a, b = torch.zeros((5, 33)), torch.zeros((7, 33))
    assert ops.check_feature_match_arguments(a, b) == (5, 7, 33)
    assert ops.check_feature_match_arguments(torch.zeros((0, 4)), torch.zeros((1, 4))) == (0, 1, 4)
    for args in ((a, torch.zeros((7, 32))), (a, torch.zeros((0, 33))), (torch.zeros((5, 65)), torch.zeros((7, 65))),
                 (torch.zeros((5, 0)), torch.zeros((7, 0))), (torch.zeros(33), b), (a, torch.zeros((7, 33, 1)))):
        with pytest.raises(ValueError):
            ops.check_feature_match_arguments(*args)
        with pytest.raises(ValueError):
            ops.feature_match(*args)
    corr = torch.zeros((3, 2), dtype=torch.int32)
    assert ops.check_ransac_arguments(p, p, corr, 0.5) == (10, 10, 3)
    for args, kwargs in (((torch.zeros((10, 2)), p, corr, 0.5), {}), ((p, torch.zeros((0, 3)), corr, 0.5), {}),
                         ((p, p, torch.zeros((2, 2)), 0.5), {}), ((p, p, torch.zeros((3, 3)), 0.5), {}),
                         ((p, p, torch.zeros(6), 0.5), {}),
                         ((p, p, corr, 0.0), {}), ((p, p, corr, -1.0), {}), ((p, p, corr, float("nan")), {}),
                         ((p, p, corr, float("inf")), {}), ((p, p, corr, 1e-50), {}), ((p, p, corr, "far"), {}),
                         ((p, p, corr, 0.5), dict(edge_ratio=0.0)), ((p, p, corr, 0.5), dict(edge_ratio=1.5)),
                         ((p, p, corr, 0.5), dict(edge_ratio=float("nan"))), ((p, p, corr, 0.5), dict(edge_ratio="x")),
                         ((p, p, corr, 0.5), dict(hypotheses=0)), ((p, p, corr, 0.5), dict(hypotheses=2 ** 24 + 1)),
                         ((p, p, corr, 0.5), dict(hypotheses=2.5)), ((p, p, corr, 0.5), dict(hypotheses=True)),
                         ((p, p, corr, 0.5), dict(seed=-1)), ((p, p, corr, 0.5), dict(seed=2 ** 64)),
                         ((p, p, corr, 0.5), dict(seed=0.5))):
        with pytest.raises(ValueError):
            ops.check_ransac_arguments(*args, **kwargs)
        with pytest.raises(ValueError):
            ops.ransac_transform(*args, **kwargs)
    assert ops.check_ransac_arguments(p, p, corr, 0.5, 1.0, 2 ** 24, 2 ** 64 - 1) == (10, 10, 3)
    assert ops.check_global_register_arguments(p, p) == (10, 10)
    for args, kwargs in (((torch.zeros((10, 2)), p), {}), ((p, torch.zeros((2, 3))), {}), ((torch.zeros(30), p), {}),
                         ((p, p), dict(source_normals=torch.ones((9, 3)))), ((p, p), dict(target_normals=torch.ones(30))),
                         ((p, p), dict(voxel_size=0.0)), ((p, p), dict(voxel_size=float("nan"))),
                         ((p, p), dict(voxel_size="fine")), ((p, p), dict(max_distance=-1.0)),
                         ((p, p), dict(max_distance=float("inf"))),
                         ((p, p), dict(feature_k=2)), ((p, p), dict(feature_k=65)), ((p, p), dict(feature_k=7.5)),
                         ((p, p), dict(hypotheses=0)), ((p, p), dict(hypotheses=2 ** 24 + 1)), ((p, p), dict(seed=-3))):
        with pytest.raises(ValueError):
            ops.check_global_register_arguments(*args, **kwargs)
    # the operators refuse host tensors: no CPU fallback
    with pytest.raises(_lib.AsrHipError):
        ops.point_fpfh(p, nrm, idx)
    with pytest.raises(_lib.AsrHipError):
        ops.feature_match(a, b)
    with pytest.raises(_lib.AsrHipError):
        ops.ransac_transform(p, p, corr, 0.5)


def test_public_argument_checks_need_no_device():
    import adaptivesurfacereconstruction as asr
    src, tgt = np.zeros((4, 3), np.float32), np.zeros((9, 3), np.float32)
    tgt[:, 0] = np.arange(9)
    for args, kwargs in (((np.zeros((4, 2), np.float32), tgt), {}), ((src, np.zeros((2, 3), np.float32)), {}),
                         ((src, tgt), dict(source_normals=np.ones((5, 3), np.float32))),
                         ((src, tgt), dict(target_normals=np.ones((9, 2), np.float32))),
                         ((src, tgt), dict(voxel_size=0.0)), ((src, tgt), dict(voxel_size=-1.0)),
                         ((src, tgt), dict(max_distance=0.0)), ((src, tgt), dict(feature_k=2)),
                         ((src, tgt), dict(feature_k=100)), ((src, tgt), dict(hypotheses=0)),
                         ((src, tgt), dict(hypotheses=2 ** 24 + 1)), ((src, tgt), dict(seed=-1)),
                         ((src, np.full((9, 3), np.nan, np.float32)), {}),
                         ((src, np.ones((9, 3), np.float32)), {})):  # a bounding box that is a point, no voxel_size
        with pytest.raises(ValueError):
            asr.register_points_global(*args, **kwargs)


def test_asrtool_refuses_bad_global_register_arguments(tmp_path, capsys):
    import asrtool
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    open(src, "wb").write(b"not a ply file")  # never read: the options are refused first
    assert asrtool.main(["--register", src, src, "--global"]) == 1
    assert "three files" in capsys.readouterr().err
    for bad in ("x", "0", "-1", "inf", "nan"):
        assert asrtool.main(["--register", src, src, out, "--global", "--voxel", bad]) == 1
        assert "--voxel" in capsys.readouterr().err
    for bad in ("x", "0", "16777217", "2.5"):
        assert asrtool.main(["--register", src, src, out, "--global", "--hypotheses", bad]) == 1
        assert "--hypotheses" in capsys.readouterr().err
    for bad in ("x", "-1", "18446744073709551616", "0.5"):
        assert asrtool.main(["--register", src, src, out, "--global", "--seed", bad]) == 1
        assert "--seed" in capsys.readouterr().err
    for bad in ("x", "0"):
        assert asrtool.main(["--register", src, src, out, "--global", "--max-distance", bad]) == 1
        assert "--max-distance" in capsys.readouterr().err
    assert asrtool.main(["--register", src, src, out, "--global", "--point-to-point"]) == 1
    assert "--point-to-point does not apply" in capsys.readouterr().err
    assert asrtool.main(["--register", src, src, out, "--global", "--iterations", "5"]) == 1
    assert "--iterations does not apply" in capsys.readouterr().err
    assert asrtool.main(["--register", str(tmp_path / "missing.ply"), src, out, "--global"]) == 1
    assert "no such file" in capsys.readouterr().err
    assert asrtool.main(["--register", src, src, out, "--global"]) == 1  # not a PLY file
    assert "cannot read" in capsys.readouterr().err
    from asr_hip import ply
    two = str(tmp_path / "two.ply")
    ply.write_points(two, np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32))
    assert asrtool.main(["--register", two, two, out, "--global"]) == 1
    assert "at least 3 points" in capsys.readouterr().err
    assert not os.path.exists(out)
    assert "--global" in asrtool.HELP and "--voxel S" in asrtool.HELP and "--hypotheses N" in asrtool.HELP
