"""Rigid registration without a GPU: the ABI of asr_hip_icp_step / _icp_update / _register_points, the host-only solve
and update (asr_hip_icp_update) against the numpy restatement of the contract (tests/register_ref.py), the argument checks
of every layer above that need no device, and the restatement itself on motions with a known answer -- it is what
tests/test_gpu_register.py holds the kernels to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import register_ref as R
from asr_hip import _lib, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
MOTIONS = ((5, 0.05), (10, 0.1), (20, 0.2))
CAP = 0.3


# ---- 1. the ABI -------------------------------------------------------------------------------------------------------
def test_exports_and_struct_sizes():
    header = open(os.path.join(REPO, "include", "asr_hip.h")).read()
    lib = _lib.load()
    for name in ("asr_hip_icp_step", "asr_hip_icp_update", "asr_hip_register_points"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.asr_hip_struct_size(b"asr_icp_sums") == 8 * 31 == ctypes.sizeof(_lib.IcpSums)
    assert lib.asr_hip_struct_size(b"asr_icp_params") == 24 == ctypes.sizeof(_lib.IcpParams)
    assert lib.asr_hip_struct_size(b"asr_icp_report") == 40 == ctypes.sizeof(_lib.IcpReport)
    assert tuple(n for n, _ in _lib.IcpReport._fields_) == ops.ICP_REPORT
    # without a context nothing runs; the update refuses null arguments
    assert lib.asr_hip_icp_step(None, None, None, 0, None, None, 0, None, None, ctypes.c_float(1), None, None) == 1
    assert lib.asr_hip_register_points(None, None, None, 0, None, None, 0, None, None, None) == 1
    assert lib.asr_hip_icp_update(None, None, None, None) == -1
    # the count/fill comment of the header names the two entry points that recycle the scratch arena
    rule = header[:header.index("#ifndef ASR_HIP_H")]
    assert "icp_step" in rule and "register_points" in rule


# ---- 2. the restatement recovers known motions ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return {m: R.moved_pair(*m) for m in MOTIONS}


@pytest.mark.parametrize("plane", (True, False), ids=("plane", "point"))
@pytest.mark.parametrize("motion", MOTIONS, ids=lambda m: "%ddeg" % m[0])
def test_reference_driver_recovers_the_motion(cases, motion, plane):
    target, normals, source, truth = cases[motion]
    t, report = R.driver(target, normals if plane else None, source, np.zeros(3), CAP, 50 if plane else 200)
    err = R.coordinate_error(t, source, truth)
    print("motion %s plane %s: %s, max coordinate error %.3e" % (motion, plane, report, err))
    assert report["converged"] and not report["degenerate"]
    assert report["pairs"] == len(source) and report["fitness"] == 1.0
    assert report["iterations"] <= (8 if plane else 150)
    # the source is the truth moved in f64 and rounded to f32 once, and once more on the way back: two roundings of
    # coordinates below 2 -> 2 ulp(1) of f32
    assert err <= 2 * 2.0 ** -23
    assert np.abs(t - R.motion(*motion)).max() < 1e-6


def test_tree_pairs_equal_brute_force_pairs(cases):
    target, _, source, _ = cases[MOTIONS[0]]
    for t in (R.identity(), R.motion(3, 0.02)):
        q = R.transform_f32(t, source)
        assert np.array_equal(R.pairs_tree(target, q, 0.05), R.pairs_brute(target, q, 0.05))


# ---- 3. asr_hip_icp_update --------------------------------------------------------------------------------------------
def _ulp_close(a, b, scale=1.0, ulps=4):
    """within `ulps` f64 ulp of the largest operand: the rotation's entries are sums of products of magnitude <= 1, the
    translation Rw (t - o) + v + o adds terms as large as |t - o| and |o| (`scale`), whatever is left after they cancel"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= ulps * EPS * max(1.0, scale)))


@pytest.mark.parametrize("plane", (True, False), ids=("plane", "point"))
@pytest.mark.parametrize("origin", ((0.0, 0.0, 0.0), (0.25, -0.5, 0.125), (1000.0, 1000.0, 1000.0)), ids=("o0", "o1", "far"))
def test_update_solves_the_reference_sums(cases, plane, origin):
    target, normals, source, _ = cases[MOTIONS[1]]
    o = np.array(origin)
    shift = np.float32(origin[0] if origin[0] == 1000.0 else 0.0)  # the far origin comes with a cloud out there
    start = R.motion(2, 0.01)
    start[:, 3] += np.float64(shift) - start[:, :3] @ np.full(3, np.float64(shift))
    sums, _, _ = R.step(target + shift, normals if plane else None, source + shift, start, o, CAP, R.pairs_tree)
    assert sums["pairs"] == len(source)
    got, xi, degenerate = ops.icp_update(sums, o, start)
    assert not degenerate
    a, b = R.matrix(sums), sums["atb"]
    residual = np.abs(a @ xi + b).max()
    bound = 64 * EPS * (np.abs(a).sum(1).max() * np.abs(xi).max() + np.abs(b).max())
    print("plane %s origin %s: |A xi + b| = %.3e, bound %.3e" % (plane, origin, residual, bound))
    assert residual <= bound
    assert _ulp_close(got, R.apply_update(start, xi, o), max(np.abs(o).max(), np.abs(start[:, 3] - o).max()))
    ref_t, ref_xi, _ = R.update(sums, o, start)
    assert np.abs(xi - ref_xi).max() <= 1e-9 * max(1.0, np.abs(ref_xi).max())
    assert np.abs(got - ref_t).max() <= 1e-9 * max(1.0, np.abs(ref_t).max())
    # the structure takes the same sums
    s = _lib.IcpSums()
    s.ata[:], s.atb[:] = list(sums["ata"]), list(sums["atb"])
    s.pairs, s.mode = sums["pairs"], sums["mode"]
    got2, xi2, _ = ops.icp_update(s, o, start)
    assert np.array_equal(got2, got) and np.array_equal(xi2, xi)


def test_update_of_a_tiny_and_a_zero_rotation():
    # A = I, b chosen: xi = -b.  A rotation below 1e-300 is the identity; a translation alone moves t only
    sums = {"ata": [1.0 if i == j else 0.0 for i, j in R.TRIANGLE], "atb": [0, 0, 0, -0.5, 0.25, -2.0],
            "sq_residual": 1.0, "sq_distance": 1.0, "pairs": 10, "mode": 1}
    start = R.motion(30, 0.3)
    got, xi, degenerate = ops.icp_update(sums, (1.0, 2.0, 3.0), start)
    assert not degenerate and np.array_equal(xi, [0, 0, 0, 0.5, -0.25, 2.0])
    assert np.array_equal(got[:, :3], start[:, :3]) and _ulp_close(got[:, 3], start[:, 3] + xi[3:], 4.0)
    sums["atb"] = [-1e-301, 0, 0, 0, 0, 0]
    got, xi, degenerate = ops.icp_update(sums, (0, 0, 0), start)
    assert not degenerate and xi[0] == 1e-301 and np.array_equal(got, start)
    sums["atb"] = [0, 0, -np.pi / 2, 0, 0, 0]  # a quarter turn about z, about the origin (1, 0, 0)
    got, xi, _ = ops.icp_update(sums, (1.0, 0.0, 0.0), R.identity())
    assert np.abs(got - np.array([[0, -1, 0, 1], [1, 0, 0, -1], [0, 0, 1, 0]], np.float64)).max() < 4 * EPS


def test_update_reports_degenerate_systems_and_leaves_the_transform():
    start = R.motion(7, 0.07)
    # a planar target in plane mode: three directions are not constrained, the rank is 3
    rng = np.random.default_rng(5)
    flat = np.concatenate([rng.uniform(-1, 1, (2000, 2)), np.zeros((2000, 1))], 1).astype(np.float32)
    up = np.tile(np.float32([0, 0, 1]), (2000, 1))
    sums, _, _ = R.step(flat, up, flat[:500] + np.float32([0, 0, 0.01]), R.identity(), np.zeros(3), CAP, R.pairs_tree)
    assert sums["pairs"] == 500 and np.linalg.matrix_rank(R.matrix(sums)) == 3
    cases = {"planar": sums,
             "zero": {"ata": np.zeros(21), "atb": np.zeros(6), "sq_residual": 0.0, "sq_distance": 0.0, "pairs": 100, "mode": 1},
             "nan": dict(sums, ata=np.full(21, np.nan))}
    good, _, _ = R.step(*R.moved_pair(5, 0.05)[:3], R.identity(), np.zeros(3), CAP, R.pairs_tree)
    cases["five pairs, plane"] = dict(good, pairs=5)
    cases["two pairs, point"] = dict(good, pairs=2, mode=0)
    for name, s in cases.items():
        got, xi, degenerate = ops.icp_update(s, (0.0, 0.0, 0.0), start)
        assert degenerate, name
        assert np.array_equal(got, start) and not xi.any(), name
    # the same sums with enough pairs are solved; three pairs are enough in point mode
    assert not ops.icp_update(dict(good, pairs=6), (0, 0, 0), start)[2]
    assert not ops.icp_update(dict(good, pairs=3, mode=0), (0, 0, 0), start)[2]


# ---- 4. argument checks that need no device ---------------------------------------------------------------------------
def test_check_register_arguments():
    tgt, src, nrm = torch.zeros((9, 3)), torch.zeros((4, 3)), torch.ones((9, 3))
    n, m, t = ops.check_register_arguments(tgt, nrm, src, 0.5)
    assert (n, m) == (9, 4) and np.array_equal(t, R.identity())
    assert ops.check_register_arguments(tgt, None, torch.zeros((0, 3)), 0.5)[1] == 0
    t44 = np.vstack([R.motion(5, 0.1), [0, 0, 0, 1]])
    assert np.array_equal(ops.check_register_arguments(tgt, None, src, 1, init=t44)[2], R.motion(5, 0.1))
    assert np.array_equal(ops.check_register_arguments(tgt, None, src, 1, init=torch.from_numpy(t44))[2], R.motion(5, 0.1))
    nan_init = R.identity()
    nan_init[1, 3] = np.nan
    bad_row = t44.copy()
    bad_row[3, 0] = 1.0
    for args, kwargs in (((torch.zeros((9, 2)), None, src, 0.5), {}), ((torch.zeros((0, 3)), None, src, 0.5), {}),
                         ((tgt, torch.ones((8, 3)), src, 0.5), {}), ((tgt, nrm, torch.zeros((4, 4)), 0.5), {}),
                         ((tgt, nrm, torch.zeros(12), 0.5), {}),
                         ((tgt, nrm, src, 0.0), {}), ((tgt, nrm, src, -1.0), {}), ((tgt, nrm, src, float("nan")), {}),
                         ((tgt, nrm, src, float("inf")), {}), ((tgt, nrm, src, 1e-50), {}),  # 0 as a float32
                         ((tgt, nrm, src, "far"), {}),
                         ((tgt, nrm, src, 0.5), dict(init=nan_init)), ((tgt, nrm, src, 0.5), dict(init=np.eye(3))),
                         ((tgt, nrm, src, 0.5), dict(init=bad_row)), ((tgt, nrm, src, 0.5), dict(init="identity")),
                         ((tgt, nrm, src, 0.5), dict(max_iterations=0)), ((tgt, nrm, src, 0.5), dict(max_iterations=1001)),
                         ((tgt, nrm, src, 0.5), dict(max_iterations=2.5)), ((tgt, nrm, src, 0.5), dict(max_iterations=True)),
                         ((tgt, nrm, src, 0.5), dict(rotation_tolerance=-1e-9)),
                         ((tgt, nrm, src, 0.5), dict(translation_tolerance=float("nan"))),
                         ((tgt, nrm, src, 0.5), dict(translation_tolerance=None))):
        with pytest.raises(ValueError):
            ops.check_register_arguments(*args, **kwargs)
    # the operators check before they look for a device
    frame = _lib.frame_init([-1, -1, -1], [1, 1, 1])
    with pytest.raises(ValueError):
        ops.icp_step(frame, tgt, nrm, src, R.identity(), (0, 0, 0), -1.0)
    with pytest.raises(ValueError):
        ops.icp_step(frame, tgt, nrm, src, nan_init, (0, 0, 0), 1.0)
    with pytest.raises(ValueError):
        ops.icp_step(frame, tgt, nrm, src, R.identity(), (0, np.inf, 0), 1.0)
    with pytest.raises(ValueError):
        ops.register_points(frame, tgt, nrm, src, 1.0, max_iterations=0)
    with pytest.raises(_lib.AsrHipError):  # and refuse host tensors: no CPU fallback
        ops.icp_step(frame, tgt, nrm, src, R.identity(), (0, 0, 0), 1.0)
    assert ops.icp_origin(frame) == list(R.frame_origin(frame))
    assert np.abs(np.array(ops.icp_origin(frame))).max() < 1e-6  # the cube around [-1, 1]^3 is centred on 0


def test_public_argument_checks_need_no_device():
    import adaptivesurfacereconstruction as asr
    tgt, src = np.zeros((9, 3), np.float32), np.zeros((4, 3), np.float32)
    tgt[:, 0] = np.arange(9)
    bad = tgt.copy()
    bad[3, 1] = np.inf
    nan_init = np.eye(4)
    nan_init[0, 0] = np.nan
    for args, kwargs in (((src, bad), {}), ((src, tgt), dict(max_distance=0.0)), ((src, tgt), dict(max_distance=-2.0)),
                         ((src, tgt), dict(init=nan_init)), ((src, np.zeros((0, 3), np.float32)), {}),
                         ((src, tgt), dict(target_normals=np.ones((8, 3), np.float32))),
                         ((np.zeros((4, 2), np.float32), tgt), {}), ((src, tgt), dict(max_iterations=0))):
        with pytest.raises(ValueError):
            asr.register_points(*args, **kwargs)


def test_transform_points_against_a_direct_f64_evaluation():
    import adaptivesurfacereconstruction as asr
    rng = np.random.default_rng(11)
    p = rng.uniform(-50, 50, (1000, 3)).astype(np.float32)
    nrm = rng.normal(size=(1000, 3)).astype(np.float32)
    t = R.motion(33, 0.7)
    want = (p.astype(np.float64) @ t[:, :3].T + t[:, 3])
    for transform in (t, np.vstack([t, [0, 0, 0, 1]]), torch.from_numpy(t)):
        got, gn = asr.transform_points(p, transform, nrm)
        assert got.dtype == np.float32 and gn.dtype == np.float32
        # one rounding to f32 of a value whose f64 evaluation order may differ in the last f64 bits
        assert np.all(np.abs(got.astype(np.float64) - want) <= 0.5 * np.spacing(np.abs(want).astype(np.float32)) * (1 + 1e-6))
        assert np.abs(gn.astype(np.float64) - nrm.astype(np.float64) @ t[:, :3].T).max() < 1e-6
        assert np.array_equal(got, R.transform_f32(t, p))
    assert np.array_equal(asr.transform_points(p, R.identity()), p)
    with pytest.raises(ValueError):
        asr.transform_points(p, np.eye(3))
    with pytest.raises(ValueError):
        asr.transform_points(p, t, nrm[:10])


def test_asrtool_refuses_bad_register_arguments(tmp_path, capsys):
    import asrtool
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    open(src, "wb").write(b"not a ply file")  # never read: the options are refused first
    assert asrtool.main(["--register", src, src]) == 1
    assert "three files" in capsys.readouterr().err
    assert asrtool.main(["--register", src, src, "--max-distance", "1"]) == 1
    assert "three files" in capsys.readouterr().err
    for bad in ("x", "0", "-1", "inf", "nan"):
        assert asrtool.main(["--register", src, src, out, "--max-distance", bad]) == 1
        assert "--max-distance" in capsys.readouterr().err
    for bad in ("x", "0", "1001", "2.5"):
        assert asrtool.main(["--register", src, src, out, "--iterations", bad]) == 1
        assert "--iterations" in capsys.readouterr().err
    assert asrtool.main(["--register", str(tmp_path / "missing.ply"), src, out]) == 1
    assert "no such file" in capsys.readouterr().err
    assert asrtool.main(["--register", src, src, out]) == 1  # not a PLY file
    assert "cannot read" in capsys.readouterr().err
    assert not os.path.exists(out)
    assert "--register SOURCE.ply TARGET.ply OUT.ply" in asrtool.HELP and "--point-to-point" in asrtool.HELP
