"""Normal estimation without a GPU: the NumPy restatement (tests/normals_ref.py) orients spheres
outward, and every argument check of the new entry points raises before a device is touched (CPU tensors with good
shapes would be refused with AsrHipError; a ValueError therefore comes from the check)."""
import numpy as np
import pytest
import torch

import asrtool
import normals_ref as R
from asr_hip import _lib, ops, ply, synth

FRAME = None  # the checks come before the frame is looked at


def _estimate(points, k):
    idx, _ = R.knn_lists(points, k)
    nrm, _, ok, _, _ = R.point_normals(points, idx)
    out, flips, report = R.orient(points, nrm, idx)
    return out, ok, report


@pytest.mark.parametrize("n,k", [(2000, 12), (500, 8), (4000, 16)])
def test_reference_orients_a_sphere_outward(n, k):
    pts, _ = synth.sphere_cloud(n, seed=1)
    out, ok, report = _estimate(pts, k)
    d = (out.astype(np.float64) * pts).sum(1)
    print("n=%d k=%d: components %d, outward share %.4f, smallest |n.p| %.4f"
          % (n, k, report["components"], (d > 0).mean(), np.abs(d).min()))
    assert ok.all() and report["components"] == 1 and report["skipped"] == 0
    assert (d > 0).all()
    if (n, k) == (2000, 12):
        assert np.abs(d).min() > 0.9


def test_reference_two_spheres_are_two_components():
    pts, centres = R.two_spheres(1000, seed=3)
    out, ok, report = _estimate(pts, 12)
    assert ok.all() and report["components"] == 2
    assert ((out.astype(np.float64) * (pts - centres)).sum(1) > 0).all()


def test_reference_lists_ties_and_padding():
    pts = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, 0]])
    idx, sq = R.knn_lists(pts, 8)
    assert idx[0].tolist() == [0, 4, 1, 2, 3, -1, -1, -1] and idx[4].tolist() == [0, 4, 1, 2, 3, -1, -1, -1]
    assert sq[0].tolist()[:5] == [0, 0, 1, 1, 1] and np.isposinf(sq[:, 5:]).all()
    idx2, _ = R.knn_lists(pts, 2)
    assert idx2.tolist() == [[0, 4], [1, 0], [2, 0], [3, 0], [0, 4]]


def test_reference_orientation_of_a_chain_follows_the_edges():
    n = 50
    pts = np.stack([np.arange(n), np.zeros(n), np.zeros(n)], 1).astype(np.float32)
    rng = np.random.default_rng(0)
    nrm = np.tile(np.float32([0, 0, 1]), (n, 1)) * rng.choice(np.float32([-1, 1]), size=(n, 1))
    idx = np.stack([np.arange(n), np.arange(n) + 1], 1).astype(np.int32)
    idx[-1, 1] = -1
    out, flips, report = R.orient(pts, nrm, idx)
    assert report["components"] == 1 and (out[:, 2] == 1).all() and np.array_equal(flips, nrm[:, 2] < 0)


def test_op_argument_checks_come_before_the_device():
    p = torch.zeros((10, 3))
    with pytest.raises(ValueError):
        ops.knn_index(FRAME, torch.zeros((10, 2)), 4)
    with pytest.raises(ValueError):
        ops.knn_index(FRAME, torch.zeros((0, 3)), 4)
    for k in (0, 65, 2.5, True, "many"):
        with pytest.raises(ValueError):
            ops.knn_index(FRAME, p, k)
    with pytest.raises(ValueError):
        ops.point_normals(torch.zeros(30), torch.zeros((10, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.point_normals(p, torch.zeros((9, 4), dtype=torch.int32))
    for k in (2, 65):
        with pytest.raises(ValueError):
            ops.point_normals(p, torch.zeros((10, k), dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.point_normals(p, torch.zeros(40, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.orient_normals(p, torch.zeros((9, 3)), torch.zeros((10, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.orient_normals(p, p)  # neither lists nor viewpoints
    with pytest.raises(ValueError):
        ops.orient_normals(p, p, torch.zeros((10, 0), dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.orient_normals(p, p, torch.zeros((9, 4), dtype=torch.int32))
    for v in (torch.zeros(2), torch.zeros((9, 3)), torch.zeros((10, 2))):
        with pytest.raises(ValueError):
            ops.orient_normals(p, p, viewpoints=v)
    # good shapes on the CPU: refused like every other op, there is no CPU path
    with pytest.raises(_lib.AsrHipError):
        ops.knn_index(FRAME, p, 4)
    with pytest.raises(_lib.AsrHipError):
        ops.point_normals(p, torch.zeros((10, 4), dtype=torch.int32))
    with pytest.raises(_lib.AsrHipError):
        ops.orient_normals(p, p, viewpoints=torch.zeros(3))


def test_module_argument_checks_come_before_the_device():
    import adaptivesurfacereconstruction as asr
    pts, _ = synth.sphere_cloud(100, seed=2)
    for k in (2, 65, 7.5):
        with pytest.raises(ValueError):
            asr.estimate_normals(pts, k)
        with pytest.raises(ValueError):
            asr.reconstruct_surface(pts, None, normal_k=k, weights={})
    with pytest.raises(ValueError):
        asr.estimate_normals(pts[:, :2], 8)
    bad = pts.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError):
        asr.estimate_normals(bad, 8)
    for v in ([0, 0], np.zeros((99, 3)), [0, np.inf, 0]):
        with pytest.raises(ValueError):
            asr.estimate_normals(pts, 8, viewpoint=v)
        with pytest.raises(ValueError):
            asr.reconstruct_surface(pts, None, viewpoint=v, weights={})
    with pytest.raises(ValueError):
        asr.reconstruct_surface(pts, pts[:50], weights={})  # given normals are still checked


RAW = ("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
       "property float radius\nend_header\n0 0 0 0.5\n1 0 0 0.25\n0 1 0 0.125\n")


def test_read_points_without_normals(tmp_path):
    path = str(tmp_path / "raw.ply")
    with open(path, "w") as f:
        f.write(RAW)
    with pytest.raises(ValueError):
        ply.read_points(path)
    with pytest.raises(ValueError):
        ply.read_points(path, require_normals=True)
    p, n, r = ply.read_points(path, require_normals=False)
    assert n is None and p.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0]] and r.tolist() == [0.5, 0.25, 0.125]
    full = str(tmp_path / "full.ply")
    ply.write_points(full, p, np.float32([[0, 0, 1]] * 3))
    assert ply.read_points(full, require_normals=False)[1].tolist() == [[0, 0, 1]] * 3
    with open(path, "w") as f:
        f.write(RAW.replace("property float z\n", ""))
    with pytest.raises(ValueError):
        ply.read_points(path, require_normals=False)


def test_asrtool_normal_options_fail_before_the_gpu(tmp_path, capsys):
    raw = str(tmp_path / "raw.ply")
    with open(raw, "w") as f:
        f.write(RAW)
    out = str(tmp_path / "out.ply")
    bad = [["--orient-cloud", raw],
           ["--orient-cloud", raw, "--k", "8"],
           ["--orient-cloud", raw, out, "--k", "2"],
           ["--orient-cloud", raw, out, "--k", "65"],
           ["--orient-cloud", raw, out, "--k", "x"],
           ["--orient-cloud", raw, out, "--viewpoint", "1,2"],
           ["--orient-cloud", raw, out, "--viewpoint", "a,b,c"],
           ["--orient-cloud", str(tmp_path / "missing.ply"), out],
           ["--in", raw, "--out", out, "--estimate-normals", "2"],
           ["--in", raw, "--out", out, "--estimate-normals", "lots"],
           ["--in", raw, "--out", out, "--estimate-normals", "8", "--viewpoint", "1;2;3"],
           ["--in", raw, "--out", out, "--viewpoint", "1,2,3"]]
    for argv in bad:
        assert asrtool.main(argv) == 1, argv
        assert capsys.readouterr().err.startswith("asrtool: "), argv
    assert asrtool.HELP.startswith("usage: asrtool --in point_cloud.ply --out mesh.ply\n")
    assert "--estimate-normals" in asrtool.HELP and "--orient-cloud" in asrtool.HELP
