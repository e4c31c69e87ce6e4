"""GPU tests of the normal estimation against its NumPy restatement, tests/normals_ref.py.

knn_index: indices and distance bits array_equal with the brute-force lists, no tolerance.
point_normals: with C the reference's f64 covariance of the row, the Rayleigh quotient of the returned normal exceeds the
  smallest eigenvalue by at most 1e-6 trace(C) and every eigenvalue is within 1e-6 trace(C) of numpy's.  The bound does
  not depend on the eigenvalue gap: an f32 unit vector is off by about 1e-7 rad, which adds about 1e-14 l2 to the
  quotient, while a wrong eigenvector adds l1 - l0, at least 0.03 trace on the spheres used here.
orient_normals: flips, components and skipped array_equal with Kruskal over the same keys."""
import ctypes
import json

import numpy as np
import pytest
import torch

import asrtool
import crowded_inputs
import normals_ref as R
from asr_hip import _lib, ops, ply, synth
from asr_hip._lib import AsrHipError
from stream_helpers import late

pytestmark = pytest.mark.gpu


def frame_of(points, margin=0.1):
    return _lib.frame_init(*synth.bounding_box(np.asarray(points, np.float32), margin))


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# knn_index
# ---------------------------------------------------------------------------------------------------------------------
def check_lists(gpu, points, k, ref=None, frame=None, what=""):
    points = np.ascontiguousarray(points, np.float32)
    frame = frame or frame_of(points)
    idx, sq = ops.knn_index(frame, dev(points, gpu), k)
    assert idx.dtype == torch.int32 and sq.dtype == torch.float32
    assert tuple(idx.shape) == (len(points), k) and tuple(sq.shape) == (len(points), k)
    ref_idx, ref_sq = ref if ref is not None else R.knn_lists(points, k)
    ref_idx, ref_sq = ref_idx[:, :k], ref_sq[:, :k]
    idx, sq = idx.cpu().numpy(), sq.cpu().numpy()
    bad = np.flatnonzero(((idx != ref_idx) | (bits(sq) != bits(ref_sq))).any(1))
    print("%s: n=%d k=%d, %d rows differ%s" % (what, len(points), k, len(bad), "" if not len(bad) else
                                                " (first: row %d, got %r / %r, want %r / %r)"
                                                % (bad[0], idx[bad[0]], sq[bad[0]], ref_idx[bad[0]], ref_sq[bad[0]])))
    assert np.array_equal(idx, ref_idx), what
    assert np.array_equal(bits(sq), bits(ref_sq)), what
    return idx, sq


@pytest.fixture(scope="module")
def uniform():
    pts = np.random.default_rng(11).uniform(-1, 1, size=(3000, 3)).astype(np.float32)
    return pts, R.knn_lists(pts, 64)


@pytest.mark.parametrize("k", [1, 8, 16, 33, 64])
def test_knn_index_uniform(gpu, uniform, k):
    pts, ref = uniform
    idx, sq = check_lists(gpu, pts, k, ref, what="uniform")
    if k == 16:  # the same bits on a second run
        idx2, sq2 = ops.knn_index(frame_of(pts), dev(pts, gpu), k)
        assert np.array_equal(idx2.cpu().numpy(), idx) and np.array_equal(bits(sq2.cpu().numpy()), bits(sq))


@pytest.fixture(scope="module")
def lattice():
    g = np.arange(12, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts = np.ascontiguousarray(pts[np.random.default_rng(12).permutation(len(pts))])
    return pts, R.knn_lists(pts, 27)


@pytest.mark.parametrize("k", [7, 27])
def test_knn_index_lattice_ties(gpu, lattice, k):
    """every row is full of ties: 6 neighbours at distance 1, 12 at sqrt 2, 8 at sqrt 3"""
    pts, ref = lattice
    check_lists(gpu, pts, k, ref, what="12^3 lattice")


def test_knn_index_every_point_twice(gpu):
    p, _ = synth.sphere_cloud(1000, seed=13)
    pts = np.concatenate([p, p]).astype(np.float32)
    idx, _ = check_lists(gpu, pts, 8, what="duplicates")
    assert np.array_equal(idx[:, 0], np.arange(2000) % 1000) and np.array_equal(idx[:, 1], np.arange(2000) % 1000 + 1000)


def test_knn_index_padding(gpu):
    pts = np.random.default_rng(14).normal(size=(5, 3)).astype(np.float32)
    idx, sq = check_lists(gpu, pts, 8, what="n < k")
    assert (idx[:, 5:] == -1).all() and np.isposinf(sq[:, 5:]).all() and (idx[:, :5] >= 0).all()


def test_knn_index_crowded_cell_takes_the_deep_path(gpu):
    """8 sites of 1100 points, each inside one cell of the finest level of the index (level 6 for 8800 points: one below
    the level at which 8^level reaches n): more than the 1024 points above which a point starts its search on a deeper
    level"""
    pts, _, _, box = crowded_inputs.lattice_sites(2, 1100, 6, seed=15)
    assert len(pts) == 8800
    check_lists(gpu, pts, 8, frame=_lib.frame_init(*box), what="crowded cells")


def test_knn_index_refuses_bad_input(gpu):
    frame = _lib.frame_init([-1, -1, -1], [1, 1, 1])
    pts = torch.zeros((4, 3), device=gpu)
    bad = pts.clone()
    bad[2, 1] = float("nan")
    with pytest.raises(AsrHipError):
        ops.knn_index(frame, bad, 3)
    ctx = ops.context(gpu)
    for k in (0, 65):
        with pytest.raises(AsrHipError):
            ctx.call("asr_hip_knn_index", ctypes.byref(frame), _lib.ptr(pts), ctypes.c_int64(4), k, None, None)
    idx, sq = ops.knn_index(frame, pts, 3)  # the context works afterwards
    assert idx.cpu().tolist() == [[0, 1, 2]] * 4 and sq.cpu().tolist() == [[0, 0, 0]] * 4


# ---------------------------------------------------------------------------------------------------------------------
# point_normals
# ---------------------------------------------------------------------------------------------------------------------
class Sphere:
    def __init__(self, n=2000, k=12, seed=1, scale=1.0, centre=(0, 0, 0)):
        p, _ = synth.sphere_cloud(n, seed=seed)
        self.centre = np.float32(centre)
        self.pts = np.ascontiguousarray((p * np.float32(scale) + self.centre).astype(np.float32))
        self.idx, _ = R.knn_lists(self.pts, k)
        self.nrm, self.eig, self.ok, self.C, self.m = R.point_normals(self.pts, self.idx)


@pytest.fixture(scope="module")
def sphere():
    return Sphere()


def check_normals(gpu, pts, idx, what):
    """-> (normals, eigenvalues, ok) of the GPU, checked against the reference by the bounds of the module docstring"""
    nrm, eig, ok = ops.point_normals(dev(pts, gpu), dev(idx, gpu), return_eigenvalues=True, return_ok=True)
    assert nrm.dtype == torch.float32 and eig.dtype == torch.float32 and ok.dtype == torch.bool
    nrm, eig, ok = nrm.cpu().numpy(), eig.cpu().numpy(), ok.cpu().numpy()
    _, ref_eig, ref_ok, C, _ = R.point_normals(pts, idx)
    assert np.array_equal(ok, ref_ok), what
    trace = np.trace(C, axis1=1, axis2=2)
    w = np.linalg.eigvalsh(C)
    n64 = nrm[ok].astype(np.float64)
    len2 = (n64 * n64).sum(1)
    quot = np.einsum("ni,nij,nj->n", n64, C[ok], n64) / len2
    excess = (quot - w[ok, 0]) / trace[ok]
    eig_err = np.abs(eig.astype(np.float64) - w)[ok] / trace[ok, None]
    print("%s: %d rows, %d ok; quotient excess / trace max %.3g, eigenvalue error / trace max %.3g, | |n| - 1 | max %.3g"
          % (what, len(pts), ok.sum(), excess.max(), eig_err.max(), np.abs(np.sqrt(len2) - 1).max()))
    assert (excess <= 1e-6).all(), what
    assert (eig_err <= 1e-6).all(), what
    assert (np.abs(np.sqrt(len2) - 1) <= 1e-6).all(), what
    assert np.array_equal(bits(R.sign_convention(nrm)), bits(nrm)), what
    assert (eig[:, 0] <= eig[:, 1]).all() and (eig[:, 1] <= eig[:, 2]).all()
    assert (nrm[~ok] == 0).all()
    return nrm, eig, ok


def test_point_normals_sphere(gpu, sphere):
    nrm, _, ok = check_normals(gpu, sphere.pts, sphere.idx, "sphere")
    assert ok.all()
    assert (np.abs((nrm * sphere.pts).sum(1)) > 0.9).all()
    again = ops.point_normals(dev(sphere.pts, gpu), dev(sphere.idx, gpu))
    assert np.array_equal(bits(again.cpu().numpy()), bits(nrm))


def test_point_normals_small_sphere_far_from_the_origin(gpu):
    """radius 0.01 around (1000, 1000, 1000): a one-pass E[x^2] - E[x]^2 loses everything here"""
    s = Sphere(scale=0.01, centre=(1000, 1000, 1000))
    nrm, _, ok = check_normals(gpu, s.pts, s.idx, "small far sphere")
    assert ok.all()


def test_point_normals_lattice_plane_is_exact(gpu):
    pts = R.lattice_plane(20, 3.0, seed=2)
    idx, _ = R.knn_lists(pts, 9)
    nrm, eig, ok = check_normals(gpu, pts, idx, "lattice plane")
    assert ok.all() and np.array_equal(nrm, np.tile(np.float32([0, 0, 1]), (len(pts), 1))) and (eig[:, 0] == 0).all()


def test_point_normals_degenerate_rows(gpu):
    t = np.arange(50, dtype=np.float32)
    line = np.stack([t, 2 * t, -t], 1)                      # exactly collinear in f32
    same = np.tile(np.float32([0.5, 0.25, 4]), (10, 1))      # coincident
    pts = np.concatenate([line, same]).astype(np.float32)
    idx = np.full((60, 6), -1, np.int32)
    idx[:50] = (np.arange(50)[:, None] + np.arange(6)[None, :]) % 50
    idx[50:] = 50 + (np.arange(10)[:, None] + np.arange(6)[None, :]) % 10
    idx[3, 2:] = -1    # two valid entries
    idx[4, 1:] = -1    # one
    idx[5, :] = -1     # none
    nrm, eig, ok = ops.point_normals(dev(pts, gpu), dev(idx, gpu), return_eigenvalues=True, return_ok=True)
    assert not ok.any().item() and (nrm == 0).all().item()
    assert (eig[50:] == 0).all().item() and (eig[5] == 0).all().item() and (eig[:3, 2] > 0).all().item()
    assert np.array_equal(ok.cpu().numpy(), R.point_normals(pts, idx)[2])


def test_point_normals_hand_made_lists(gpu):
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(300, 3)).astype(np.float32)
    idx = rng.integers(0, 300, size=(300, 5)).astype(np.int32)
    idx[rng.random(idx.shape) < 0.1] = -1
    check_normals(gpu, pts, idx, "five arbitrary indices")


def test_point_normals_refuses_a_bad_index(gpu, sphere):
    p = dev(sphere.pts, gpu)
    for bad in (len(sphere.pts), -2, 2 ** 31 - 1):
        idx = sphere.idx.copy()
        idx[77, 3] = bad
        with pytest.raises(AsrHipError):
            ops.point_normals(p, dev(idx, gpu))
    nrm = ops.point_normals(p, dev(sphere.idx, gpu))  # the context works afterwards
    assert torch.isfinite(nrm).all().item()


# ---------------------------------------------------------------------------------------------------------------------
# orient_normals
# ---------------------------------------------------------------------------------------------------------------------
def check_orient(gpu, pts, nrm, idx, what):
    out, flips, report = ops.orient_normals(dev(pts, gpu), dev(nrm, gpu), dev(idx, gpu), return_flips=True,
                                            return_report=True)
    ref_out, ref_flips, ref_report = R.orient(pts, nrm, idx)
    out, flips = out.cpu().numpy(), flips.cpu().numpy()
    print("%s: n=%d, report %r, reference %r, %d flips differ" % (what, len(pts), report, ref_report,
                                                                   (flips != ref_flips).sum()))
    assert np.array_equal(flips, ref_flips), what
    assert {k: report[k] for k in ref_report} == ref_report, what
    assert np.array_equal(bits(out), bits(ref_out)), what
    n = max(2, len(pts))
    assert 0 <= report["rounds"] <= int(np.ceil(np.log2(n))) + 1
    return out, flips, report


def test_orient_sphere_outward(gpu, sphere):
    out, _, report = check_orient(gpu, sphere.pts, sphere.nrm, sphere.idx, "sphere")
    assert report["components"] == 1 and ((out * sphere.pts).sum(1) > 0).all()
    again = ops.orient_normals(dev(sphere.pts, gpu), dev(sphere.nrm, gpu), dev(sphere.idx, gpu))
    assert np.array_equal(bits(again.cpu().numpy()), bits(out))


def test_orient_two_spheres(gpu):
    pts, centres = R.two_spheres(1000, seed=3)
    idx, _ = R.knn_lists(pts, 12)
    nrm = R.point_normals(pts, idx)[0]
    out, _, report = check_orient(gpu, pts, nrm, idx, "two spheres")
    assert report["components"] == 2 and ((out * (pts - centres)).sum(1) > 0).all()


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def test_orient_chain_of_5000(gpu):
    n = 5000
    rng = np.random.default_rng(4)
    pts = np.stack([np.arange(n), np.zeros(n), rng.normal(size=n)], 1).astype(np.float32)
    idx = np.stack([np.arange(n), np.arange(n) + 1], 1).astype(np.int32)
    idx[-1, 1] = -1
    _, _, report = check_orient(gpu, pts, _unit(rng, n), idx, "chain")
    assert report["components"] == 1 and report["rounds"] >= 2


def test_orient_ring_of_64(gpu):
    n = 64
    rng = np.random.default_rng(5)
    a = 2 * np.pi * np.arange(n) / n
    pts = np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1).astype(np.float32)
    idx = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1).astype(np.int32)
    _, _, report = check_orient(gpu, pts, _unit(rng, n), idx, "ring")
    assert report["components"] == 1


def test_orient_lattice_plane_equal_weights(gpu):
    """all weights are equal (0): the slot numbers decide, and every normal ends as (0, 0, 1)"""
    pts = R.lattice_plane(20, 3.0, seed=6)
    idx, _ = R.knn_lists(pts, 9)
    sign = np.random.default_rng(7).choice(np.float32([-1, 1]), size=len(pts))
    nrm = np.stack([np.zeros_like(sign), np.zeros_like(sign), sign], 1).astype(np.float32)
    out, flips, report = check_orient(gpu, pts, nrm, idx, "lattice plane")
    assert report["components"] == 1 and (out[:, 2] == 1).all() and np.array_equal(flips, sign < 0)


def test_orient_zero_normals_and_missing_entries(gpu, sphere):
    rng = np.random.default_rng(8)
    nrm, idx = sphere.nrm.copy(), sphere.idx.copy()
    nrm[rng.choice(len(nrm), 100, replace=False)] = 0
    idx[rng.random(idx.shape) < 0.3] = -1
    out, flips, report = check_orient(gpu, sphere.pts, nrm, idx, "zero normals, -1 entries")
    assert report["skipped"] == 100 and not flips[(nrm == 0).all(1)].any()


@pytest.fixture(scope="module")
def scan():
    p, _ = synth.scan_cloud(6000, seed=31, device="cpu")
    pts = np.ascontiguousarray(p.numpy())
    idx, _ = R.knn_lists(pts, 12)
    return pts, idx, R.point_normals(pts, idx)[0]


def test_orient_scan_cloud(gpu, scan):
    pts, idx, nrm = scan
    check_orient(gpu, pts, nrm, idx, "scan cloud")


def test_orient_refuses_a_bad_index(gpu, sphere):
    idx = sphere.idx.copy()
    idx[5, 5] = len(idx)
    with pytest.raises(AsrHipError):
        ops.orient_normals(dev(sphere.pts, gpu), dev(sphere.nrm, gpu), dev(idx, gpu))
    check_orient(gpu, sphere.pts[:64], sphere.nrm[:64], np.minimum(sphere.idx[:64], 63), "after a refusal")


def test_orient_viewpoints(gpu, sphere):
    p, n = dev(sphere.pts, gpu), dev(sphere.nrm, gpu)
    out, flips, report = ops.orient_normals(p, n, viewpoints=torch.zeros(3, device=gpu), return_flips=True,
                                            return_report=True)
    ref_out, ref_flips, ref_report = R.orient_viewpoint(sphere.pts, sphere.nrm, np.zeros(3, np.float32))
    assert np.array_equal(flips.cpu().numpy(), ref_flips) and np.array_equal(bits(out.cpu().numpy()), bits(ref_out))
    assert report == dict(ref_report, rounds=0)
    assert ((out.cpu().numpy() * sphere.pts).sum(1) < 0).all()          # the centre sees the inside
    out = ops.orient_normals(p, n, viewpoints=2 * p)                     # a viewpoint above every point
    assert np.array_equal(bits(out.cpu().numpy()), bits(R.orient_viewpoint(sphere.pts, sphere.nrm, 2 * sphere.pts)[0]))
    assert ((out.cpu().numpy() * sphere.pts).sum(1) > 0).all()
    # n . (v - p) == 0 leaves the normal alone, whatever its sign; a zero normal is skipped
    pts = np.zeros((3, 3), np.float32)
    nrm = np.float32([[1, 0, 0], [-1, 0, 0], [0, 0, 0]])
    out, flips, report = ops.orient_normals(dev(pts, gpu), dev(nrm, gpu), viewpoints=dev(np.float32([0, 1, 0]), gpu),
                                            return_flips=True, return_report=True)
    assert np.array_equal(out.cpu().numpy(), nrm) and not flips.any().item()
    assert report == {"components": 0, "flipped": 0, "skipped": 1, "rounds": 0}


def test_orient_in_place(gpu, sphere):
    p, idx = dev(sphere.pts, gpu), dev(sphere.idx, gpu)
    want, want_flips = ops.orient_normals(p, dev(sphere.nrm, gpu), idx, return_flips=True)
    for view in (None, torch.zeros((1, 3), device=gpu)):
        n = dev(sphere.nrm, gpu)
        report = (ctypes.c_int64 * 4)()
        ops.context(gpu).call("asr_hip_normals_orient", _lib.ptr(p), _lib.ptr(n), ctypes.c_int64(len(sphere.pts)),
                              _lib.ptr(idx), 12, _lib.ptr(view), ctypes.c_int64(0 if view is None else 1), _lib.ptr(n),
                              None, report)
        ref = want if view is None else ops.orient_normals(p, dev(sphere.nrm, gpu), viewpoints=view)
        assert np.array_equal(bits(n.cpu().numpy()), bits(ref.cpu().numpy()))


def test_orient_on_a_side_stream(gpu, sphere):
    args = (dev(sphere.pts, gpu), dev(sphere.nrm, gpu), dev(sphere.idx, gpu))
    want = ops.orient_normals(*args, return_flips=True, return_report=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    largs, _ = late(side, *args)
    with torch.cuda.stream(side):
        got = ops.orient_normals(*largs, return_flips=True, return_report=True)
    side.synchronize()
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(want[0].cpu().numpy()))
    assert torch.equal(got[1], want[1]) and got[2] == want[2]


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_estimate_normals_is_the_composition(gpu, scan):
    import adaptivesurfacereconstruction as asr
    pts = scan[0]
    est = asr.estimate_normals(pts, 12)
    frame = asr._margin_frame(pts)
    p = dev(pts, gpu)
    idx, sq = ops.knn_index(frame, p, 12)
    nrm, eig, ok = ops.point_normals(p, idx, return_eigenvalues=True, return_ok=True)
    out, report = ops.orient_normals(p, nrm, idx, return_report=True)
    assert np.array_equal(est["neighbors"], idx.cpu().numpy()) and np.array_equal(est["neighbors"], scan[1])
    assert np.array_equal(bits(est["normals"]), bits(out.cpu().numpy()))
    assert np.array_equal(est["ok"], ok.cpu().numpy()) and est["ok"].dtype == np.bool_
    assert np.array_equal(bits(est["eigenvalues"]), bits(eig.cpu().numpy())) and est["report"] == report
    e = est["eigenvalues"]
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(est["ok"], e[:, 0] / e.sum(1, dtype=np.float32), np.float32(0))
    assert est["variation"].dtype == np.float32 and np.array_equal(est["variation"], want)
    kidx, ksq = asr.KDTree(pts).knn(12)
    assert np.array_equal(kidx, est["neighbors"]) and np.array_equal(bits(ksq), bits(sq.cpu().numpy()))
    view = asr.estimate_normals(pts, 12, viewpoint=[0, 0, 10])
    ref = R.orient_viewpoint(pts, nrm.cpu().numpy(), np.float32([0, 0, 10]))[0]
    assert np.array_equal(bits(view["normals"]), bits(ref)) and view["report"]["components"] == 0


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(4, seed=31)


def same_mesh(a, b):
    return np.array_equal(bits(a["vertices"]), bits(b["vertices"])) and np.array_equal(a["triangles"], b["triangles"])


def write_raw(path, pts):
    """a PLY without nx ny nz; nine digits carry an f32 exactly"""
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
                % len(pts))
        np.savetxt(f, pts, fmt="%.9g")


def test_reconstruct_surface_without_normals(gpu, scan, weights, tmp_path, capsys):
    import adaptivesurfacereconstruction as asr
    pts = scan[0]
    est = asr.estimate_normals(pts, 12)
    ok = est["ok"]
    want = asr.reconstruct_surface(pts[ok], est["normals"][ok], weights=weights)
    got = asr.reconstruct_surface(pts, None, normal_k=12, weights=weights)
    assert sorted(got) == ["triangles", "vertices"] and len(got["triangles"]) > 100
    assert same_mesh(got, want)
    # the command line on a file without normals reproduces the call
    raw, out, w = str(tmp_path / "raw.ply"), str(tmp_path / "m.ply"), str(tmp_path / "w.npz")
    write_raw(raw, pts)
    np.savez(w, **weights)
    assert asrtool.main(["--in", raw, "--out", out, "--estimate-normals", "12", "--weights", w]) == 0
    capsys.readouterr()
    v, t = ply.read_mesh(out)
    assert same_mesh({"vertices": v, "triangles": t}, want)


def test_reconstruct_surface_without_normals_thinned(gpu, scan, weights):
    import adaptivesurfacereconstruction as asr
    pts = scan[0]
    merged = asr.merge_points(pts, cell_size=0.05)
    assert 100 < len(merged["points"]) < len(pts)
    est = asr.estimate_normals(merged["points"], 12)
    ok = est["ok"]
    want = asr.reconstruct_surface(merged["points"][ok], est["normals"][ok], weights=weights)
    got = asr.reconstruct_surface(pts, None, normal_k=12, weights=weights, thin=0.05)
    assert same_mesh(got, want)


def test_asrtool_orient_cloud(gpu, scan, tmp_path, capsys):
    import adaptivesurfacereconstruction as asr
    pts = scan[0]
    raw, out = str(tmp_path / "raw.ply"), str(tmp_path / "oriented.ply")
    write_raw(raw, pts)
    for extra, view in (([], None), (["--viewpoint", "0,0,10"], (0, 0, 10))):
        assert asrtool.main(["--orient-cloud", raw, out, "--k", "12"] + extra) == 0
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        est = asr.estimate_normals(pts, 12, view)
        ok = est["ok"]
        p, n, r = ply.read_points(out)
        assert np.array_equal(p, pts[ok]) and np.array_equal(bits(n), bits(est["normals"][ok])) and len(r) == 0
        assert line == dict(est["report"], points=int(ok.sum()), dropped=int((~ok).sum()))
