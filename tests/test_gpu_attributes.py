"""GPU tests of per-point attributes carried onto positions (asr_hip_point_attributes_at): the fused
search-and-blend kernel against the float64 reference of tests/test_attributes.py, against the composition of the
project's own search / importance / reduction ops at a million points, and its users (ImplicitPipeline.transfer,
reconstruct_surface(point_attributes=...), asrtool --colors).

Tolerance (derived, not measured; eps = 2^-24): a weight carries an absolute error of at most about 32 eps (distance,
division, cube, compatibility, all quantities <= 1), a sum of n terms in any order n eps relative, so per row
    |A - A_ref| <= amax * eps * n * (64 / W + 4)            (test_attributes.row_bound)
with n and W the reference's at the chosen k and amax = max |a|.  The choice of k is a threshold: rows where some W_k
of the reference (k up to the chosen one) lies within a relative 1e-4 of min_weight may differ in k and are left out of
the value comparison -- at most 0.1 % of the rows, asserted; every other row must have the reference's k exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from asr_hip import _lib, ops, ply, synth
from asr_hip._lib import AsrHipError
from asr_hip.pipeline import ImplicitPipeline
from test_attributes import row_bound, transfer_reference

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "adaptive-surface-reconstruction_amd", "asrtool.py")
EPS = 2.0 ** -24
MIN_WEIGHT = 1e-2


def _cloud(kind, n, seed):
    if kind == "sphere":
        pts, _ = synth.sphere_cloud(n, seed)
    else:
        p, _ = synth.scan_cloud(n, seed=seed, device="cpu", density_variance=10.0 if kind == "mixed" else 1.0)
        pts = p.numpy()
    if kind == "far":
        pts = (pts + 100).astype(np.float32)
    return pts, synth.knn_radii(pts, min(24, len(pts))), synth.bounding_box(pts, 0.1)


def _near_threshold(W, k, min_weight):
    """rows whose choice of k is not decided by the reference: some W_k (k up to the chosen one; all of them when
    none was chosen) within a relative 1e-4 of min_weight"""
    kk = np.arange(W.shape[1])[None, :]
    seen = np.isfinite(W) & ((kk <= k[:, None]) | (k[:, None] < 0))
    return (seen & (np.abs(W - min_weight) <= 1e-4 * min_weight)).any(1)


def _check_against_reference(out, weight, widen, ref, amax, min_weight, fill, what):
    A, W, cnt, k = ref
    c = out.shape[1]
    unsure = _near_threshold(W, k, min_weight)
    print("%s: %d rows, %d near the threshold, k histogram %s" % (what, len(k), unsure.sum(),
                                                                  np.bincount(k + 1, minlength=5).tolist()))
    assert unsure.mean() <= 1e-3
    sure = ~unsure
    assert np.array_equal(widen[sure].astype(np.int64), k[sure]), what
    hit = sure & (k >= 0)
    miss = sure & (k < 0)
    assert np.all(out[miss] == np.float32(fill)) and np.all(weight[miss] == 0)
    rows = np.flatnonzero(hit)
    n, w = cnt[rows, k[rows]].astype(np.float64), W[rows, k[rows]]
    err = np.abs(out[rows].astype(np.float64) - A[rows, :c]).max(1)
    bound = row_bound(amax, n, w)
    print("%s: max |A - A_ref| / bound = %.3g (max err %.3g)" % (what, (err / bound).max() if len(rows) else 0,
                                                                  err.max() if len(rows) else 0))
    assert np.all(err <= bound), what
    werr = np.abs(weight[rows].astype(np.float64) - w)
    print("%s: max |W - W_ref| / (W n eps 40) = %.3g" % (what, (werr / (w * n * EPS * 40)).max() if len(rows) else 0))
    assert np.all(werr <= w * n * EPS * 40), what


# ---- 1. the kernel against the reference ------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,seed", [("sphere", 50000, 0), ("scan", 20000, 1), ("mixed", 30000, 2), ("scan", 300, 3),
                                         ("far", 20000, 4)])
def test_kernel_equals_the_reference(gpu, kind, n, seed):
    pts, rad, bb = _cloud(kind, n, seed)
    frame = _lib.frame_init(*bb)
    tp, tr = torch.from_numpy(pts).to(gpu), torch.from_numpy(rad).to(gpu)
    _, leaves = ops.octree_build(frame, tp, tr)
    centers, vsizes = ops.voxel_info(frame, leaves)
    rng = np.random.default_rng(seed)
    lo = (-np.array(frame.offset[:], np.float64)) * frame.voxel_size[21]
    hi = lo + 2 ** 21 * float(frame.voxel_size[21])
    nq = min(8000, 4 * len(pts))
    pick = rng.integers(0, len(pts), nq)
    mesh_like = pts[pick] + (rng.normal(size=(nq, 3)) * 0.5 * rad[pick, None]).astype(np.float32)
    cen = centers.cpu().numpy()[rng.integers(0, len(leaves), min(4000, len(leaves)))]
    uniform = rng.uniform(lo, hi, size=(600, 3)).astype(np.float32)
    outside = rng.uniform(lo - 0.2 * (hi - lo), lo - 0.01 * (hi - lo), size=(20, 3)).astype(np.float32)
    bad = np.array([[np.inf, 0, 0], [-np.inf, 0, 0], [0, np.nan, 0], [0, 0, 1e30], [-1e30, 0, 0]], np.float32)
    q = np.concatenate([mesh_like, cen, uniform, outside, bad]).astype(np.float32)
    tq = torch.from_numpy(q).to(gpu)
    rows = ops.leaf_locate(frame, leaves, tq).long()
    # the located leaf's size from the device, given to the reference as it is; rows outside the cube get a usable size
    # (the kernel has to refuse them by itself) and a few inside rows an unusable one
    sizes = torch.where(rows >= 0, vsizes[rows.clamp(min=0)], torch.full((), 0.05, device=gpu)).contiguous()
    sizes[:4] = torch.tensor([0.0, -1.0, float("nan"), float("inf")], device=gpu)
    s = sizes.cpu().numpy()
    assert (rows[:nq] >= 0).float().mean() > 0.8 and (rows[-25:] < 0).all()  # (the inputs are what they are meant to be)
    attr = rng.uniform(0, 255, size=(len(pts), 16)).astype(np.float32)
    amax = float(np.abs(attr).max())
    for max_widen in (0, 3):
        fill = -7.0 if max_widen else 0.0
        ref = transfer_reference(pts, rad, attr, q, s, max_widen, MIN_WEIGHT, fill, frame=frame)
        assert (ref[3][-25:] == -1).all() and (ref[3][:4] == -1).all()
        for c in (1, 3, 4, 16):
            ta = torch.from_numpy(np.ascontiguousarray(attr[:, :c])).to(gpu)
            out, weight, widen = ops.point_attributes_at(frame, tp, tr, ta, tq, sizes, max_widen, MIN_WEIGHT, fill,
                                                         return_info=True)
            again = ops.point_attributes_at(frame, tp, tr, ta, tq, sizes, max_widen, MIN_WEIGHT, fill, return_info=True)
            for a, b in zip((out, weight, widen), again):  # the same bits, run to run
                assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                   b.view(torch.int32) if b.dtype == torch.float32 else b)
            assert out.shape == (len(q), c) and widen.dtype == torch.int8
            _check_against_reference(out.cpu().numpy(), weight.cpu().numpy(), widen.cpu().numpy(), ref, amax, MIN_WEIGHT,
                                     fill, "%s %d C=%d widen<=%d" % (kind, n, c, max_widen))
            plain = ops.point_attributes_at(frame, tp, tr, ta if c > 1 else ta[:, 0], tq, sizes, max_widen, MIN_WEIGHT, fill)
            assert torch.equal(plain.view(torch.int32), out.view(torch.int32))
    # convexity: a blend never leaves the range of the input
    got = out.cpu().numpy()[widen.cpu().numpy() >= 0]
    assert got.min() >= attr.min() and got.max() <= attr.max()


def test_empty_inputs_and_argument_errors(gpu):
    pts, rad, bb = _cloud("scan", 300, 3)
    frame = _lib.frame_init(*bb)
    tp, tr = torch.from_numpy(pts).to(gpu), torch.from_numpy(rad).to(gpu)
    q = tp[:50].contiguous()
    s = torch.full((50,), 0.1, device=gpu)
    none3 = torch.zeros((0, 3), device=gpu)
    out, w, k = ops.point_attributes_at(frame, none3, torch.zeros(0, device=gpu), torch.zeros((0, 2), device=gpu), q, s,
                                        fill=4.0, return_info=True)  # N = 0
    assert out.shape == (50, 2) and (out == 4.0).all() and (w == 0).all() and (k == -1).all()
    out = ops.point_attributes_at(frame, tp, tr, tp, none3, torch.zeros(0, device=gpu))  # M = 0
    assert out.shape == (0, 3)
    with pytest.raises(AsrHipError, match="attribute channels"):
        ops.point_attributes_at(frame, tp, tr, torch.zeros((300, 17), device=gpu), q, s)
    with pytest.raises(AsrHipError, match="attribute channels"):
        ops.point_attributes_at(frame, tp, tr, torch.zeros((300, 0), device=gpu), q, s)
    with pytest.raises(AsrHipError, match="min_weight"):
        ops.point_attributes_at(frame, tp, tr, tp, q, s, min_weight=0.0)
    with pytest.raises(AsrHipError, match="max_widen"):
        ops.point_attributes_at(frame, tp, tr, tp, q, s, max_widen=-1)
    with pytest.raises(ValueError):
        ops.point_attributes_at(frame, tp, tr, tp[:10], q, s)
    with pytest.raises(ValueError):
        ops.point_attributes_at(frame, tp, tr, tp, q, s[:10])
    # a radius as large as the root cube (and larger): every point is a member
    big = torch.full((50,), 4 * float(frame.voxel_size[0]), device=gpu)
    out, w, k = ops.point_attributes_at(frame, tp, tr, torch.ones(300, device=gpu), q, big, max_widen=0, min_weight=1e-30,
                                        return_info=True)
    ref = transfer_reference(pts, rad, np.ones(300), pts[:50], big.cpu().numpy(), 0, 1e-30, 0.0, frame=frame)
    assert (ref[2][:, 0] == 300).all() and (k == 0).all()
    assert np.allclose(w.cpu().numpy(), ref[1][:, 0], rtol=300 * EPS * 40, atol=0)


# ---- 2. against the project's own ops, at size -------------------------------------------------------------------
def test_fused_call_equals_the_composition_at_a_million_points(gpu):
    """max_widen = 0 against multi_radius_search -> squared distance / size^2 -> aggregation_importance -> gather,
    multiply, reduce_subarrays_sum -> divide: the search is checked bit for bit at 10 M points elsewhere, this pins the
    fused kernel to it where a brute-force reference cannot go"""
    n = 1_000_000
    pts, _ = synth.scan_cloud(n, seed=5, device=gpu)
    rad = synth.knn_radii_gpu(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    frame = _lib.frame_init(*bb)
    _, leaves = ops.octree_build(frame, pts, rad)
    _, vsizes = ops.voxel_info(frame, leaves)
    g = torch.Generator(device=gpu)
    g.manual_seed(6)
    q = (pts + 0.5 * rad[:, None] * torch.randn((n, 3), device=gpu, generator=g)).contiguous()
    rows = ops.leaf_locate(frame, leaves, q).long()
    sizes = torch.where(rows >= 0, vsizes[rows.clamp(min=0)], torch.zeros((), device=gpu)).contiguous()
    c = 3
    attr = (255 * torch.rand((n, c), device=gpu, generator=g)).contiguous()
    out, weight, widen = ops.point_attributes_at(frame, pts, rad, attr, q, sizes, 0, MIN_WEIGHT, 0.0, return_info=True)
    # the composition, from ops that exist without this feature
    idx, dist, rs, compat = ops.multi_radius_search(frame, pts, rad, q, sizes)
    cnt = rs[1:] - rs[:-1]
    row = torch.repeat_interleave(torch.arange(n, device=gpu), cnt)
    dn = dist / (sizes * sizes)[row]  # the search returns the raw squared distance
    imp = ops.aggregation_importance(compat, dn)
    den = ops.reduce_subarrays_sum(imp, rs)
    num = torch.stack([ops.reduce_subarrays_sum(imp * attr[idx.long(), ch], rs) for ch in range(c)], 1)
    comp = num / den[:, None]
    w64 = torch.zeros(n, dtype=torch.float64, device=gpu).index_add_(0, row, imp.double())
    unsure = (w64 - MIN_WEIGHT).abs() <= 1e-4 * MIN_WEIGHT
    valid = sizes > 0
    hit = valid & ~unsure & (w64 >= MIN_WEIGHT)
    miss = ~unsure & ~(valid & (w64 >= MIN_WEIGHT))
    print("composition: %d pairs, %.1f members per row (max %d), hit %.4f, near the threshold %d"
          % (idx.numel(), cnt.float().mean().item(), cnt.max().item(), hit.float().mean().item(), int(unsure.sum())))
    assert unsure.float().mean().item() <= 1e-3 and hit.float().mean().item() > 0.95
    assert (widen[hit] == 0).all() and (widen[miss] == -1).all() and (out[miss] == 0).all() and (weight[miss] == 0).all()
    amax = float(attr.abs().max())
    bound = amax * EPS * cnt.double() * (64.0 / w64 + 4.0)
    err = (out.double() - comp.double()).abs().max(1).values
    print("composition: max |fused - composition| / bound = %.3g (max err %.3g)"
          % ((err[hit] / bound[hit]).max().item(), err[hit].max().item()))
    assert (err[hit] <= bound[hit]).all()
    assert ((weight.double() - w64).abs()[hit] <= (w64 * cnt.double() * EPS * 40)[hit]).all()


# ---- 3. pipeline and user surface ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(gpu):
    p, q = synth.scan_cloud(6000, seed=31, device="cpu")
    pts, nrm = p.numpy(), q.numpy()
    rad = synth.knn_radii(pts, 24)
    return pts, nrm, rad, synth.bounding_box(pts, 0.1), synth.make_weights(4, seed=31)


def test_pipeline_transfer_equals_the_op_called_by_hand(gpu, scene):
    pts, nrm, rad, bb, weights = scene
    pipe = ImplicitPipeline(weights, device=gpu)
    tp, tn, tr = (torch.from_numpy(a).to(gpu) for a in (pts, nrm, rad))
    attr = torch.from_numpy(np.random.default_rng(0).uniform(0, 255, (len(pts), 3)).astype(np.float32)).to(gpu)
    with pytest.raises(AsrHipError) as before:  # no forward yet: the query's own error
        pipe.transfer(tp, tr, attr, tp)
    with pytest.raises(AsrHipError) as query_error:
        pipe.query(tp)
    assert str(before.value) == str(query_error.value) and "no complete network output" in str(before.value)
    pipe.forward(tp, tn, tr, *bb)
    v, t = pipe.mesh()
    assert len(v) > 500
    got = pipe.transfer(tp, tr, attr, v, return_info=True)
    frame = _lib.frame_init(*bb)
    rows = ops.leaf_locate(frame, pipe.get("voxel_keys0"), v).long()
    assert (rows >= 0).all()
    want = ops.point_attributes_at(frame, tp, tr, attr, v, pipe.get("voxel_sizes0")[rows], return_info=True)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert (got[2] >= 0).float().mean() > 0.9  # (a seeded net's surface lies anywhere: no coverage claim here)
    # numpy positions, keywords, a position outside the octree
    out = pipe.transfer(tp, tr, attr[:, 0].contiguous(), np.array([[1e3, 0, 0]], np.float32), fill=-1.0)
    assert out.shape == (1, 1) and out.item() == -1.0
    # the forward's own results are untouched by a transfer
    assert torch.equal(pipe.query(v), pipe.query(v))
    pipe.build(tp, tr, *bb)  # a build alone leaves no usable forward
    with pytest.raises(AsrHipError, match="no complete network output"):
        pipe.transfer(tp, tr, attr, v)


def test_reconstruct_surface_point_attributes(gpu, scene, monkeypatch):
    import adaptivesurfacereconstruction as asr
    pts, nrm, _, _, weights = scene
    rng = np.random.default_rng(1)
    # a few far outliers, so that the pre-filter really drops points
    extra = rng.uniform(5, 6, (40, 3)).astype(np.float32)
    pts = np.concatenate([pts[:3000], extra, pts[3000:]])
    nrm = np.concatenate([nrm[:3000], np.tile(np.float32([0, 0, 1]), (40, 1)), nrm[3000:]])
    plain = asr.reconstruct_surface(pts, nrm, weights=weights)
    seen = {}
    transfer = ImplicitPipeline.transfer

    def spy(self, points, radii, attributes, positions, **kw):
        seen.update(pipe=self, points=points.clone(), radii=radii.clone(), attributes=attributes.clone())
        return transfer(self, points, radii, attributes, positions, **kw)

    monkeypatch.setattr(ImplicitPipeline, "transfer", spy)
    res = asr.reconstruct_surface(pts, nrm, weights=weights, point_attributes=pts)
    monkeypatch.undo()
    assert sorted(plain) == ["triangles", "vertices"]  # without the keyword: today's keys
    assert sorted(res) == ["triangles", "vertex_attributes", "vertices"]
    assert np.array_equal(res["vertices"], plain["vertices"]) and np.array_equal(res["triangles"], plain["triangles"])
    va, v = res["vertex_attributes"], res["vertices"]
    assert va.dtype == np.float32 and va.shape == v.shape and len(v) > 500
    fp, fr = seen["points"].cpu().numpy(), seen["radii"].cpu().numpy()
    assert len(fp) < len(pts)  # the pre-filter dropped something
    assert np.array_equal(seen["attributes"].cpu().numpy(), fp)  # ... and the attributes went through the same mask
    # attribute = position: the blend lies within the ball it was taken from
    pipe = seen["pipe"]
    tv = torch.from_numpy(v).to(gpu)
    _, weight, widen = pipe.transfer(seen["points"], seen["radii"], seen["attributes"], tv, return_info=True)
    frame = _lib.frame_init(fp.min(0), fp.max(0))
    rows = ops.leaf_locate(frame, pipe.get("voxel_keys0"), tv).long()
    s = pipe.get("voxel_sizes0")[rows].cpu().numpy()
    ref = transfer_reference(fp, fr, fp, v, s, frame=frame)
    k = widen.cpu().numpy().astype(np.int64)
    sure = ~_near_threshold(ref[1], ref[3], MIN_WEIGHT)
    assert np.array_equal(k[sure], ref[3][sure]) and (k >= 0).all()
    n, w = ref[2][np.arange(len(k)), ref[3]], ref[1][np.arange(len(k)), ref[3]]
    tol = row_bound(float(np.abs(fp).max()), n, w)
    assert np.all(np.linalg.norm(va.astype(np.float64) - v, axis=1)[sure] <= (s * 2.0 ** k + np.sqrt(3) * tol)[sure])
    assert np.all(np.abs(va - ref[0]).max(1)[sure] <= tol[sure])
    # a constant colour stays constant to amax n eps; 1-D attributes give [V,1]
    const = asr.reconstruct_surface(pts, nrm, weights=weights, point_attributes=np.full(len(pts), 255.0))
    assert const["vertex_attributes"].shape == (len(v), 1)
    cerr = np.abs(const["vertex_attributes"][:, 0].astype(np.float64) - 255.0)
    print("constant colour: max error / (amax n eps) = %.3g, fewest members %d" % ((cerr / (255.0 * n * EPS))[sure].max(), n[sure].min()))
    assert np.all(cerr[sure] <= (255.0 * n * EPS)[sure])
    for wrong in (pts[:-1], np.zeros((len(pts), 2, 2)), np.zeros((len(pts), 0)), ["a"] * len(pts)):
        with pytest.raises(ValueError):
            asr.reconstruct_surface(pts, nrm, weights=weights, point_attributes=wrong)


# ---- 4. command line -----------------------------------------------------------------------------------------------
def test_asrtool_colors_and_normals_end_to_end(gpu, scene, tmp_path):
    pts, nrm, _, _, weights = scene
    rng = np.random.default_rng(2)
    col = np.stack([rng.integers(40, 200, len(pts)), rng.integers(0, 256, len(pts)), np.full(len(pts), 90)], 1).astype(np.uint8)
    np.savez(str(tmp_path / "w.npz"), **weights)
    ply.write_points(str(tmp_path / "in.ply"), pts, nrm, colors=col)
    r = subprocess.run([sys.executable, TOOL, "--in", str(tmp_path / "in.ply"), "--out", str(tmp_path / "out.ply"),
                        "--weights", str(tmp_path / "w.npz"), "--colors", "--normals"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    v, t, n, c = ply.read_mesh(str(tmp_path / "out.ply"), with_normals=True, with_colors=True)
    assert len(t) > 100 and n is not None and n.shape == v.shape
    assert c is not None and c.dtype == np.uint8 and c.shape == v.shape
    for ch in range(3):  # convexity
        assert col[:, ch].min() <= c[:, ch].min() and c[:, ch].max() <= col[:, ch].max()
    assert np.all(c[:, 2] == 90) and c[:, 1].std() > 1
    # the same mesh as without the flags
    r = subprocess.run([sys.executable, TOOL, "--in", str(tmp_path / "in.ply"), "--out", str(tmp_path / "plain.ply"),
                        "--weights", str(tmp_path / "w.npz")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    v2, t2, c2 = ply.read_mesh(str(tmp_path / "plain.ply"), with_colors=True)
    assert np.array_equal(v2, v) and np.array_equal(t2, t) and c2 is None
