"""GPU tests of the implicit field at arbitrary points: leaf location (asr_hip_leaf_locate) against the numpy oracle
of tests/test_query.py, the decoder at shifts (asr_hip_decode_mlp_at) against the reference-recorded fixture and a
float64 autograd evaluation, the whole-path query (asr_hip_implicit_query) against the forward and against finite
differences of itself, and its users (reconstruct_surface(vertex_normals=True), asrtool --normals)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from asr_hip import _lib, ply, synth
from asr_hip._lib import AsrHipError
from asr_hip.pipeline import ImplicitPipeline
from test_query import locate_oracle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "adaptive-surface-reconstruction_amd", "asrtool.py")
DEC = ("dense_decoder1.weight", "dense_decoder1.bias", "dense_decoder2.weight", "dense_decoder2.bias",
       "dense_decoder3.weight")


def _cloud(kind, n, seed):
    if kind == "sphere":
        pts, _ = synth.sphere_cloud(n, seed)
    else:
        p, _ = synth.scan_cloud(n, seed=seed, device="cpu", density_variance=10.0 if kind == "mixed" else 1.0)
        pts = p.numpy()
    if kind == "far":
        pts = (pts + 100).astype(np.float32)
    return pts, synth.knn_radii(pts, min(24, len(pts))), synth.bounding_box(pts, 0.1)


# ---- location ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,seed", [("sphere", 50000, 0), ("scan", 20000, 1), ("mixed", 30000, 2), ("scan", 300, 3),
                                         ("far", 20000, 4)])
def test_leaf_locate_equals_the_oracle(gpu, kind, n, seed):
    from asr_hip import ops
    pts, rad, bb = _cloud(kind, n, seed)
    frame = _lib.frame_init(*bb)
    tp, tr = torch.from_numpy(pts).to(gpu), torch.from_numpy(rad).to(gpu)
    _, leaves = ops.octree_build(frame, tp, tr)
    centers, sizes = ops.voxel_info(frame, leaves)
    keys = leaves.cpu().numpy().view(np.uint64)
    c, s = centers.cpu().numpy(), sizes.cpu().numpy()
    rng = np.random.default_rng(seed)
    # the root cube in positions, a little enlarged; leaf faces and corners; the cube's own faces
    lo = (-np.array(frame.offset[:], np.float64)) * frame.voxel_size[21]
    hi = lo + 2 ** 21 * float(frame.voxel_size[21])
    q = rng.uniform(lo - 0.01 * (hi - lo), hi + 0.01 * (hi - lo), size=(100000, 3)).astype(np.float32)
    pick = rng.integers(0, len(keys), 30000)
    sgn = rng.integers(-1, 2, size=(30000, 3)).astype(np.float32)
    q[:30000] = c[pick] + sgn * (0.5 * s[pick])[:, None]
    face = rng.integers(0, 3, 5000)
    q[30000:35000, :] = c[rng.integers(0, len(keys), 5000)]
    q[30000:35000][np.arange(5000), face] = np.where(rng.random(5000) < 0.5, lo[face], hi[face]).astype(np.float32)
    q[35000:35000 + len(pts[:5000])] = pts[:5000]
    rows = ops.leaf_locate(frame, leaves, torch.from_numpy(q).to(gpu)).cpu().numpy()
    want, hits = locate_oracle(frame, keys, q)
    assert np.array_equal(rows, want)
    assert np.all(hits[want >= 0] == 1)  # the leaves tile the cube: one level holds each inside point
    assert (rows >= 0).mean() > 0.9
    # input points: the located leaf is the point's own octree node or one of its descendants
    pk = ops.point_keys(frame, tp, tr).cpu().numpy().view(np.uint64)
    prow = ops.leaf_locate(frame, leaves, tp).cpu().numpy()
    ok = pk != 0
    assert np.all(prow[ok] >= 0)
    lk = keys[prow[ok]]
    first = np.array([1 << (3 * lev) for lev in range(22)], np.uint64)  # the first key of every level
    d = np.searchsorted(first, lk, "right") - np.searchsorted(first, pk[ok], "right")
    assert np.all(d >= 0) and np.array_equal(lk >> (3 * d).astype(np.uint64), pk[ok])
    if kind != "far":  # centres near the origin round back into their own voxel
        assert np.array_equal(ops.leaf_locate(frame, leaves, centers).cpu().numpy(), np.arange(len(keys)))
    bad = np.array([[np.inf, 0, 0], [-np.inf, 0, 0], [0, np.nan, 0], [0, 0, 1e30], [-1e30, 0, 0],
                    [lo[0] - 1e-3 * (hi[0] - lo[0]), c[0, 1], c[0, 2]], [c[0, 0], hi[1] + 1e-3 * (hi[1] - lo[1]), c[0, 2]]],
                   np.float32)
    assert np.all(ops.leaf_locate(frame, leaves, torch.from_numpy(bad).to(gpu)).cpu().numpy() == -1)
    # memory safety on an unsorted key list: rows stay in [-1, n)
    shuffled = leaves[torch.randperm(len(keys), device=gpu)].contiguous()
    r2 = ops.leaf_locate(frame, shuffled, torch.from_numpy(q).to(gpu)).cpu().numpy()
    assert r2.min() >= -1 and r2.max() < len(keys)


# ---- decoder at shifts ---------------------------------------------------------------------------------------------
def test_decode_mlp_at_matches_the_reference_fixture(gpu, golden_dir):
    from asr_hip import ops
    f = np.load(os.path.join(golden_dir, "decode_shifts_d1.npz"))
    w = [torch.from_numpy(f[k]).to(gpu) for k in DEC]
    vals, grad = ops.decode_mlp_at(torch.from_numpy(f["code"]).to(gpu), torch.from_numpy(f["shifts"]).to(gpu), *w,
                                   rows=torch.from_numpy(f["rows"]).to(gpu), gradient=True)
    vals, grad = vals.cpu().numpy(), grad.cpu().numpy()
    assert np.abs(vals - f["values"]).max() <= 1e-5 * np.abs(f["values"]).max()
    assert np.abs(grad - f["grad"]).max() <= 1e-5 * np.abs(f["grad"]).max()
    # rows < 0 give NaN; voxel sizes scale values[:, 0] only; the gradient is not computed when not asked for
    rows = torch.from_numpy(f["rows"]).to(gpu).clone()
    rows[::7] = -1
    sizes = torch.rand(f["code"].shape[0], device=gpu) + 0.5
    v2 = ops.decode_mlp_at(torch.from_numpy(f["code"]).to(gpu), torch.from_numpy(f["shifts"]).to(gpu), *w, rows=rows,
                           voxel_sizes=sizes).cpu().numpy()
    bad = np.zeros(len(v2), bool)
    bad[::7] = True
    assert np.all(np.isnan(v2[bad]))
    r = f["rows"][~bad]
    assert np.array_equal(v2[~bad, 1], vals[~bad, 1])
    assert np.allclose(v2[~bad, 0], vals[~bad, 0] * sizes.cpu().numpy()[r], rtol=1e-6, atol=0)


def _decode64(weights, code, shifts):
    """float64 torch autograd: values [M,2] and d values[:,0] / d shift"""
    w = {k: torch.as_tensor(np.asarray(weights[k]), dtype=torch.float64) for k in DEC}
    s = torch.as_tensor(np.asarray(shifts), dtype=torch.float64).requires_grad_(True)
    x = torch.cat([s, torch.as_tensor(np.asarray(code), dtype=torch.float64)], 1)
    f1 = torch.relu(x @ w[DEC[0]].T + w[DEC[1]])
    f2 = torch.relu(f1 @ w[DEC[2]].T + w[DEC[3]])
    v = f2 @ w[DEC[4]].T
    (g,) = torch.autograd.grad(v[:, 0].sum(), s)
    return v.detach().numpy(), g.numpy()


@pytest.mark.parametrize("channel_div", [4, 1])
def test_decode_mlp_at_matches_float64_autograd(gpu, channel_div):
    from asr_hip import ops
    weights = synth.make_weights(channel_div, seed=9)
    c = weights[DEC[0]].shape[1] - 3
    rng = np.random.default_rng(channel_div)
    code = rng.standard_normal((3000, c)).astype(np.float32)
    shifts = rng.uniform(-1.5, 1.5, size=(3000, 3)).astype(np.float32)
    vals, grad = ops.decode_mlp_at(torch.from_numpy(code).to(gpu), torch.from_numpy(shifts).to(gpu),
                                   *[torch.from_numpy(weights[k]).to(gpu) for k in DEC], gradient=True)
    v64, g64 = _decode64(weights, code, shifts)
    assert np.abs(vals.cpu().numpy() - v64).max() <= 1e-5 * np.abs(v64).max()
    assert np.abs(grad.cpu().numpy() - g64).max() <= 1e-5 * np.abs(g64).max()
    # no gradient buffer: the same values
    v_only = ops.decode_mlp_at(torch.from_numpy(code).to(gpu), torch.from_numpy(shifts).to(gpu),
                               *[torch.from_numpy(weights[k]).to(gpu) for k in DEC])
    assert torch.equal(v_only, vals)


# ---- whole path ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(gpu):
    p, q = synth.scan_cloud(4000, seed=5, device="cpu")
    pts, nrm = p.numpy(), q.numpy()
    rad = synth.knn_radii(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    return dict(pts=pts, bb=bb, args=(t(pts), t(nrm), t(rad), bb[0], bb[1]), weights=synth.make_weights(1, seed=5))


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_query_at_the_centres_is_the_forward_bit_for_bit(gpu, scene, precision):
    pipe = ImplicitPipeline(scene["weights"], device=gpu, precision=precision)
    values = pipe.forward(*scene["args"]).clone()
    centres = pipe.get("voxel_centers0")
    got, rows = pipe.query(centres, return_rows=True)
    assert np.array_equal(rows.cpu().numpy(), np.arange(len(values)))
    assert np.array_equal(got.cpu().numpy(), values.cpu().numpy())
    v2, g2 = pipe.query(centres, gradient=True)
    assert np.array_equal(v2.cpu().numpy(), values.cpu().numpy())
    assert torch.isfinite(g2).all()


@pytest.mark.parametrize("scale_sdf", [True, False])
def test_query_matches_float64_on_the_code(gpu, scene, scale_sdf):
    pipe = ImplicitPipeline(scene["weights"], device=gpu, scale_sdf=scale_sdf)
    pipe.forward(*scene["args"])
    code = pipe.get("code").cpu().numpy()
    keys = pipe.get("voxel_keys0").cpu().numpy().view(np.uint64)
    c, s = pipe.get("voxel_centers0").cpu().numpy(), pipe.get("voxel_sizes0").cpu().numpy()
    frame = _lib.frame_init(*scene["bb"])
    rng = np.random.default_rng(2)
    q = np.concatenate([rng.uniform(scene["bb"][0], scene["bb"][1], size=(20000, 3)),
                        scene["pts"][:3000] + rng.normal(0, 0.01, size=(3000, 3))]).astype(np.float32)
    vals, grad, rows = pipe.query(torch.from_numpy(q).to(gpu), gradient=True, return_rows=True)
    vals, grad, rows = vals.cpu().numpy(), grad.cpu().numpy(), rows.cpu().numpy()
    want_rows, _ = locate_oracle(frame, keys, q)
    assert np.array_equal(rows, want_rows)
    inside = rows >= 0
    r = rows[inside]
    shifts = (q[inside] - c[r]) / s[r][:, None]  # float32, as the contract
    v64, g64 = _decode64(scene["weights"], code[r], shifts)
    if scale_sdf:
        v64[:, 0] *= s[r]
    else:
        g64 /= s[r][:, None]
    assert np.abs(vals[inside] - v64).max() <= 1e-5 * np.abs(v64).max()
    assert np.abs(grad[inside] - g64).max() <= 1e-5 * np.abs(g64).max()
    assert np.all(np.isnan(vals[~inside])) and np.all(np.isnan(grad[~inside]))


def test_query_gradient_agrees_with_finite_differences(gpu, scene):
    """Central differences of the query's own values (h = 1e-3 size) against its gradient.  The field is piecewise
    linear in the position (ReLU network) and the gradient depends on the ReLU pattern only, so the comparison takes
    the samples whose +-h points lie in the same leaf and the same linear piece (bit-equal gradients at p - h, p, p + h);
    what remains is f32 rounding of the values."""
    pipe = ImplicitPipeline(scene["weights"], device=gpu)
    pipe.forward(*scene["args"])
    s = pipe.get("voxel_sizes0").cpu().numpy()
    rng = np.random.default_rng(4)
    p = (scene["pts"][:4000] + rng.normal(0, 0.005, size=(4000, 3))).astype(np.float32)
    _, g, rows = pipe.query(torch.from_numpy(p).to(gpu), gradient=True, return_rows=True)
    g, rows = g.cpu().numpy(), rows.cpu().numpy()
    keep = rows >= 0
    p, g, rows = p[keep], g[keep], rows[keep]
    h = (1e-3 * s[rows]).astype(np.float32)
    fd = np.zeros(g.shape, np.float64)
    same_leaf = np.ones(len(p), bool)
    same_piece = np.ones(len(p), bool)
    for d in range(3):
        pp, pm = p.copy(), p.copy()
        pp[:, d] += h
        pm[:, d] -= h
        vp, gp, rp = (t.cpu().numpy() for t in pipe.query(torch.from_numpy(pp).to(gpu), gradient=True, return_rows=True))
        vm, gm, rm = (t.cpu().numpy() for t in pipe.query(torch.from_numpy(pm).to(gpu), gradient=True, return_rows=True))
        same_leaf &= (rp == rows) & (rm == rows)
        same_piece &= np.all(gp == g, 1) & np.all(gm == g, 1)
        step = pp[:, d].astype(np.float64) - pm[:, d].astype(np.float64)  # the step the queries really took
        fd[:, d] = (vp[:, 0].astype(np.float64) - vm[:, 0].astype(np.float64)) / step
    sel = same_leaf & same_piece
    assert same_leaf.mean() > 0.8 and sel.sum() > 0.5 * same_leaf.sum()
    err = np.linalg.norm(fd - g, axis=1) / np.maximum(np.linalg.norm(g, axis=1), 1e-30)
    assert (err[sel] <= 1e-3).mean() >= 0.99, (sel.sum(), same_leaf.sum(), np.sort(err[sel])[-20:])
    # a wrong convention (a missing 1 / size, a sign, swapped axes) would fail on most samples of every leaf
    assert np.median(err[same_leaf]) <= 1e-3


def _free_port():
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def _sharded_worker(rank, world, port, out):
    sys.path[:0] = [REPO, os.path.join(REPO, "adaptive-surface-reconstruction_amd"), os.path.join(REPO, "tests")]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from asr_hip import shardcomm
    pts, nrm = synth.scan_cloud(6000, seed=55, device=dev)
    rad = synth.knn_radii_gpu(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    pipe = ImplicitPipeline(synth.make_weights(2, seed=6), device=dev)
    pipe.forward_sharded(shardcomm.HostStagedComm(), pts, nrm, rad, bb[0], bb[1])
    try:
        pipe.query(pts[:10])
        msg = None
    except AsrHipError as e:
        msg = str(e)
    out.put({"rank": rank, "msg": msg})
    dist.barrier()
    dist.destroy_process_group()


def test_query_refuses_a_context_without_a_complete_code(gpu, scene):
    pipe = ImplicitPipeline(scene["weights"], device=gpu)
    q = torch.zeros((4, 3), device=gpu)
    with pytest.raises(AsrHipError, match="implicit_query"):
        pipe.query(q)  # before any forward
    pts, nrm, rad, bmin, bmax = scene["args"]
    pipe.build(pts, rad, bmin, bmax)
    with pytest.raises(AsrHipError, match="implicit_query"):
        pipe.query(q)  # a build alone
    pipe.forward(*scene["args"])
    assert pipe.query(torch.zeros((0, 3), device=gpu)).shape == (0, 2)  # m = 0: nothing to do
    assert torch.isfinite(pipe.query(pipe.get("voxel_centers0")[:5])).all()
    pipe.build(pts, rad, bmin, bmax)
    with pytest.raises(AsrHipError, match="implicit_query"):
        pipe.query(q)  # the next build invalidates the code
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    infos = [out.get(timeout=600) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(i["msg"] is not None and "implicit_query" in i["msg"] for i in infos), infos


# ---- users ---------------------------------------------------------------------------------------------------------
def test_reconstruct_surface_vertex_normals(gpu, tmp_path, monkeypatch):
    import adaptivesurfacereconstruction as asr
    p, q = synth.scan_cloud(6000, seed=31, device="cpu")
    pts, nrm = p.numpy(), q.numpy()
    weights = synth.make_weights(4, seed=31)
    plain = asr.reconstruct_surface(pts, nrm, weights=weights)
    seen = {}
    query = ImplicitPipeline.query

    def spy(self, positions, gradient=False, return_rows=False):
        seen["pipe"], seen["positions"] = self, positions.clone()
        return query(self, positions, gradient, return_rows)

    monkeypatch.setattr(ImplicitPipeline, "query", spy)
    res = asr.reconstruct_surface(pts, nrm, weights=weights, vertex_normals=True)
    monkeypatch.undo()
    assert sorted(plain) == ["triangles", "vertices"]
    assert sorted(res) == ["triangles", "vertex_normals", "vertices"]
    assert np.array_equal(res["vertices"], plain["vertices"]) and np.array_equal(res["triangles"], plain["triangles"])
    assert len(res["triangles"]) > 100
    nv = res["vertex_normals"]
    assert nv.dtype == np.float32 and nv.shape == res["vertices"].shape
    assert np.array_equal(seen["positions"].cpu().numpy(), res["vertices"])
    _, g = seen["pipe"].query(torch.from_numpy(res["vertices"]).to(gpu), gradient=True)
    g = g.cpu().numpy()
    norm = np.linalg.norm(g, axis=1)
    live = norm > 0  # where every ReLU path of the narrow net is off the gradient vanishes: the normal is zero there
    assert live.mean() > 0.9
    assert np.allclose(nv[live], g[live] / norm[live][:, None], rtol=0, atol=1e-6)
    assert np.allclose(np.linalg.norm(nv[live], axis=1), 1, atol=1e-5) and np.all(nv[~live] == 0)
    # asrtool --normals writes the same normals; without the flag the file has none
    np.savez(str(tmp_path / "w.npz"), **weights)
    ply.write_points(str(tmp_path / "in.ply"), pts, nrm)
    base = [sys.executable, TOOL, "--in", str(tmp_path / "in.ply"), "--weights", str(tmp_path / "w.npz")]
    r = subprocess.run(base + ["--out", str(tmp_path / "n.ply"), "--normals"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    v, t, n = ply.read_mesh(str(tmp_path / "n.ply"), with_normals=True)
    assert np.array_equal(v, res["vertices"]) and np.array_equal(t, res["triangles"]) and np.array_equal(n, nv)
