"""GPU checks of the bf16x3_2acc precision (ASR_CONV16_BF16X3_2ACC): bf16x3's operands and six products, the five small
products of every step in a second accumulator that is added once before the epilogue.  Single layers against the oracle
on every instance, bit-identity across instances / kernels / sharded runs, packing, the slot-range split, the error of the
whole network against the oracle's double-accumulating evaluation at 1 M and 10 M points, and the user surfaces."""
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity
from asr_hip import ply, synth
from oracle import oracle as O
from test_gpu_conv16 import SHAPES, _csr, _t, geo  # noqa: F401  (geo: module fixture)
from test_gpu_sharded import _free_port, _native_worker, _worker

pytestmark = pytest.mark.gpu

MODE = "bf16x3_2acc"
_close = parity.assert_close
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "adaptive-surface-reconstruction_amd", "asrtool.py")


def _layer(geo, shape, seed_extra=0):
    kind, level, K, cin, ca, cb, nt, waves = shape
    idx, kidx, rs, num_inp = _csr(geo, kind, level)
    rng = np.random.default_rng(cin * 31 + ca + level + seed_extra)
    occ = 8.0 if K == 55 else 1.0
    f = rng.standard_normal((num_inp, cin)).astype(np.float32)
    Wa = (rng.standard_normal((K, cin, ca)) * np.sqrt(2.0 / (occ * cin))).astype(np.float32)
    ba = (rng.standard_normal(ca) * 0.1).astype(np.float32)
    imp = rng.uniform(0.05, 1.0, size=num_inp).astype(np.float32)
    Wb = (rng.standard_normal((K, cin, cb)) * np.sqrt(2.0 / (occ * cin))).astype(np.float32) if cb else None
    bb = (rng.standard_normal(cb) * 0.1).astype(np.float32) if cb else None
    return idx, kidx, rs, f, Wa, ba, imp, Wb, bb


def _run(gpu, shape, data, packed, nt, waves, plan_on):
    """one convolution in the new mode (two-bank + importance + normalised where the shape has bank b); returns
    (output, launch key)"""
    from asr_hip import ops
    kind, level, K, cin, ca, cb, _, _ = shape
    idx, kidx, rs, f, Wa, ba, imp, Wb, bb = data
    ctx = ops.context(gpu)
    ctx.set_option("sconv_plan", int(plan_on))
    try:
        ctx.sconv_variant_counts(reset=True)
        kw = dict(bias=_t(ba, gpu), relu=True, force_nt=nt, force_waves=waves)
        if cb:
            out = ops.sparse_conv16(MODE, packed, K, cin, ca, _t(f, gpu), _t(idx, gpu), _t(kidx, gpu), _t(rs, gpu),
                                    inp_importance=_t(imp, gpu), normalize=True, cout_b=cb, bias_b=_t(bb, gpu), **kw)
        else:
            out = ops.sparse_conv16(MODE, packed, K, cin, ca, _t(f, gpu), _t(idx, gpu), _t(kidx, gpu), _t(rs, gpu), **kw)
        keys = list(ctx.sconv_variant_counts())
    finally:
        ctx.set_option("sconv_plan", 1)
    assert len(keys) == 1 and keys[0][5] == 4, keys
    return out.cpu().numpy(), keys[0]


@pytest.mark.parametrize("plan_on", [1, 0], ids=["plan", "table"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s%d-%dx%d+%d-nt%dw%d" % (s[0], s[1], s[3], s[4], s[5], s[6], s[7]))
def test_every_instance_vs_oracle(geo, gpu, shape, plan_on):
    """every shape of tests/test_gpu_conv16.py on both kernels: plain / two-bank, and the importance-weighted single bank"""
    from asr_hip import ops
    kind, level, K, cin, ca, cb, nt, waves = shape
    if cin % 4:
        pytest.skip("f32 rows need cin % 4 == 0")
    data = _layer(geo, shape)
    idx, kidx, rs, f, Wa, ba, imp, Wb, bb = data
    nimp = imp[idx.astype(np.int64)]
    packed = ops.pack_filters(_t(Wa, gpu), MODE, _t(Wb, gpu) if cb else None)
    with O.precise():
        ref = np.maximum(O.sparse_conv(Wa, f, idx, kidx, None, rs, False) + ba, 0)
        if cb:
            ref = np.concatenate([ref, np.maximum(O.sparse_conv(Wb, f, idx, kidx, nimp, rs, True) + bb, 0)], 1)
        ref_imp = np.maximum(O.sparse_conv(Wa, f, idx, kidx, nimp, rs, True) + ba, 0)
    out, key = _run(gpu, shape, data, packed, nt, waves, plan_on)
    _close(out, ref)
    assert key[6] == int(plan_on and cin % 32 == 0) and (nt == 0 or key[0] == nt), key
    if not cb:
        ctx = ops.context(gpu)
        ctx.set_option("sconv_plan", plan_on)
        try:
            out2 = ops.sparse_conv16(MODE, packed, K, cin, ca, _t(f, gpu), _t(idx, gpu), _t(kidx, gpu), _t(rs, gpu),
                                     inp_importance=_t(imp, gpu), normalize=True, bias=_t(ba, gpu), relu=True,
                                     force_nt=nt, force_waves=waves)
        finally:
            ctx.set_option("sconv_plan", 1)
        _close(out2.cpu().numpy(), ref_imp)


@pytest.mark.parametrize("shape", [("nb", 1, 55, 128, 128, 0, 0, 0), ("nb", 1, 55, 128, 120, 8, 0, 0),
                                   ("nb", 0, 55, 64, 64, 0, 0, 0), ("nb", 0, 55, 32, 56, 8, 0, 0)],
                         ids=["plain128", "dual128", "plain64", "dual64"])
def test_rounding_order_does_not_depend_on_the_instance(geo, gpu, shape):
    """every forced column tile (NT) and block shape (WAVES) of one layer, on the plan and the table kernel, returns the
    same bits (two-bank layers: bank b is normalised by an importance sum the two kernels form in different orders, so
    across kernels only bank a is compared bit for bit)"""
    from asr_hip import ops
    kind, level, K, cin, ca, cb, _, _ = shape
    data = _layer(geo, shape, 7)
    packed = ops.pack_filters(_t(data[4], gpu), MODE, _t(data[7], gpu) if cb else None)
    ctot = (ca + cb + 15) // 16 * 16
    outs = {}
    for plan_on in (1, 0):
        for nt in (1, 2, 4, 8):
            if ctot % (nt * 16):
                continue
            for waves in (4, 8):
                out, key = _run(gpu, shape, data, packed, nt, waves, plan_on)
                assert key[0] == nt and key[3] == waves and key[6] == plan_on, key
                outs[(plan_on, nt, waves)] = out
    assert len(outs) >= 12
    first = outs[(1, 8 if ctot % 128 == 0 else 4, 8)]
    for k, o in outs.items():
        if k[0] == 1 or not cb:
            assert np.array_equal(o.view(np.uint32), first.view(np.uint32)), k
        else:
            assert np.array_equal(o[:, :ca].view(np.uint32), first[:, :ca].view(np.uint32)), k
            assert np.abs(o - first).max() <= 1e-6 * max(1.0, float(np.abs(first).max())), k


def test_packing_is_bf16x3s(gpu):
    from asr_hip import ops
    rng = np.random.default_rng(3)
    for K, cin, ca, cb in ((55, 128, 120, 8), (55, 64, 64, 0), (9, 40, 24, 0), (55, 32, 56, 8)):
        Wa = _t(rng.standard_normal((K, cin, ca)).astype(np.float32), gpu)
        Wb = _t(rng.standard_normal((K, cin, cb)).astype(np.float32), gpu) if cb else None
        a = ops.pack_filters(Wa, MODE, Wb)
        b = ops.pack_filters(Wa, "bf16x3", Wb)
        assert a.dtype == b.dtype and torch.equal(a, b), (K, cin, ca, cb)


def test_slot_range_split(geo, gpu):
    """the split of the coarse grids' plain 55-slot layers runs in the new mode exactly when it runs in bf16x3, and stays
    within the oracle tolerance; whatever rows share a tile, the same bits"""
    from asr_hip import ops
    idx, kidx, rs, num_inp = _csr(geo, "nb", 0)
    v = len(rs) - 1
    ctx = ops.context(gpu)
    assert ctx.get_option("sconv_split_min_rows") <= v <= ctx.get_option("sconv_split_rows"), v
    rng = np.random.default_rng(78)
    K, cin, ca = 55, 64, 128
    f = rng.standard_normal((num_inp, cin)).astype(np.float32)
    W = (rng.standard_normal((K, cin, ca)) * np.sqrt(2.0 / (8 * cin))).astype(np.float32)
    b = (rng.standard_normal(ca) * 0.1).astype(np.float32)
    res = rng.standard_normal((v, ca)).astype(np.float32)
    d_idx, d_k, d_rs = _t(idx, gpu), _t(kidx, gpu), _t(rs, gpu)
    with O.precise():
        ref = np.maximum(O.sparse_conv(W, f, idx, kidx, None, rs, False) + b, 0) + res
    keys, outs = {}, {}
    for name, perm in (("regrouped", ops.row_groups(d_k, d_rs)),
                       ("shuffled", torch.from_numpy(rng.permutation(v).astype(np.int32)).to(gpu))):
        plan = ops.ConvPlan(K, d_idx, d_k, d_rs, row_perm=perm)
        for mode in ("bf16x3", MODE):
            ctx.sconv_variant_counts(reset=True)
            out = ops.sparse_conv16(mode, ops.pack_filters(_t(W, gpu), mode), K, cin, ca, _t(f, gpu), d_idx, d_k, d_rs,
                                    row_perm=perm, plan=plan, bias=_t(b, gpu), relu=True, residual=_t(res, gpu))
            k = list(ctx.sconv_variant_counts())
            assert len(k) == 1, k
            keys[(name, mode)] = k[0][:5] + k[0][6:]
            outs[(name, mode)] = out.cpu().numpy()
            _close(outs[(name, mode)], ref)
        del plan
    assert len(keys[("regrouped", MODE)]) == 7 and keys[("regrouped", MODE)][-1] == 1  # the split ran
    assert keys[("regrouped", MODE)] == keys[("regrouped", "bf16x3")]
    assert np.array_equal(outs[("regrouped", MODE)], outs[("shuffled", MODE)])


def _stats(got, exact):
    e = np.asarray(got, np.float64) - exact
    scale = max(1.0, float(np.abs(exact).max()))
    return {"max": float(np.abs(e).max()) / scale, "rms": float(np.sqrt(np.mean(e * e))) / scale,
            "mean": float(e.mean()) / scale, "share": parity.pass_fraction(got, exact)}


def test_one_million_points_error_below_the_fp32_oracle(gpu):
    """the cloud and weights of scripts/split_error_study.py (1 M points, full width): against the oracle's
    double-accumulating network, the new mode's rms error is at most 0.6 x that of the oracle's own fp32 evaluation and
    below bf16x3's, its max error no larger, its share within 1e-5 + 1e-5 |exact| no smaller, its mean error below 1e-8 of
    the range; two forwards return the same bits"""
    from asr_hip.pipeline import ImplicitPipeline
    pts, nrm = synth.scan_cloud(1_000_000, seed=1000, device=gpu)
    radii = torch.from_numpy(synth.knn_radii(pts.cpu().numpy(), 24)).to(gpu)
    bb = synth.bounding_box(pts, 0.1)
    weights = synth.make_weights(1, seed=2)
    hp, hn = pts.cpu().numpy(), nrm.cpu().numpy()
    item = parity.oracle_geometry(hp, radii.cpu().numpy(), bb[0], bb[1])
    with O.precise():
        exact = parity.oracle_network(item, hp, hn, weights)
    ref32 = parity.oracle_network(item, hp, hn, weights)
    got = {}
    for precision in (MODE, "bf16x3"):
        pipe = ImplicitPipeline(weights, device=gpu, precision=precision)
        values = pipe.forward(pts, nrm, radii, bb[0], bb[1]).clone()
        got[precision] = {"code": pipe.get("code").cpu().numpy(), "values": values.cpu().numpy()}
        if precision == MODE:
            again = pipe.forward(pts, nrm, radii, bb[0], bb[1])
            assert torch.equal(values, again)
        del pipe
    for k in ("code", "values"):
        cpu, new, old = _stats(ref32[k], exact[k]), _stats(got[MODE][k], exact[k]), _stats(got["bf16x3"][k], exact[k])
        print("1 M points, %s: fp32 oracle %s | bf16x3_2acc %s | bf16x3 %s" % (k, cpu, new, old))
        assert new["rms"] <= 0.6 * cpu["rms"], (k, new, cpu)
        assert new["max"] <= cpu["max"], (k, new, cpu)
        assert new["share"] >= cpu["share"], (k, new, cpu)
        assert abs(new["mean"]) <= 1e-8, (k, new)
        assert new["rms"] < old["rms"], (k, new, old)


def test_ten_million_points_full_width_vs_oracle(gpu):
    """C3 at the size, widths and weights of the bench (as test_ten_million_points_full_width_headline_arithmetic_vs_oracle):
    geometry equal to the oracle's; code and values no further from the exact result than the oracle's fp32 evaluation
    (max error) with no smaller share within 1e-5 + 1e-5 |exact|; the 44 launches are the bench's instances in mode 4"""
    from asr_hip.pipeline import ImplicitPipeline
    from sconv_instances import BENCH_SHAPES16, BENCH_SPLIT16
    pts, nrm = synth.scan_cloud(10_000_000, seed=1000, device=gpu)
    radii = torch.from_numpy(synth.knn_radii(pts.cpu().numpy(), 24)).to(gpu)
    bb = synth.bounding_box(pts, 0.1)
    weights = synth.make_weights(1, seed=2)
    hp, hn = pts.cpu().numpy(), nrm.cpu().numpy()
    item = parity.oracle_geometry(hp, radii.cpu().numpy(), bb[0], bb[1])
    with O.precise():
        exact = parity.oracle_network(item, hp, hn, weights)
    ref32 = parity.oracle_network(item, hp, hn, weights)
    pipe = ImplicitPipeline(weights, device=gpu, precision=MODE)
    pipe.ctx.sconv_variant_counts(reset=True)
    values = pipe.forward(pts, nrm, radii, bb[0], bb[1])
    counts = pipe.ctx.sconv_variant_counts()
    want = {s + (4, 1) for s in BENCH_SHAPES16} | {s + (4, 1, 1) for s in BENCH_SPLIT16}
    assert sum(counts.values()) == 44 and set(counts) == want, counts
    for i in range(5):
        s = str(i)
        assert np.array_equal(pipe.get("voxel_keys" + s).cpu().numpy().view(np.uint64), item["voxel_keys" + s])
        for k in ("neighbors_index", "neighbors_kernel_index", "neighbors_row_splits"):
            assert np.array_equal(pipe.get(k + s).cpu().numpy(), item[k + s]), k + s
    assert np.array_equal(pipe.get("aggregation_neighbors_index").cpu().numpy(), item["aggregation_neighbors_index"])
    for k, g in (("code", pipe.get("code")), ("values", values)):
        cpu, new = _stats(ref32[k], exact[k]), _stats(g.cpu().numpy(), exact[k])
        print("10 M points, %s: fp32 oracle %s | bf16x3_2acc %s" % (k, cpu, new))
        assert new["max"] <= cpu["max"], (k, new, cpu)
        assert new["share"] >= cpu["share"], (k, new, cpu)


def _spawn(target, world, *args):
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (out,)) for r in range(world)]
    for p in procs:
        p.start()
    infos = sorted([out.get(timeout=900) for _ in range(world)], key=lambda d: d["rank"])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return infos


@pytest.mark.parametrize("world", [2, 3])
def test_library_sharded_forward_equals_single_process(gpu, world):
    """asr_hip_implicit_forward_sharded, 2 and 3 processes on one GPU: the values equal the one-GPU pipeline bit for bit"""
    infos = _spawn(_native_worker, world, 30000, 1, MODE)
    assert infos[0]["equal"], infos[0]["max_abs_diff"]
    assert all(i["repeat_equal"] for i in infos)
    assert sum(i["stats"]["owned_rows"][0] for i in infos) == infos[0]["v0"]


def test_python_sharded_driver_equals_single_process(gpu):
    """the Python reference driver (HipBackend) at world 2"""
    infos = _spawn(_worker, 2, 30000, 1, MODE)
    assert infos[0]["equal"], infos[0]["max_abs_diff"]


def test_reconstruct_surface_and_asrtool(gpu, tmp_path):
    """the 50 k sphere through reconstruct_surface in the new mode against f32: vertex and triangle counts within 0.1 %,
    >= 99.9 % of either mesh's vertices within 1e-5 of the bounding-box diagonal of a vertex of the other; asrtool
    --precision bf16x3_2acc writes a readable PLY"""
    from scipy.spatial import cKDTree
    import adaptivesurfacereconstruction as asr
    pts, nrm = synth.sphere_cloud(50000, seed=0)
    pts, nrm = np.asarray(pts, np.float32), np.asarray(nrm, np.float32)
    weights = synth.make_weights(4, seed=31)
    m32 = asr.reconstruct_surface(pts, nrm, weights=weights)
    m2 = asr.reconstruct_surface(pts, nrm, weights=weights, precision=MODE)
    for k in ("vertices", "triangles"):
        n32, n2 = len(m32[k]), len(m2[k])
        assert n32 > 100 and abs(n2 - n32) <= 1e-3 * n32, (k, n32, n2)
    v32, v2 = m32["vertices"], m2["vertices"]
    diag = float(np.linalg.norm(v32.max(0) - v32.min(0)))
    for a, b in ((v32, v2), (v2, v32)):
        d, _ = cKDTree(b).query(a)
        assert np.mean(d <= 1e-5 * diag) >= 0.999, np.mean(d <= 1e-5 * diag)
    np.savez(str(tmp_path / "w.npz"), **weights)
    ply.write_points(str(tmp_path / "in.ply"), pts, nrm)
    r = subprocess.run([sys.executable, TOOL, "--in", str(tmp_path / "in.ply"), "--out", str(tmp_path / "out.ply"),
                        "--weights", str(tmp_path / "w.npz"), "--precision", MODE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    v, t = ply.read_mesh(str(tmp_path / "out.ply"))
    assert len(t) > 100 and abs(len(v) - len(v32)) <= 1e-3 * len(v32)
