"""GPU parity, floating point rows (a10, a12-a14) and the whole path: HIP through the C ABI vs the
oracle and vs the committed reference-model fixtures.  Tolerance: north_star asks for implicit
values within 1e-5 (fp32); per-op checks use 1e-5 absolute on O(1) activations plus a relative
check, summation order being the only difference."""
import os

import numpy as np
import pytest
import torch

import parity
from asr_hip import synth
from oracle import oracle as O
from sconv_lists import dense_autograd_reference

pytestmark = pytest.mark.gpu

ATOL = 1e-5


_close = parity.assert_close
_close_scaled = parity.assert_close_scaled


def _t(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.fixture(scope="module")
def geo():
    p, q = synth.scan_cloud(6000, seed=11, device="cpu")
    pts, nrm = p.numpy(), q.numpy()
    rad = synth.knn_radii(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    item = parity.oracle_geometry(pts, rad, *bb)
    return pts, nrm, rad, bb, item


def test_aggregation_importance_and_continuous_conv(geo, gpu):
    from asr_hip import ops
    pts, nrm, rad, bb, item = geo
    rng = np.random.default_rng(0)
    imp = ops.aggregation_importance(_t(item["aggregation_scale_compat"], gpu),
                                     _t(item["aggregation_neighbors_dist"], gpu))
    imp_ref = (item["aggregation_scale_compat"] * O.window_poly6(item["aggregation_neighbors_dist"]))
    _close(imp.cpu().numpy(), imp_ref, 1e-7)
    feats = np.concatenate([nrm, np.ones((len(pts), 1), np.float32)], 1)
    for cout in (8, 32, 5, 20):  # (widths that leave lanes of the contraction's output blocks idle too)
        W = (rng.standard_normal((4, 4, 4, 4, cout)) * 0.7).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32) * 0.1
        for nimp, normalize in ((imp_ref.astype(np.float32), True), (None, True), (None, False)):
            out = ops.continuous_conv(_t(W, gpu), _t(item["voxel_centers0"], gpu),
                                      _t(item["voxel_sizes0"], gpu), _t(pts, gpu), _t(feats, gpu),
                                      _t(item["aggregation_neighbors_index"], gpu),
                                      _t(nimp, gpu) if nimp is not None else None,
                                      _t(item["aggregation_row_splits"], gpu), normalize, bias=_t(b, gpu),
                                      relu=True)
            ref = O.continuous_conv(W, item["voxel_centers0"], item["voxel_sizes0"], pts, feats,
                                    item["aggregation_neighbors_index"], nimp,
                                    item["aggregation_row_splits"], normalize)
            ref = np.maximum(ref + b, 0)
            _close(out.cpu().numpy(), ref, 2e-5 if not normalize else ATOL)
    # rows without neighbours give relu(bias)
    empty = np.diff(item["aggregation_row_splits"]) == 0
    if empty.any():
        assert np.allclose(out.cpu().numpy()[empty], np.maximum(b, 0))


def test_continuous_conv_ragged_and_long_rows(gpu):
    """rows of 0 .. 6000 neighbours: rows above 256 pairs (CCONV_HEAVY) take the 16-wave long-row kernels, which cut a
    row into segments of 4096 pairs (CCH_SEG): 6000 is two segments.  The values next to these constants are in
    tests/test_gpu_cconv.py."""
    from asr_hip import ops
    rng = np.random.default_rng(3)
    n, cin, cout = 8000, 4, 32
    pos = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    feat = rng.standard_normal((n, cin)).astype(np.float32)
    lens = np.array([0, 3, 1500, 1, 6000, 1024, 1025, 0, 64, 2500])
    v = len(lens)
    out_pos = rng.uniform(-0.3, 0.3, size=(v, 3)).astype(np.float32)
    ext = rng.uniform(1.5, 3.0, size=v).astype(np.float32)
    rs = np.zeros(v + 1, np.int64)
    rs[1:] = np.cumsum(lens)
    idx = np.concatenate([rng.choice(n, size=l, replace=False) for l in lens]).astype(np.int32)
    imp = rng.uniform(0.1, 1, size=rs[-1]).astype(np.float32)
    W = (rng.standard_normal((4, 4, 4, cin, cout)) * 0.5).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    for nimp, normalize in ((imp, True), (None, False)):
        out = ops.continuous_conv(_t(W, gpu), _t(out_pos, gpu), _t(ext, gpu), _t(pos, gpu), _t(feat, gpu),
                                  _t(idx, gpu), _t(nimp, gpu) if nimp is not None else None, _t(rs, gpu),
                                  normalize, bias=_t(b, gpu), relu=True)
        ref = np.maximum(O.continuous_conv(W, out_pos, ext, pos, feat, idx, nimp, rs, normalize) + b, 0)
        _close(out.cpu().numpy(), ref, 2e-5)


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("cin,cout", [(32, 56), (32, 8), (64, 64), (128, 120), (12, 20), (256, 256)])
def test_sparse_conv_k55(geo, gpu, algo, cin, cout):
    from asr_hip import ops
    pts, nrm, rad, bb, item = geo
    level = 0 if cin <= 64 else 1
    idx, kidx, rs = (item["neighbors_index%d" % level], item["neighbors_kernel_index%d" % level],
                     item["neighbors_row_splits%d" % level])
    v = len(rs) - 1
    rng = np.random.default_rng(cin * 1000 + cout)
    f = rng.standard_normal((v, cin)).astype(np.float32)
    W = (rng.standard_normal((55, cin, cout)) * np.sqrt(2.0 / (8 * cin))).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    imp = rng.uniform(0.05, 1.0, size=v).astype(np.float32)
    # plain conv + bias + relu
    out = ops.sparse_conv(_t(W, gpu), _t(f, gpu), _t(idx, gpu), _t(kidx, gpu), _t(rs, gpu),
                          bias=_t(b, gpu), relu=True, algo=algo)
    ref = np.maximum(O.sparse_conv(W, f, idx, kidx, None, rs, False) + b, 0)
    _close(out.cpu().numpy(), ref)
    # importance weighted + normalised (conv1b), importance sum returned
    out, oimp = ops.sparse_conv(_t(W, gpu), _t(f, gpu), _t(idx, gpu), _t(kidx, gpu), _t(rs, gpu),
                                inp_importance=_t(imp, gpu), normalize=True, bias=_t(b, gpu), relu=True,
                                return_importance=True, algo=algo)
    nimp = imp[idx.astype(np.int64)]
    ref = np.maximum(O.sparse_conv(W, f, idx, kidx, nimp, rs, True) + b, 0)
    _close(out.cpu().numpy(), ref)
    _close(oimp.cpu().numpy(), O.reduce_subarrays_sum(nimp, rs), 1e-5)
    # row regrouping changes the tiling only: identical bits with and without the permutation
    if algo == 2:
        perm = ops.row_groups(_t(kidx, gpu), _t(rs, gpu), 256)
        assert sorted(perm.cpu().tolist()) == list(range(v))
        out_p, oimp_p = ops.sparse_conv(_t(W, gpu), _t(f, gpu), _t(idx, gpu), _t(kidx, gpu), _t(rs, gpu),
                                        inp_importance=_t(imp, gpu), normalize=True, bias=_t(b, gpu),
                                        relu=True, return_importance=True, algo=2, row_perm=perm)
        assert torch.equal(out_p, out) and torch.equal(oimp_p, oimp)
    # per-pair importance (open3d::sparse_conv signature), no normalisation, no activation
    pimp = rng.uniform(0.05, 1.0, size=len(idx)).astype(np.float32)
    out = ops.sparse_conv(_t(W, gpu), _t(f, gpu), _t(idx, gpu), _t(kidx, gpu), _t(rs, gpu),
                          neighbors_importance=_t(pimp, gpu), algo=algo)
    _close(out.cpu().numpy(), O.sparse_conv(W, f, idx, kidx, pimp, rs, False))


@pytest.mark.parametrize("cin,ca", [(32, 56), (16, 8), (64, 120), (128, 248)])
def test_sparse_conv_two_banks_equals_two_launches(geo, gpu, cin, ca):
    """conv1a + conv1b fused (second filter bank): same bits as the two separate launches, and both
    against the oracle"""
    from asr_hip import ops
    pts, nrm, rad, bb, item = geo
    rng = np.random.default_rng(5)
    L = 1
    idx, kidx, rs = item["neighbors_index%d" % L], item["neighbors_kernel_index%d" % L], item["neighbors_row_splits%d" % L]
    v = len(rs) - 1
    f = rng.normal(size=(v, cin)).astype(np.float32)
    Wa = (rng.normal(size=(55, cin, ca)) * 0.1).astype(np.float32)
    Wb = (rng.normal(size=(55, cin, 8)) * 0.1).astype(np.float32)
    ba, bb_ = rng.normal(size=ca).astype(np.float32), rng.normal(size=8).astype(np.float32)
    imp = rng.uniform(0.05, 1.0, size=v).astype(np.float32)
    perm = ops.row_groups(_t(kidx, gpu), _t(rs, gpu))
    common = (_t(idx, gpu), _t(kidx, gpu), _t(rs, gpu))
    out, oimp = ops.sparse_conv(_t(Wa, gpu), _t(f, gpu), *common, inp_importance=_t(imp, gpu), normalize=True,
                                bias=_t(ba, gpu), relu=True, return_importance=True, algo=2, row_perm=perm,
                                filters_b=_t(Wb, gpu), bias_b=_t(bb_, gpu))
    assert out.shape == (v, ca + 8)
    oa = ops.sparse_conv(_t(Wa, gpu), _t(f, gpu), *common, bias=_t(ba, gpu), relu=True, algo=2, row_perm=perm)
    ob, oimp2 = ops.sparse_conv(_t(Wb, gpu), _t(f, gpu), *common, inp_importance=_t(imp, gpu), normalize=True,
                                bias=_t(bb_, gpu), relu=True, return_importance=True, algo=2, row_perm=perm)
    assert torch.equal(out[:, :ca], oa) and torch.equal(out[:, ca:], ob) and torch.equal(oimp, oimp2)
    ones = np.ones(len(idx), np.float32)
    _close(out[:, :ca].cpu().numpy(), np.maximum(O.sparse_conv(Wa, f, idx, kidx, ones, rs, False) + ba, 0))
    _close(out[:, ca:].cpu().numpy(), np.maximum(O.sparse_conv(Wb, f, idx, kidx, imp[idx.astype(np.int64)], rs, True) + bb_, 0))
    with pytest.raises(RuntimeError):  # widths the fused kernel does not take
        ops.sparse_conv(_t(np.zeros((55, cin, 16), np.float32), gpu), _t(f, gpu), *common,
                        inp_importance=_t(imp, gpu), algo=2, filters_b=_t(Wb, gpu))


def test_sparse_conv_strided_io_residual_and_k9(geo, gpu):
    from asr_hip import ops
    pts, nrm, rad, bb, item = geo
    rng = np.random.default_rng(5)
    v0, v1 = len(item["voxel_sizes0"]), len(item["voxel_sizes1"])
    up = (item["up_neighbors_index0"], item["up_neighbors_kernel_index0"], item["up_neighbors_row_splits0"])
    d_idx, d_rs, d_attr = O.invert_neighbors_list(v1, up[0], up[2], up[1])
    cin, cout = 64, 128
    W = (rng.standard_normal((9, cin, cout)) * np.sqrt(2.0 / cin)).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    # down: rows = coarse voxels; input is a column slice of a wider buffer (zero-copy concat)
    wide = rng.standard_normal((v0, 96)).astype(np.float32)
    wide_t = _t(wide, gpu)
    # strided views would be made contiguous by the tensor wrapper: call the ABI with explicit strides
    from asr_hip import _lib
    import ctypes
    a = _lib.SparseConvArgs()
    Wt, bt = _t(W, gpu), _t(b, gpu)
    di, da, dr = _t(d_idx, gpu), _t(d_attr, gpu), _t(d_rs, gpu)
    res = rng.standard_normal((v1, cout)).astype(np.float32)
    res_t = _t(res, gpu)
    out_wide = torch.zeros((v1, cout + 16), dtype=torch.float32, device=gpu)
    for algo in (1, 2):
        out_wide.zero_()
        a.filters, a.inp_features, a.inp_ld = Wt.data_ptr(), wide_t.data_ptr() + 32 * 4, 96
        a.inp_importance = None
        a.neighbors_importance = None
        a.neighbors_index, a.neighbors_kernel_index, a.neighbors_row_splits = di.data_ptr(), da.data_ptr(), dr.data_ptr()
        a.num_out, a.num_inp, a.kernel_size, a.cin, a.cout = v1, v0, 9, cin, cout
        a.normalize, a.bias, a.relu = 0, bt.data_ptr(), 1
        a.residual, a.residual_ld = res_t.data_ptr(), cout
        a.out, a.out_ld, a.out_importance, a.algo = out_wide.data_ptr() + 16 * 4, cout + 16, None, algo
        ops.context().call("asr_hip_sparse_conv_f32", ctypes.byref(a))
        ref = np.maximum(O.sparse_conv(W, np.ascontiguousarray(wide[:, 32:]), d_idx, d_attr, None, d_rs, False) + b, 0) + res
        got = out_wide.cpu().numpy()
        _close(got[:, 16:], ref)
        assert np.all(got[:, :16] == 0)  # columns outside the slice untouched
    # up: rows = fine voxels, one entry per row, slots 0..8
    f1 = rng.standard_normal((v1, cin)).astype(np.float32)
    out = ops.sparse_conv(Wt, _t(f1, gpu), _t(up[0], gpu), _t(up[1], gpu), _t(up[2], gpu), bias=bt, relu=True)
    _close(out.cpu().numpy(), np.maximum(O.sparse_conv(W, f1, up[0], up[1], None, up[2], False) + b, 0))


def test_reduce_and_decode(geo, gpu):
    from asr_hip import ops
    pts, nrm, rad, bb, item = geo
    rng = np.random.default_rng(6)
    rs, idx = item["neighbors_row_splits0"], item["neighbors_index0"]
    vals = rng.uniform(0, 1, size=len(idx)).astype(np.float32)
    _close(ops.reduce_subarrays_sum(_t(vals, gpu), _t(rs, gpu)).cpu().numpy(), O.reduce_subarrays_sum(vals, rs))
    per_v = rng.uniform(0, 1, size=len(rs) - 1).astype(np.float32)
    _close(ops.reduce_subarrays_sum(_t(per_v, gpu), _t(rs, gpu), _t(idx, gpu)).cpu().numpy(),
           O.reduce_subarrays_sum(per_v[idx], rs))
    w = synth.make_weights(1, seed=4)
    code = rng.standard_normal((len(rs) - 1, 32)).astype(np.float32)
    args = [w["dense_decoder1.weight"], w["dense_decoder1.bias"], w["dense_decoder2.weight"],
            w["dense_decoder2.bias"], w["dense_decoder3.weight"]]
    out = ops.decode_mlp(_t(code, gpu), *[_t(x, gpu) for x in args], voxel_sizes=_t(item["voxel_sizes0"], gpu))
    _close(out.cpu().numpy(), O.decode(code, *args, item["voxel_sizes0"]))


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("tag", ["d4_3k", "d1_2k"])
def test_whole_path_against_reference_model_fixture(golden_dir, gpu, tag, precision):
    """points/normals/radii -> values through asr_hip_implicit_forward vs the outputs of the
    reference's own model code over the oracle ops (tests/golden/make_unet_fixture.py), for the exact f32 kernel and
    the two split arithmetics (fp32-class: the same tolerance)"""
    from asr_hip.pipeline import ImplicitPipeline
    fx = np.load(os.path.join(golden_dir, "unet_%s.npz" % tag))
    d = int(fx["channel_div"])
    weights = synth.make_weights(d, seed=int(fx["seed"]))
    pipe = ImplicitPipeline(weights, device=gpu, precision=precision)
    values = pipe.forward(_t(fx["points"], gpu), _t(fx["normals"], gpu), _t(fx["radii"], gpu),
                          fx["bb_min"], fx["bb_max"])
    torch.cuda.synchronize()
    # integer structures: bit exact
    for k in fx.files:
        if not k.startswith("geom_"):
            continue
        name = k[5:]
        got = pipe.get(name).cpu().numpy()
        ref = fx[k]
        if name.startswith("voxel_keys"):
            got = got.view(np.uint64)
        if name == "aggregation_scale_compat":
            _close(got, ref, 1e-6)
        else:
            assert np.array_equal(got, ref), name
    _close(pipe.get("feats1").cpu().numpy(), fx["out_feats1"])
    _close(pipe.get("importance").cpu().numpy(), fx["out_importance"], 1e-6)
    _close_scaled(pipe.get("code").cpu().numpy(), fx["out_code"])
    if d == 1:
        _close(values.cpu().numpy(), fx["out_values"])   # 1e-5, the north_star tolerance
    ms = pipe.stage_ms()
    assert all(v >= 0 for v in ms.values())


def test_model_pt_archive_reproduces_the_fixture(golden_dir, gpu, tmp_path):
    """weights delivered as the reference delivers them -- a TorchScript archive with the state_dict names of
    UNet5 (cpp/lib/asr.cpp:138-139) -- loaded by the module's loader, give the fixture's values"""
    import adaptivesurfacereconstruction as asr
    from asr_hip.pipeline import ImplicitPipeline
    fx = np.load(os.path.join(golden_dir, "unet_d1_2k.npz"))
    path = str(tmp_path / "model.pt")
    parity.save_torchscript_weights(synth.make_weights(int(fx["channel_div"]), seed=int(fx["seed"])), path)
    pipe = ImplicitPipeline(asr._load_weights(path), device=gpu)
    values = pipe.forward(_t(fx["points"], gpu), _t(fx["normals"], gpu), _t(fx["radii"], gpu), fx["bb_min"], fx["bb_max"])
    _close(values.cpu().numpy(), fx["out_values"])


@pytest.mark.parametrize("kernel", ["f32", "bf16x3", "f16x2"])
def test_every_layer_of_the_reference_graph_separately(gpu, kernel):
    """the 53 SpecialSparseConv calls of the reference's UNet5 graph (tests/golden/unet_layers_d4_1k.npz, recorded
    from the reference's own model code), each one through the HIP sparse conv with the call's own inputs:
    within 1e-5 of the recorded output, for the f32-input MFMA kernel and for the two split arithmetics"""
    import layer_fixture
    from asr_hip import ops
    for l in layer_fixture.load():
        idx, kidx, rs = (_t(a, gpu) for a in l["csr"])
        imp = _t(l["imp"], gpu) if l["imp"] is not None else None
        cin, cout = l["kernel"].shape[1:]
        if kernel == "f32" or cin % 4:
            r = ops.sparse_conv(_t(l["kernel"], gpu), _t(l["inp"], gpu), idx, kidx, rs, inp_importance=imp,
                                normalize=l["normalize"], bias=_t(l["bias"], gpu), relu=True,
                                return_importance=imp is not None)
        else:
            packed = ops.pack_filters(_t(l["kernel"], gpu), kernel)
            r = ops.sparse_conv16(kernel, packed, l["K"], cin, cout, _t(l["inp"], gpu), idx, kidx, rs,
                                  inp_importance=imp, normalize=l["normalize"], bias=_t(l["bias"], gpu), relu=True,
                                  return_importance=imp is not None)
        out, oimp = r if imp is not None else (r, None)
        _close(out.cpu().numpy(), l["out"])
        if oimp is not None:
            _close(oimp.cpu().numpy(), l["oimp"])


def test_batched_tiling_orders_equal_the_per_csr_routine(gpu):
    """implicit_build computes the MFMA tiling orders of all 13 CSRs in one batched sort; each must equal
    asr_hip_row_groups on that CSR alone (and be a permutation of the rows)"""
    from asr_hip import ops
    from asr_hip.pipeline import ImplicitPipeline
    p, q = synth.scan_cloud(40000, seed=12, device=gpu)
    rad = synth.knn_radii_gpu(p, 24)
    bb = synth.bounding_box(p, 0.1)
    pipe = ImplicitPipeline(synth.make_weights(4, seed=1), device=gpu)
    for seg in (0, 4096):
        if seg:
            pipe.ctx.set_option("row_segment", seg)
        pipe.build(p, rad, bb[0], bb[1])
        for i in range(5):
            names = [("tiling%d" % i, "neighbors")] + ([("tiling_up%d" % i, "up_neighbors"), ("tiling_down%d" % i, "down_neighbors")] if i < 4 else [])
            for tname, pre in names:
                got = pipe.get(tname)
                want = ops.row_groups(pipe.get("%s_kernel_index%d" % (pre, i)), pipe.get("%s_row_splits%d" % (pre, i)), seg)
                assert torch.equal(got, want), (tname, seg)
                assert torch.equal(torch.sort(got.long()).values, torch.arange(got.numel(), device=gpu))


def test_sparse_conv_backward_against_torch_autograd(geo, gpu):
    """"next" row f4: gradients of open3d::sparse_conv / reduce_subarrays_sum (models/common_torch.py:127-142) with
    respect to features and filters, against torch autograd over a dense fp64 restatement of the same sum"""
    import open3d.ml.torch as ml3d
    pts, nrm, rad, bb, item = geo
    rng = np.random.default_rng(17)
    # (level, cin, cout, neighbour importance, normalize); normalize without importance divides by the neighbour count
    for level, cin, cout, with_imp, normalize in ((2, 8, 12, True, True), (3, 16, 8, False, False), (2, 8, 8, False, True),
                                                  (3, 8, 8, True, False)):
        idx, kidx, rs = (item["neighbors_index%d" % level], item["neighbors_kernel_index%d" % level],
                         item["neighbors_row_splits%d" % level])
        v = len(rs) - 1
        f0 = rng.standard_normal((v, cin)).astype(np.float32)
        W0 = (rng.standard_normal((55, cin, cout)) * 0.2).astype(np.float32)
        imp = rng.uniform(0.1, 1.0, size=len(idx)).astype(np.float32)
        gout = rng.standard_normal((v, cout)).astype(np.float32)
        empty = torch.empty((0,), dtype=torch.float32, device=gpu)
        f = _t(f0, gpu).requires_grad_(True)
        W = _t(W0, gpu).requires_grad_(True)
        nimp = _t(imp, gpu) if with_imp else empty
        out = ml3d.ops.sparse_conv(filters=W, inp_features=f, inp_importance=empty, neighbors_index=_t(idx, gpu),
                                   neighbors_kernel_index=_t(kidx, gpu), neighbors_importance=nimp,
                                   neighbors_row_splits=_t(rs, gpu), normalize=normalize)
        out.backward(_t(gout, gpu))
        # dense fp64 reference on the CPU
        ref, f_grad, W_grad = dense_autograd_reference(f0, W0, idx, kidx, rs, imp if with_imp else None, normalize, gout)
        _close(out.detach().cpu().numpy(), ref)
        _close(f.grad.cpu().numpy(), f_grad, 2e-5, 2e-5)
        _close(W.grad.cpu().numpy(), W_grad, 2e-5, 2e-5)
    vals = _t(rng.uniform(0, 1, size=len(idx)).astype(np.float32), gpu).requires_grad_(True)
    s = ml3d.ops.reduce_subarrays_sum(vals, _t(rs, gpu))
    s.backward(torch.arange(v, dtype=torch.float32, device=gpu))
    assert torch.equal(vals.grad, torch.repeat_interleave(torch.arange(v, dtype=torch.float32, device=gpu),
                                                          _t(np.diff(rs), gpu)))


def test_continuous_conv_filter_gradient(geo, gpu):
    """"next" row f4: the continuous conv is linear in its filters, so <dL/dW, D> must equal L(W + D) - L(W) for any
    direction D (L = sum(out * g)); the gradient comes from the HIP basis kernel + one GEMM"""
    import open3d.ml.torch as ml3d
    pts, nrm, rad, bb, item = geo
    rng = np.random.default_rng(23)
    feats = _t(np.concatenate([nrm, np.ones((len(pts), 1), np.float32)], 1), gpu)
    nimp = _t(rng.uniform(0.1, 1, size=len(item["aggregation_neighbors_index"])).astype(np.float32), gpu)
    args = dict(out_positions=_t(item["voxel_centers0"], gpu), extents=_t(item["voxel_sizes0"], gpu),
                offset=torch.zeros(3, device=gpu), inp_positions=_t(pts, gpu), inp_features=feats,
                inp_importance=torch.empty((0,), device=gpu), neighbors_index=_t(item["aggregation_neighbors_index"], gpu),
                neighbors_importance=nimp, neighbors_row_splits=_t(item["aggregation_row_splits"], gpu),
                align_corners=True, coordinate_mapping="ball_to_cube_radial", interpolation="linear")
    for normalize in (True, False):
        W = _t((rng.standard_normal((4, 4, 4, 4, 32)) * 0.3).astype(np.float32), gpu).requires_grad_(True)
        D = _t((rng.standard_normal((4, 4, 4, 4, 32)) * 0.3).astype(np.float32), gpu)
        g = _t(rng.standard_normal((len(item["voxel_sizes0"]), 32)).astype(np.float32), gpu)
        out = ml3d.ops.continuous_conv(filters=W, normalize=normalize, **args)
        (out * g).sum().backward()
        with torch.no_grad():
            l0 = (out.double() * g.double()).sum()
            l1 = (ml3d.ops.continuous_conv(filters=W + D, normalize=normalize, **args).double() * g.double()).sum()
            want = float(l1 - l0)
            got = float((W.grad.double() * D.double()).sum())
        assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (normalize, got, want)
    with pytest.raises(RuntimeError):  # gradients with respect to the point features are not implemented
        f = feats.clone().requires_grad_(True)
        a2 = dict(args, inp_features=f)
        ml3d.ops.continuous_conv(filters=W.detach(), normalize=True, **a2).sum().backward()


def test_octree_handles_are_self_contained(gpu):
    """module.cpp:230-235: create_dual_vertex_indices works on any live tree, however many were built since
    (models/v0/datareader.py:224-243,802 keeps trees across calls)"""
    import adaptivesurfacereconstruction as asr
    trees, want = [], []
    for seed in (1, 2, 3):
        p, _ = synth.scan_cloud(3000 + 500 * seed, seed=seed, device="cpu")
        pts = p.numpy()
        rad = synth.knn_radii(pts, 24)
        bb = synth.bounding_box(pts, 0.1)
        trees.append(asr.create_octree(pts, rad, bb[0], bb[1]))
        o = O.Oracle()
        o.build_octree(pts, rad, *bb)
        o.create_grids(1)
        want.append(o.create_dual_vertex_indices())
    for tree, w in zip(trees, want):  # oldest first, after all three were built
        got = asr.create_dual_vertex_indices(tree)
        assert got.dtype == np.uint64 and np.array_equal(got, w.astype(np.uint64))


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_whole_path_against_oracle_fresh_cloud(gpu, precision):
    from asr_hip.pipeline import ImplicitPipeline
    p, q = synth.scan_cloud(20000, seed=21, device="cpu", density_variance=10.0)
    pts, nrm = p.numpy(), q.numpy()
    rad = synth.knn_radii(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    weights = synth.make_weights(2, seed=21)
    with O.precise():  # double-accumulating checker: see parity.assert_close_scaled
        ref = parity.oracle_forward(pts, nrm, rad, bb[0], bb[1], weights)
    pipe = ImplicitPipeline(weights, device=gpu, precision=precision)
    values = pipe.forward(_t(pts, gpu), _t(nrm, gpu), _t(rad, gpu), bb[0], bb[1]).clone()
    assert np.array_equal(pipe.get("voxel_keys0").cpu().numpy().view(np.uint64), ref["voxel_keys0"])
    assert np.array_equal(pipe.get("aggregation_neighbors_index").cpu().numpy(), ref["aggregation_neighbors_index"])
    _close(pipe.get("feats1").cpu().numpy(), ref["feats1"])
    _close_scaled(pipe.get("code").cpu().numpy(), ref["code"])
    _close_scaled(values.cpu().numpy(), ref["values"])
    # running twice on the same context gives identical bits (deterministic kernels, arena reuse; f16x2: the running
    # maxima are order-independent)
    v2 = pipe.forward(_t(pts, gpu), _t(nrm, gpu), _t(rad, gpu), bb[0], bb[1])
    assert torch.equal(values, v2)


def test_reconstruct_surface_end_to_end(gpu):
    """module.cpp:291-346: pre-filter -> values -> contouring -> component filter.  The mesh is compared
    bit for bit with the serial restatement run on the SAME values (north_star: indexing bit-exact given
    identical values); the values themselves are covered by the 1e-5 tests above."""
    import adaptivesurfacereconstruction as asr
    from asr_hip.pipeline import ImplicitPipeline
    p, q = synth.scan_cloud(6000, seed=31, device="cpu")
    pts, nrm = p.numpy(), q.numpy()
    weights = synth.make_weights(4, seed=31)
    for given_radii in (False, True):
        if given_radii:
            rad_in = O.knn_radius(pts, 24)
            counts = O.radius_count(pts, rad_in)
            from asr_hip import ops
            inl = ops.density_inlier(counts, 10.0)
            out = asr.reconstruct_surface(pts, nrm, rad_in, weights=weights, keep_n_connected_components=4)
            rad = rad_in
        else:
            rad = O.knn_radius(pts, 24)
            d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2)
            d2 = (d2[..., 0] + d2[..., 1]) + d2[..., 2]
            order = np.argsort(d2, axis=1, kind="stable")[:, :24]  # exactly k, ties by index
            votes = (rad[order] < (rad * np.float32(0.5))[:, None]).sum(1)
            inl = votes < 1
            out = asr.reconstruct_surface(pts, nrm, weights=weights, keep_n_connected_components=4)
        fp, fn, fr = pts[inl], nrm[inl], rad[inl]
        bb = (fp.min(0), fp.max(0))
        pipe = ImplicitPipeline(weights, device=gpu)
        values = pipe.forward(_t(fp, gpu), _t(fn, gpu), _t(fr, gpu), *bb).cpu().numpy()
        o = O.Oracle()
        o.build_octree(fp, fr, *bb)
        g0 = o.create_grids(1)[0]
        du = o.create_dual_vertex_indices().astype(np.int64)
        assert np.array_equal(pipe.dual_cells().cpu().numpy(), du)
        v, t = O.create_triangle_mesh(values, du, g0["voxel_centers"], 1.0)
        v, t = O.remove_connected_components(v, t, 4, 3)
        assert out["vertices"].dtype == np.float32 and out["triangles"].dtype == np.int32
        assert t.shape[0] > 100
        assert np.array_equal(out["vertices"].view(np.uint32), v.view(np.uint32))
        assert np.array_equal(out["triangles"], t)
    with pytest.raises(RuntimeError):
        asr.reconstruct_surface(pts[:0], nrm[:0], weights=weights)
    with pytest.raises(ValueError):
        asr.reconstruct_surface(pts, nrm[:10], weights=weights)
    with pytest.raises(RuntimeError):
        asr.reconstruct_surface(pts, nrm)  # no weights anywhere


def test_pipeline_errors(gpu):
    from asr_hip.pipeline import ImplicitPipeline
    from asr_hip._lib import AsrHipError
    w = synth.make_weights(4, seed=1)
    pipe = ImplicitPipeline(w, device=gpu)
    z = torch.zeros((10, 3), device=gpu)
    with pytest.raises(ValueError):
        pipe.forward(z, torch.zeros((9, 3), device=gpu), torch.zeros(10, device=gpu), [0, 0, 0], [1, 1, 1])
    with pytest.raises(RuntimeError):  # "points is null!" cpp/lib/asr.cpp:101-103
        pipe.forward(torch.zeros((0, 3), device=gpu), torch.zeros((0, 3), device=gpu),
                     torch.zeros(0, device=gpu), [0, 0, 0], [1, 1, 1])
    bad = dict(w)
    del bad["sparseconv_up2.conv1.kernel"]
    pipe2 = ImplicitPipeline(bad, device=gpu)
    p, q = synth.scan_cloud(2000, seed=2, device="cpu")
    rad = synth.knn_radii(p.numpy(), 24)
    bb = synth.bounding_box(p.numpy(), 0.1)
    with pytest.raises(AsrHipError, match="missing weight"):
        pipe2.forward(p.to(gpu), q.to(gpu), torch.from_numpy(rad).to(gpu), bb[0], bb[1])


def test_open3d_facade_ops_on_gpu(geo, gpu):
    """the registered torch ops (B1 boundary) serve GPU tensors from libasr_hip.so"""
    import open3d.ml.torch as ml3d
    pts, nrm, rad, bb, item = geo
    rng = np.random.default_rng(8)
    idx, kidx, rs = item["neighbors_index0"], item["neighbors_kernel_index0"], item["neighbors_row_splits0"]
    v = len(rs) - 1
    f = rng.standard_normal((v, 32)).astype(np.float32)
    W = (rng.standard_normal((55, 32, 56)) * 0.1).astype(np.float32)
    empty = torch.empty((0,), dtype=torch.float32, device=gpu)
    imp = rng.uniform(0.1, 1, size=len(idx)).astype(np.float32)
    out = ml3d.ops.sparse_conv(filters=_t(W, gpu), inp_features=_t(f, gpu), inp_importance=empty,
                               neighbors_index=_t(idx, gpu), neighbors_kernel_index=_t(kidx, gpu),
                               neighbors_importance=_t(imp, gpu), neighbors_row_splits=_t(rs, gpu),
                               normalize=True)
    _close(out.cpu().numpy(), O.sparse_conv(W, f, idx, kidx, imp, rs, True))
    s = ml3d.ops.reduce_subarrays_sum(_t(imp, gpu), _t(rs, gpu))
    _close(s.cpu().numpy(), O.reduce_subarrays_sum(imp, rs))
    v1 = len(item["voxel_sizes1"])
    ans = ml3d.ops.invert_neighbors_list(v1, _t(item["up_neighbors_index0"], gpu),
                                         _t(item["up_neighbors_row_splits0"], gpu),
                                         _t(item["up_neighbors_kernel_index0"], gpu))
    o = O.invert_neighbors_list(v1, item["up_neighbors_index0"], item["up_neighbors_row_splits0"],
                                item["up_neighbors_kernel_index0"])
    assert np.array_equal(ans.neighbors_index.cpu().numpy(), o[0])
    assert np.array_equal(ans.neighbors_row_splits.cpu().numpy(), o[1])
    assert np.array_equal(ans.neighbors_attributes.cpu().numpy(), o[2])
    conv = ml3d.layers.ContinuousConv(in_channels=4, filters=16, kernel_size=[4, 4, 4],
                                      activation=torch.relu, coordinate_mapping='ball_to_cube_radial',
                                      normalize=True).to(gpu)
    feats = np.concatenate([nrm, np.ones((len(pts), 1), np.float32)], 1)
    nimp = rng.uniform(0.1, 1, size=len(item["aggregation_neighbors_index"])).astype(np.float32)
    with torch.no_grad():
        y = conv(_t(feats, gpu), _t(pts, gpu), _t(item["voxel_centers0"], gpu),
                 extents=_t(item["voxel_sizes0"], gpu),
                 user_neighbors_index=_t(item["aggregation_neighbors_index"], gpu),
                 user_neighbors_row_splits=_t(item["aggregation_row_splits"], gpu),
                 user_neighbors_importance=_t(nimp, gpu))
    ref = O.continuous_conv(conv.kernel.detach().cpu().numpy(), item["voxel_centers0"], item["voxel_sizes0"],
                            pts, feats, item["aggregation_neighbors_index"], nimp,
                            item["aggregation_row_splits"], True)
    _close(y.cpu().numpy(), np.maximum(ref + conv.bias.detach().cpu().numpy(), 0))
    with pytest.raises(NotImplementedError):  # no CPU kernel in the product facade
        ml3d.ops.reduce_subarrays_sum(torch.zeros(3), torch.tensor([0, 3]))


@pytest.mark.parametrize("n", [1, 2, 9, 65, 300])
def test_whole_path_tiny_clouds(gpu, n):
    """degenerate sizes: a handful of points still gives the oracle's grids and values (single voxel
    levels, rows shorter than a wave, empty coarse grids' neighbours)"""
    from asr_hip.pipeline import ImplicitPipeline
    rng = np.random.default_rng(n)
    pts = rng.uniform(-0.5, 0.5, size=(n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rad = rng.uniform(0.02, 0.1, size=n).astype(np.float32)
    bb = (np.full(3, -0.6, np.float32), np.full(3, 0.6, np.float32))
    weights = synth.make_weights(4, seed=3)
    pipe = ImplicitPipeline(weights, device=gpu)
    try:
        ref = parity.oracle_forward(pts, nrm, rad, bb[0], bb[1], weights)
    except IndexError:
        # the per-pair importance array is indexed with voxel indices; with fewer aggregation
        # pairs than voxels the reference indexes out of bounds -- the library reports that as an error
        with pytest.raises(RuntimeError):
            pipe.forward(_t(pts, gpu), _t(nrm, gpu), _t(rad, gpu), bb[0], bb[1])
        return
    values = pipe.forward(_t(pts, gpu), _t(nrm, gpu), _t(rad, gpu), bb[0], bb[1])
    for i in range(5):
        assert np.array_equal(pipe.get("voxel_keys%d" % i).cpu().numpy().view(np.uint64), ref["voxel_keys%d" % i])
        assert np.array_equal(pipe.get("neighbors_index%d" % i).cpu().numpy(), ref["neighbors_index%d" % i])
    assert np.array_equal(pipe.get("aggregation_neighbors_index").cpu().numpy(), ref["aggregation_neighbors_index"])
    _close(values.cpu().numpy(), ref["values"])
    v, t = pipe.mesh()
    duals = pipe.dual_cells().cpu().numpy()
    o = O.Oracle()
    o.build_octree(pts, rad, bb[0], bb[1])
    o.create_grids(1)
    assert np.array_equal(duals, o.create_dual_vertex_indices().astype(np.int64))
    wv, wt = O.create_triangle_mesh(values.cpu().numpy(), duals, pipe.get("voxel_centers0").cpu().numpy(), 1.0)
    wv, wt = O.remove_connected_components(wv, wt, 2**63 - 1, 3)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), wv.view(np.uint32)) and np.array_equal(t.cpu().numpy(), wt)
