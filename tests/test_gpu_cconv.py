"""Continuous conv (row a10, asr_conv.hip): every kernel family behind asr_hip_continuous_conv_f32 and the whole path's
first stage against the CPU oracle under O.precise() (double accumulation, any cin / cout), at the row lengths where
the kernels change path.

The constants the row lengths are chosen around (asr_conv.hip):
  CCONV_HEAVY = 256   a row of 256 pairs stays in the light kernel, 257 goes to the long-row kernels
  CCH_SEG = 4096      a long row of the matrix-core path is cut into segments of 4096 pairs (4096: one, 4097: two)
  64 pairs            one batch of a wave; 16 x 64 = 1024 pairs per round of a 16-wave block
  8192 rows           512 blocks x 16 waves of the general kernel: its grid-stride loop runs twice only above that

Which test runs which kernel instance (AoS = the public operator, Morton = the whole path's 32-byte records):
  k_cconv_mfma<false,4>                       test_row_length_boundaries (4,32) (4,5), test_geometry_edges (4,16),
                                              test_whole_path_layouts_agree
  k_cconv_heavy4_items, k_cconv_heavy4<32,false>, k_cconv_heavy4_finish<32>
                                              test_row_length_boundaries (4,32) (4,5): rows of 257 .. 4096 pairs are one
                                              item, finished by their block; rows of 4097 .. 9000 are two or three
                                              partial slots added by the finish pass
  k_cconv_mfma<true,4>, k_cconv_heavy4<32,true>
                                              test_whole_path_long_rows, cconv_valu = 0 (the cloud has rows of both classes)
  k_cconv<8,false> / <32,false> / <64,false>  test_general_kernels (the three groups of widths), 8 492 rows
  k_cconv_heavy<8,false>                      test_row_length_boundaries (3,8) (1,1); (4,8) with cconv_valu = 1
  k_cconv_heavy<32,false>                     test_row_length_boundaries (7,32); (4,32) with cconv_valu = 1
  k_cconv_heavy<64,false>                     test_row_length_boundaries (4,64) (7,33) (12,64)
    (cin == 4 feeds the VALU contraction from the matrix-core pair loop, every other cin from cconv_batch)
  k_cconv<8,true> + k_cconv_heavy<8,true>     test_whole_path_long_rows, channel_div 4, cconv_valu = 1
  k_cconv<32,true> + k_cconv_heavy<32,true>   test_whole_path_long_rows, channel_div 1, cconv_valu = 1
  k_cconv<64,true> + k_cconv_heavy<64,true>   test_aggregate_wide_first_stage (a 48- and a 64-wide first stage)
  k_cconv_absmax                              test_whole_path_long_rows_f16x2_valu
  basis output of k_cconv_mfma                test_basis_and_norm, test_filter_gradient_whole_tensor
"""
import functools

import numpy as np
import pytest
import torch

import parity
from asr_hip import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

BOUNDARY_LENS = [0, 9000, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 0, 4097]
N_INPUT = 10000


def _t(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@functools.lru_cache(maxsize=None)
def _short_lens():
    """8192 + 300 rows of 0 .. 20 pairs: more rows than the general kernel has waves; first and last row empty, a few more
    empty rows in between (besides the ones the draw gives)"""
    rng = np.random.default_rng(41)
    lens = rng.integers(0, 21, size=8192 + 300)
    lens[[0, -1]] = 0
    lens[[1, 63, 64, 100, 4095, 4096, 8191, 8192, 8193]] = 0
    return tuple(int(x) for x in lens)


@functools.lru_cache(maxsize=None)
def _geometry(lens, seed):
    """the ragged test's recipe: points in [-1, 1]^3, indices without replacement per row, outputs in [-0.3, 0.3]^3,
    extents in [1.5, 3], per-pair importance in [0.1, 1]"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    v = len(lens)
    pos = rng.uniform(-1, 1, size=(N_INPUT, 3)).astype(np.float32)
    out_pos = rng.uniform(-0.3, 0.3, size=(v, 3)).astype(np.float32)
    ext = rng.uniform(1.5, 3.0, size=v).astype(np.float32)
    rs = np.zeros(v + 1, np.int64)
    rs[1:] = np.cumsum(lens)
    idx = np.concatenate([rng.choice(N_INPUT, size=l, replace=False) for l in lens]).astype(np.int32)
    imp = rng.uniform(0.1, 1, size=rs[-1]).astype(np.float32)
    return dict(pos=pos, out_pos=out_pos, ext=ext, rs=rs, idx=idx, imp=imp, lens=lens)


@functools.lru_cache(maxsize=None)
def _weights(cin, cout):
    rng = np.random.default_rng(1000 * cin + cout)
    feat = rng.standard_normal((N_INPUT, cin)).astype(np.float32)
    W = (rng.standard_normal((4, 4, 4, cin, cout)) * 0.5).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    return feat, W, b


def _boundary():
    return _geometry(tuple(BOUNDARY_LENS), 7)


def _short():
    return _geometry(_short_lens(), 8)


@functools.lru_cache(maxsize=None)
def _reference(which, cin, cout, with_imp, normalize, precise=True):
    """the oracle's raw convolution (no bias, no activation); computed once per case and shared"""
    geo = _boundary() if which == "boundary" else _short()
    feat, W, _ = _weights(cin, cout)
    nimp = geo["imp"] if with_imp else None
    if precise:
        with O.precise():
            ref = O.continuous_conv(W, geo["out_pos"], geo["ext"], geo["pos"], feat, geo["idx"], nimp, geo["rs"], normalize)
    else:
        ref = O.continuous_conv(W, geo["out_pos"], geo["ext"], geo["pos"], feat, geo["idx"], nimp, geo["rs"], normalize)
    ref.setflags(write=False)
    return ref


def _run(gpu, geo, feat, W, nimp, normalize, bias, relu):
    from asr_hip import ops
    return ops.continuous_conv(_t(W, gpu), _t(geo["out_pos"], gpu), _t(geo["ext"], gpu), _t(geo["pos"], gpu),
                               _t(feat, gpu), _t(geo["idx"], gpu), _t(nimp, gpu) if nimp is not None else None,
                               _t(geo["rs"], gpu), normalize, bias=_t(bias, gpu) if bias is not None else None, relu=relu)


class _valu:
    """option cconv_valu of the shared context (or a pipeline's own), back to 0 afterwards"""

    def __init__(self, ctx, on):
        self.ctx, self.on = ctx, on

    def __enter__(self):
        if self.on:
            self.ctx.set_option("cconv_valu", 1)
        return self

    def __exit__(self, *exc):
        self.ctx.set_option("cconv_valu", 0)
        return False


def row_scaled_errors(got, ref):
    """|got - ref| / max(1, max|ref[row]|) per element: a 9000-pair row cannot lend its range to a 1-pair row"""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True)) if ref.shape[1] else np.ones((len(ref), 1))
    return np.abs(got - ref) / scale


def assert_close_rows(got, ref, tol=1e-5):
    """|got - ref| <= 1e-5 max(1, max|ref[row]|) for the un-normalised sums over up to 9000 pairs (|ref| reaches 265).
    What the bound rests on, measured on the CPU for BOUNDARY_LENS with and without importance: the fp32 oracle (sums in
    pair order) against the double-accumulating oracle misses the per-element 1e-5 + 1e-5 |ref| by up to 5.5 x, and
    reaches at most 0.16 of THIS bound for every (cin, cout) of test_row_length_boundaries with cout >= 5, and 0.12 of it
    for the 256-wide basis of test_basis_and_norm.  One pair dropped from the 9000-pair row moves it by 4e-3 of its
    range, 400 x the bound.
    cout == 1 is the exception: the row's range is then the one sum itself, which cancels (the fp32 oracle is at 0.88 of
    the bound with importance, 0.31 without): RANGE_BOUND_CASES take parity.assert_close_scaled instead, 1e-5 of the
    tensor's range, where the fp32 oracle stays below 0.04.  (The kernels sum in trees over lanes, waves and segments
    and measured at most 0.16 of the per-row bound in every family.)"""
    r = row_scaled_errors(got, ref)
    worst = float(r.max()) if r.size else 0.0
    assert worst <= tol, "worst row-scaled error %.3e in row %d" % (worst, int(np.argmax(r.max(axis=1))))


RANGE_BOUND_CASES = {(1, 1)}  # see assert_close_rows


# ---- 1. the general kernels ------------------------------------------------------------------------------------------
GENERAL_SHAPES = [(1, 1), (3, 8), (5, 3),          # k_cconv<8>
                  (3, 9), (8, 17), (7, 32),        # k_cconv<32>
                  (4, 33), (4, 64), (7, 33), (12, 64), (6, 48)]  # k_cconv<64>


@pytest.mark.parametrize("cin,cout", GENERAL_SHAPES)
def test_general_kernels(gpu, cin, cout):
    """k_cconv<8|32|64,false> on 8 492 short rows (the grid-stride loop runs a second time): one input chunk and several,
    a last chunk of 1, 2 and 3 channels, widths that leave output lanes idle and widths that fill them.  Per-element
    1e-5 + 1e-5 |ref| against the double-accumulating oracle (outputs are O(1): rows of at most 20 pairs, |ref| <= 24; the
    fp32 oracle itself is within 0.08 .. 0.80 of that bound over the eleven shapes, the widest input the worst); rows
    without pairs are act(bias) exactly."""
    geo = _short()
    feat, W, b = _weights(cin, cout)
    empty = geo["lens"] == 0
    assert empty[0] and empty[-1] and empty.sum() > 10 and len(empty) > 8192
    for with_imp, normalize, bias, relu in ((True, True, b, True), (False, True, b, True), (False, False, None, False)):
        out = _run(gpu, geo, feat, W, geo["imp"] if with_imp else None, normalize, bias, relu).cpu().numpy()
        ref = _reference("short", cin, cout, with_imp, normalize)
        if bias is not None:
            ref = np.maximum(ref.astype(np.float64) + bias, 0)
        parity.assert_close(out, ref)
        want_empty = np.maximum(bias, 0) if bias is not None else np.zeros(cout, np.float32)
        assert np.array_equal(out[empty], np.broadcast_to(want_empty, (int(empty.sum()), cout)))


# ---- 2. row-length boundaries, every family -------------------------------------------------------------------------
BOUNDARY_CASES = [(4, 32, 0), (4, 5, 0),                                          # k_cconv_mfma + heavy4 + finish
                  (4, 64, 0), (7, 33, 0), (12, 64, 0), (3, 8, 0), (1, 1, 0), (7, 32, 0),  # k_cconv + k_cconv_heavy
                  (4, 32, 1), (4, 8, 1)]                                          # the same with the matrix-core pair loop


@pytest.mark.parametrize("cin,cout,valu", BOUNDARY_CASES)
def test_row_length_boundaries(gpu, cin, cout, valu):
    """BOUNDARY_LENS: both sides of 64, 256 (light / long-row kernels), 1024 (one round of a 16-wave block), 4096 and 8192
    (one, two, three segments), an empty row in front of a long one, a long row last.
    Normalised + bias + relu: per-element 1e-5 + 1e-5 |ref|.  Un-normalised raw sums: assert_close_rows (see there for the
    measurement the bound rests on, and for the one width that takes the tensor-range form).
    The same call twice gives identical bits (the long-row list is filled by atomics in arbitrary order; the code
    promises one cut decision per launch and in-order segment sums), and on the matrix-core
    path a row's bits do not depend on its neighbours in the list (k_cconv_mfma: "a row's result does not depend on
    which rows share its chunk"): the list in reversed order gives the same rows."""
    from asr_hip import ops
    geo = _boundary()
    feat, W, b = _weights(cin, cout)
    lens = geo["lens"]
    assert lens[-1] > 4096 and lens[0] == 0 and lens[-2] == 0 and lens[1] > 8192
    with _valu(ops.context(gpu), valu):
        for with_imp, normalize, bias, relu in ((True, True, b, True), (False, False, None, False)):
            nimp = geo["imp"] if with_imp else None
            out_t = _run(gpu, geo, feat, W, nimp, normalize, bias, relu)
            out = out_t.cpu().numpy()
            ref = _reference("boundary", cin, cout, with_imp, normalize)
            if normalize:
                parity.assert_close(out, np.maximum(ref.astype(np.float64) + bias, 0))
            elif (cin, cout) in RANGE_BOUND_CASES:
                parity.assert_close_scaled(out, ref)
            else:
                assert_close_rows(out, ref)
            empty = lens == 0
            assert np.array_equal(out[empty], np.broadcast_to(np.maximum(bias, 0) if bias is not None else
                                                              np.zeros(cout, np.float32), (int(empty.sum()), cout)))
            again = _run(gpu, geo, feat, W, nimp, normalize, bias, relu)
            assert torch.equal(out_t, again), "two runs differ in rows %s" % (
                torch.nonzero((out_t != again).any(1)).flatten().tolist(),)
            if cin == 4 and cout <= 32 and not valu:
                rev = _reversed(geo)
                out_r = _run(gpu, rev, feat, W, rev["imp"] if with_imp else None, normalize, bias, relu)
                same = (out_r.flip(0) == out_t).all(1)
                assert bool(same.all()), "rows of %s pairs depend on their place in the list" % (
                    lens[(~same).cpu().numpy()].tolist(),)


def _reversed(geo):
    """the same rows in reversed list order: row_splits, indices, importance, positions and extents permuted together"""
    rs, v = geo["rs"], len(geo["lens"])
    order = np.arange(v)[::-1]
    pairs = np.concatenate([np.arange(rs[q], rs[q + 1]) for q in order]) if rs[-1] else np.zeros(0, np.int64)
    rs2 = np.zeros(v + 1, np.int64)
    rs2[1:] = np.cumsum(geo["lens"][order])
    return dict(pos=geo["pos"], out_pos=geo["out_pos"][order], ext=geo["ext"][order], rs=rs2, idx=geo["idx"][pairs],
                imp=geo["imp"][pairs], lens=geo["lens"][order])


# ---- 3. geometry edges of the coordinate map -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_rows():
    """rows of 0 .. 8 pairs, every pair with a point of its own.  Output positions and extents are dyadic where a
    neighbour has to sit EXACTLY on the ball's surface, so that (p - o) * (2 / extent) is +-1 without rounding."""
    s3 = 1.0 / np.sqrt(3.0)
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    diag = [(sx * s3, sy * s3, sz * s3) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    rows = []  # (output position, extent, offsets of the neighbours from the output position)
    rows.append(((0.25, -0.5, 0.75), 2.0, [(0, 0, 0)]))                                    # m < 1e-8: the centre cell mix
    rows.append(((0.0, 0.0, 0.0), 1000.0, [(1e-6, 0, 0), (0, -2e-6, 1e-6), (0, 0, 0)]))     # m < 1e-8 without coincidence
    rows.append(((0.25, -0.5, 0.75), 2.0, [tuple(1.0 * a for a in ax) for ax in axes]))     # ball surface -> cube face
    rows.append(((-0.125, 0.5, 0.25), 0.5, [tuple(0.25 * a for a in ax) for ax in axes]))
    rows.append(((0.25, -0.5, 0.75), 2.0, [tuple(1.5 * a for a in ax) for ax in axes]))     # 0.75 extent: outside, clamped
    rows.append(((0.25, -0.5, 0.75), 2.0, [tuple(1.0 * a for a in d) for d in diag]))       # diagonal at the surface -> corner
    rows.append(((0.1, 0.2, 0.3), 1e-3, [tuple(4e-4 * a for a in ax) for ax in axes]))      # tiny extent
    rows.append(((0.1, 0.2, 0.3), 1e-3, [tuple(4e-4 * a for a in d) for d in diag[:4]]))
    rows.append(((1.0, -2.0, 3.0), 1e3, [tuple(300.0 * a for a in ax) for ax in axes]))     # huge extent
    rows.append(((1.0, -2.0, 3.0), 1e3, [tuple(300.0 * a for a in d) for d in diag[4:]]))
    rows.append(((0.5, 0.5, 0.5), 4.0, []))                                                 # no neighbour
    rows.append(((0.25, -0.5, 0.75), 2.0, [(0, 0, 0), (1.0, 0, 0), (0, -1.0, 0), (0, 0, 1.5), diag[0], diag[7],
                                           (0.3, -0.2, 0.1), (-1.5, 1.5, 0)]))             # all of these in one row
    rows.append(((0.25, -0.5, 0.75), 2.0, [(-1.0, 0, 0)]))
    out_pos = np.array([r[0] for r in rows], np.float32)
    ext = np.array([r[1] for r in rows], np.float32)
    lens = np.array([len(r[2]) for r in rows], np.int64)
    pos = np.concatenate([out_pos[i].astype(np.float64) + np.array(r[2], np.float64).reshape(-1, 3)
                          for i, r in enumerate(rows)]).astype(np.float32)
    rs = np.zeros(len(rows) + 1, np.int64)
    rs[1:] = np.cumsum(lens)
    return dict(pos=pos, out_pos=out_pos, ext=ext, rs=rs, idx=np.arange(rs[-1], dtype=np.int32), lens=lens)


@pytest.mark.parametrize("cin,cout,valu", [(4, 16, 0), (4, 16, 1), (5, 40, 0)])
def test_geometry_edges(gpu, cin, cout, valu):
    """the ball -> cube -> grid map at its edges (cconv_pair_coords): a neighbour at the output position, neighbours on
    the ball's surface along the axes (cube faces, u = 0 or 3 exactly) and along the diagonals (cube corners), neighbours
    outside the ball (clamped), extents of 1e-3 and 1e3.  Unit importance and no normalisation: each output is a plain
    trilinear read of the filter, at most 8 of them summed; per-element 1e-5 + 1e-5 |ref|."""
    from asr_hip import ops
    geo = _edge_rows()
    assert 1 <= geo["lens"][geo["lens"] > 0].min() and geo["lens"].max() <= 8 and len(geo["lens"]) >= 12
    rng = np.random.default_rng(31 + cin)
    feat = rng.standard_normal((len(geo["pos"]), cin)).astype(np.float32)
    W = (rng.standard_normal((4, 4, 4, cin, cout)) * 0.5).astype(np.float32)
    with O.precise():
        ref = O.continuous_conv(W, geo["out_pos"], geo["ext"], geo["pos"], feat, geo["idx"], None, geo["rs"], False)
    assert np.abs(ref).max() > 0.5  # the rows do read the filter
    with _valu(ops.context(gpu), valu):
        out = _run(gpu, geo, feat, W, None, False, None, False).cpu().numpy()
    parity.assert_close(out, ref)


# ---- 4. basis output and the whole filter gradient ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _basis_reference(which, with_imp):
    """the oracle run with an identity filter, un-normalised: its output IS B[v][4 cell + c] (checked on the CPU for
    BOUNDARY_LENS: B @ W.reshape(256, 32) in float64 reproduces the oracle's convolution to 5.3e-6 on |ref| = 161)"""
    geo = _boundary() if which == "boundary" else _grad_rows()
    feat = _weights(4, 32)[0]
    eye = np.eye(256, dtype=np.float32).reshape(4, 4, 4, 4, 256)
    with O.precise():
        B = O.continuous_conv(eye, geo["out_pos"], geo["ext"], geo["pos"], feat, geo["idx"],
                              geo["imp"] if with_imp else None, geo["rs"], False)
    B.setflags(write=False)
    return B


def _row_sums(geo, with_imp):
    w = geo["imp"].astype(np.float64) if with_imp else np.ones(geo["rs"][-1])
    return np.array([w[geo["rs"][q]:geo["rs"][q + 1]].sum() for q in range(len(geo["lens"]))])


@pytest.mark.parametrize("with_imp", [True, False])
def test_basis_and_norm(gpu, with_imp):
    """asr_hip_continuous_conv_basis_f32 on BOUNDARY_LENS: k_cconv_mfma walks every row itself here (no long-row kernels),
    64 pairs per chunk up to 9000.  Basis against the identity-filter oracle with the per-row bound of
    assert_close_rows (the fp32 oracle is at 0.09 / 0.12 of it with / without importance), the importance sums against the
    float64 row sums with 1e-5 + 1e-5 |ref|."""
    from asr_hip import ops
    geo = _boundary()
    feat = _weights(4, 32)[0]
    basis, norm = ops.continuous_conv_basis(_t(geo["out_pos"], gpu), _t(geo["ext"], gpu), _t(geo["pos"], gpu), _t(feat, gpu),
                                            _t(geo["idx"], gpu), _t(geo["imp"], gpu) if with_imp else None, _t(geo["rs"], gpu))
    assert_close_rows(basis.cpu().numpy(), _basis_reference("boundary", with_imp))
    parity.assert_close(norm.cpu().numpy(), _row_sums(geo, with_imp))
    assert np.array_equal(basis.cpu().numpy()[geo["lens"] == 0], np.zeros((2, 256), np.float32))


@functools.lru_cache(maxsize=None)
def _grad_rows():
    lens = _short_lens()[4000:4300] + (257, 4097, 64)
    return _geometry(lens, 9)


@pytest.mark.parametrize("normalize", [True, False])
def test_filter_gradient_whole_tensor(gpu, normalize):
    """every element of W.grad of open3d::continuous_conv (basis kernel + one GEMM) against B_ref^T (g / norm) formed in
    float64 from the oracle's basis: 300 short rows (some empty) and rows of 257, 4097 and 64 pairs.
    |got - ref| <= 1e-5 max(1, max|ref|): each element is a sum over the 303 rows whose rounding is relative to the
    largest terms, and the 4097-pair row dominates the un-normalised gradient."""
    import open3d.ml.torch as ml3d
    geo = _grad_rows()
    assert (geo["lens"] == 0).any()
    feat = _weights(4, 32)[0]
    rng = np.random.default_rng(77)
    W = _t((rng.standard_normal((4, 4, 4, 4, 32)) * 0.3).astype(np.float32), gpu).requires_grad_(True)
    g = rng.standard_normal((len(geo["lens"]), 32)).astype(np.float32)
    out = ml3d.ops.continuous_conv(filters=W, out_positions=_t(geo["out_pos"], gpu), extents=_t(geo["ext"], gpu),
                                   offset=torch.zeros(3, device=gpu), inp_positions=_t(geo["pos"], gpu),
                                   inp_features=_t(feat, gpu), inp_importance=torch.empty((0,), device=gpu),
                                   neighbors_index=_t(geo["idx"], gpu), neighbors_importance=_t(geo["imp"], gpu),
                                   neighbors_row_splits=_t(geo["rs"], gpu), align_corners=True,
                                   coordinate_mapping="ball_to_cube_radial", normalize=normalize, interpolation="linear")
    (out * _t(g, gpu)).sum().backward()
    B = _basis_reference("grad", True).astype(np.float64)
    gg = g.astype(np.float64)
    if normalize:
        norm = _row_sums(geo, True)
        gg = gg / np.where(norm != 0, norm, 1.0)[:, None]
    ref = (B.T @ gg).reshape(4, 4, 4, 4, 32)
    parity.assert_close_scaled(W.grad.cpu().numpy(), ref)


# ---- 5. the whole path on a cloud that has long rows ---------------------------------------------------------------
def _make_clump_cloud():
    """a 6 k-point scan plus two clumps (9000 points around point 1234, 600 around point 4321) inside one search radius:
    the voxels around the hosts get aggregation rows of hundreds and of more than 8192 pairs, which no small scan
    cloud has (their longest row is 77 .. 153 pairs)"""
    p, q = synth.scan_cloud(6000, seed=11, device="cpu")
    pts, nrm = p.numpy(), q.numpy()
    rad = synth.knn_radii(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    rng = np.random.default_rng(5)
    for host, count in ((1234, 9000), (4321, 600)):
        extra = (pts[host] + rng.normal(0, 0.05 * rad[host], size=(count, 3))).astype(np.float32)
        pts = np.concatenate([pts, extra])
        nrm = np.concatenate([nrm, np.repeat(nrm[host:host + 1], count, 0)])
        rad = np.concatenate([rad, np.full(count, rad[host], np.float32)])
    pts, nrm, rad = (np.ascontiguousarray(a, np.float32) for a in (pts, nrm, rad))
    item = parity.oracle_geometry(pts, rad, *bb)
    return pts, nrm, rad, bb, item


@pytest.fixture(scope="module")
def clump_cloud():
    return _make_clump_cloud()


def _row_classes(rs):
    lens = np.diff(rs)
    return dict(mid=int(((lens > 256) & (lens <= 4096)).sum()), huge=int((lens > 8192).sum()), empty=int((lens == 0).sum()))


_clump_refs = {}


def _clump_reference(clump_cloud, channel_div):
    """seeded weights and the double-accumulating oracle's network on the clump cloud, computed once per width"""
    if channel_div not in _clump_refs:
        pts, nrm, rad, bb, item = clump_cloud
        weights = synth.make_weights(channel_div=channel_div, seed=11)
        with O.precise():
            _clump_refs[channel_div] = (weights, parity.oracle_network(item, pts, nrm, weights))
    return _clump_refs[channel_div]


def _forward(gpu, clump_cloud, weights, valu, precision="f32"):
    from asr_hip.pipeline import ImplicitPipeline
    pts, nrm, rad, bb, item = clump_cloud
    pipe = ImplicitPipeline(weights, device=gpu, precision=precision)
    with _valu(pipe.ctx, valu):
        values = pipe.forward(_t(pts, gpu), _t(nrm, gpu), _t(rad, gpu), bb[0], bb[1]).clone()
        torch.cuda.synchronize()
    return pipe, values


def _assert_clump_rows(clump_cloud, pipe=None):
    item = clump_cloud[4]
    cls = _row_classes(item["aggregation_row_splits"])
    assert cls["mid"] >= 1 and cls["huge"] >= 1 and cls["empty"] >= 1, cls  # or the test stops covering the long-row kernels
    if pipe is not None:
        assert np.array_equal(pipe.get("aggregation_row_splits").cpu().numpy(), item["aggregation_row_splits"])
        assert np.array_equal(pipe.get("aggregation_neighbors_index").cpu().numpy(), item["aggregation_neighbors_index"])


@pytest.mark.parametrize("valu", [0, 1])
@pytest.mark.parametrize("channel_div", [4, 1])
def test_whole_path_long_rows(gpu, clump_cloud, channel_div, valu):
    """first stage of the whole path (Morton records) on rows of 257 .. 4096 and of more than 8192 pairs, C0 = 8 and 32,
    matrix-core kernels and (cconv_valu = 1) the VALU ones: feats1 per element (the stage is normalised, |feats1| <= 3.4),
    values at the whole-path bound of 1e-5 of their range"""
    _assert_clump_rows(clump_cloud)
    weights, ref = _clump_reference(clump_cloud, channel_div)
    pipe, values = _forward(gpu, clump_cloud, weights, valu)
    _assert_clump_rows(clump_cloud, pipe)
    feats1 = pipe.get("feats1").cpu().numpy()
    assert feats1.shape == ref["feats1"].shape and feats1.shape[1] == 32 // channel_div
    parity.assert_close(feats1, ref["feats1"])
    parity.assert_close_scaled(values.cpu().numpy(), ref["values"])


def test_whole_path_long_rows_f16x2_valu(gpu, clump_cloud):
    """precision f16x2 scales the network's first sparse conv by the largest |feats1|; with cconv_valu = 1 that maximum
    comes from k_cconv_absmax (the matrix-core kernels keep it themselves).  A wrong maximum shows in the values."""
    _assert_clump_rows(clump_cloud)
    weights, ref = _clump_reference(clump_cloud, 4)
    pipe, values = _forward(gpu, clump_cloud, weights, 1, precision="f16x2")
    parity.assert_close(pipe.get("feats1").cpu().numpy(), ref["feats1"])
    parity.assert_close_scaled(values.cpu().numpy(), ref["values"])


def test_whole_path_layouts_agree(gpu, clump_cloud):
    """k_cconv_mfma / k_cconv_heavy4 promise identical bits for the Morton records of the whole path and the AoS arrays of
    the public operator: the stage recomputed through the operator on the pipeline's own lists equals feats1."""
    from asr_hip import ops
    pts, nrm, rad, bb, item = clump_cloud
    weights, ref = _clump_reference(clump_cloud, 4)
    pipe, _ = _forward(gpu, clump_cloud, weights, 0)
    _assert_clump_rows(clump_cloud, pipe)
    feats = _t(np.concatenate([nrm, np.ones((len(pts), 1), np.float32)], 1), gpu)
    again = ops.continuous_conv(_t(weights["cconv_block_in.conv1.kernel"], gpu), pipe.get("voxel_centers0"),
                                pipe.get("voxel_sizes0"), _t(pts, gpu), feats, pipe.get("aggregation_neighbors_index"),
                                pipe.get("importance"), pipe.get("aggregation_row_splits"), True,
                                _t(weights["cconv_block_in.conv1.bias"], gpu), relu=True)
    feats1 = pipe.get("feats1")
    same = (again == feats1).all(1)
    assert bool(same.all()), "rows of %s pairs differ between the layouts" % (
        np.diff(item["aggregation_row_splits"])[(~same).cpu().numpy()].tolist()[:20],)


@pytest.mark.parametrize("c0", [48, 64])
def test_aggregate_wide_first_stage(gpu, clump_cloud, c0):
    """a first stage wider than 32 channels takes k_cconv<64,true> + k_cconv_heavy<64,true> on the Morton records (no
    matrix-core kernel above 32): UNet5.aggregate alone, which needs the stage's two tensors only"""
    from asr_hip.pipeline import ImplicitPipeline
    pts, nrm, rad, bb, item = clump_cloud
    _assert_clump_rows(clump_cloud)
    rng = np.random.default_rng(c0)
    weights = {"cconv_block_in.conv1.kernel": (rng.standard_normal((4, 4, 4, 4, c0)) * 0.5).astype(np.float32),
               "cconv_block_in.conv1.bias": (rng.standard_normal(c0) * 0.1).astype(np.float32)}
    pipe = ImplicitPipeline(weights, device=gpu)
    pipe.build(_t(pts, gpu), _t(rad, gpu), bb[0], bb[1])
    feats1, imp = pipe.aggregate(_t(pts, gpu), _t(nrm, gpu), bb[0], bb[1])
    _assert_clump_rows(clump_cloud, pipe)
    imp_ref = (item["aggregation_scale_compat"] * O.window_poly6(item["aggregation_neighbors_dist"])).astype(np.float32)
    parity.assert_close(imp.cpu().numpy(), imp_ref, 1e-6)
    feats = np.concatenate([nrm, np.ones((len(pts), 1), np.float32)], 1)
    with O.precise():
        ref = O.continuous_conv(weights["cconv_block_in.conv1.kernel"], item["voxel_centers0"], item["voxel_sizes0"], pts,
                                feats, item["aggregation_neighbors_index"], imp_ref, item["aggregation_row_splits"], True)
    ref = np.maximum(ref.astype(np.float64) + weights["cconv_block_in.conv1.bias"], 0)
    parity.assert_close(feats1.cpu().numpy(), ref)


# ---- 6. argument errors (host-side checks, nothing is launched) ---------------------------------------------------
def test_argument_errors(gpu):
    from asr_hip import ops
    rng = np.random.default_rng(0)
    v, n = 5, 40
    pos = _t(rng.uniform(-1, 1, size=(n, 3)).astype(np.float32), gpu)
    out_pos = _t(rng.uniform(-0.3, 0.3, size=(v, 3)).astype(np.float32), gpu)
    ext = _t(np.full(v, 2.0, np.float32), gpu)
    rs = _t(np.arange(v + 1, dtype=np.int64) * 3, gpu)
    idx = _t(rng.integers(0, n, size=3 * v).astype(np.int32), gpu)

    def call(filter_shape, cin_feat, out_pos=out_pos, ext=ext, rs=rs, idx=idx):
        W = torch.zeros(filter_shape, device=gpu)
        feat = torch.zeros((n, cin_feat), device=gpu)
        return ops.continuous_conv(W, out_pos, ext, pos, feat, idx, None, rs, True)

    assert call((4, 4, 4, 4, 64), 4).shape == (v, 64)  # the widest filter is accepted
    with pytest.raises(RuntimeError, match="cout"):
        call((4, 4, 4, 4, 65), 4)
    with pytest.raises(RuntimeError):
        call((4, 4, 4, 4, 0), 4)
    with pytest.raises(RuntimeError, match="kernel_size"):
        call((3, 3, 3, 4, 8), 4)
    with pytest.raises(RuntimeError, match="kernel_size"):
        call((4, 4, 4, 8), 4)
    with pytest.raises(RuntimeError, match="feature width"):
        call((4, 4, 4, 4, 8), 5)
    # the context still works after the refused calls, and no output row means an empty result
    none = call((4, 4, 4, 4, 8), 4, out_pos=out_pos[:0], ext=ext[:0], rs=rs[:1], idx=idx[:0])
    assert none.shape == (0, 8)
    assert call((4, 4, 4, 4, 8), 4).shape == (v, 8)
