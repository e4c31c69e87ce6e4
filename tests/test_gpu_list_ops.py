"""The small operators between the convolutions, each alone and on lists an octree build never produces: row regrouping
(asr_geom_row_groups_batch: one list or the 13 of a build, ranked keys or full-mask keys, one sort or two),
invert_neighbors_list, reduce_subarrays_sum, decode_mlp (k_decode_mfma, the generic k_decode, the unaligned fallback),
asr_hip_absmax_f32 and asr_hip_convert_f16 -- against the plain NumPy restatements of tests/list_ops_ref.py, which
tests/test_list_ops.py pins on the CPU.  Integer results bit for bit; sums and the decoder within the bounds stated at
each test.  DESIGN.md ("The operators between the convolutions") lists the paths reached and not reached."""
import ctypes

import numpy as np
import pytest
import torch

import list_ops_ref as R
import parity
import sconv_lists as L
from asr_hip import synth

pytestmark = pytest.mark.gpu

i64 = ctypes.c_int64


def _t(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _np(t):
    return t.cpu().numpy()


# ---- A. row regrouping -----------------------------------------------------------------------------------------------
def _check_order(perm, lst, seg, lpt, drop_slot0, what):
    v = len(lst.rs) - 1
    assert perm.dtype == np.int32 and R.is_permutation(perm, v), what                # (b)
    if seg % 128 == 0:
        assert R.keeps_segments(perm, seg), what                                     # (c)
    want = R.row_groups_ref(lst.slots, lst.rs, seg, lpt, drop_slot0)
    assert np.array_equal(perm, want), (what, int(np.argmax(perm != want)))          # (a)


@pytest.mark.parametrize("lpt", [1, 0])
@pytest.mark.parametrize("v", R.ROW_GROUP_ROWS)
def test_row_groups_of_one_list_follow_the_documented_order(gpu, v, lpt):
    """asr_hip_row_groups on synthetic lists: bit-equal to the restated order (segment, slot mask, row; then the chunks
    of a segment heaviest first), a permutation, and every row inside its own segment.  A batch of one list with full-mask
    keys: one sort while segment field + 56 mask bits fit 64 bits (up to v = 3001 at 16-row segments, exactly 64), a sort
    by mask and one by segment beyond (v = 4200 at 16-row segments)"""
    from asr_hip import ops
    ctx = ops.context(gpu)
    lists = R.row_group_lists(v) + (R.fixed_row_group_lists() if v == 200 else ())
    ctx.set_option("row_lpt", lpt)
    try:
        for lst in lists:
            kidx, rs = _t(lst.slots, gpu), _t(lst.rs, gpu)
            for segment_rows in R.SEGMENT_ROWS:
                perm = _np(ops.row_groups(kidx, rs, segment_rows))
                _check_order(perm, lst, segment_rows or R.DEFAULT_SEGMENT, bool(lpt), False,
                             (lst.name, segment_rows, lpt))
    finally:
        ctx.set_option("row_lpt", 1)


@pytest.fixture(scope="module")
def build_cloud(gpu):
    from asr_hip.pipeline import ImplicitPipeline
    p, q = synth.scan_cloud(40000, seed=12, device=gpu)
    rad = synth.knn_radii_gpu(p, 24)
    bb = synth.bounding_box(p, 0.1)
    return ImplicitPipeline(synth.make_weights(4, seed=1), device=gpu), p, rad, bb


TILINGS = [("tiling%d" % i, "neighbors", i) for i in range(5)] + \
          [(t % i, pre, i) for i in range(4) for t, pre in (("tiling_up%d", "up_neighbors"), ("tiling_down%d", "down_neighbors"))]


@pytest.mark.parametrize("seg", [524288, 4096, 128])
@pytest.mark.parametrize("lpt", [1, 0])
@pytest.mark.parametrize("ranked", [1, 0])
def test_tilings_of_a_build_follow_the_documented_order(gpu, build_cloud, ranked, lpt, seg):
    """the 13 tilings of implicit_build under every (row_ranked, row_lpt, row_segment): the ranked-key sort and the
    full-mask-key sorts give the restated order, at 128-row segments too: the batch has no fallback to another routine, so
    with row_ranked = 1 the ranked keys serve that build as well, with a segment field of more than 6 bits"""
    pipe, p, rad, bb = build_cloud
    assert len(TILINGS) == 13
    try:
        for k, val in (("row_ranked", ranked), ("row_lpt", lpt), ("row_segment", seg)):
            pipe.ctx.set_option(k, val)
        pipe.build(p, rad, bb[0], bb[1])
        rows = {}
        for tname, pre, i in TILINGS:
            perm = _np(pipe.get(tname))
            lst = L.SconvList(tname, None, _np(pipe.get("%s_kernel_index%d" % (pre, i))),
                              _np(pipe.get("%s_row_splits%d" % (pre, i))), 0, 0)
            rows[tname] = len(lst.rs) - 1
            _check_order(perm, lst, seg, bool(lpt), True, (tname, ranked, lpt, seg))
            # on the lists of a build the order by the whole mask and the order without slot 0 coincide (which is why the
            # batched build and the per-list routine agree on them)
            assert np.array_equal(perm, R.row_groups_ref(lst.slots, lst.rs, seg, bool(lpt), False)), tname
    finally:
        for k, val in (("row_ranked", 1), ("row_lpt", 1), ("row_segment", 524288)):
            pipe.ctx.set_option(k, val)
    if seg == 128:
        assert rows["tiling0"] >= 63 * 128, rows  # rows // seg >= 63: a segment field wider than 6 bits was used
    else:
        assert all(v // seg < 63 for v in rows.values()), rows  # the segments fit the 6 bits the field once had: narrow fields


# ---- B. invert_neighbors_list ----------------------------------------------------------------------------------------
def _facade():
    import open3d.ml.torch  # noqa: F401  (registers torch.ops.open3d)
    return torch.ops.open3d


@pytest.mark.parametrize("case", R.invert_lists(), ids=lambda c: "%s-%d" % (c[0].name, c[1]))
def test_invert_neighbors_list_bit_exact(gpu, case):
    """empty rows at the start, in runs and at the end, no pair, no row, inputs nobody names, one input named by 5000
    pairs, rows of 3000 and more entries, a pair stored twice, num_points = 1; with uint8 attributes over 0..255 and
    without; through asr_hip.ops and through torch.ops.open3d; and twice, which sorts every row by input"""
    from asr_hip import ops
    lst, num_points = case
    idx, rs, attr = _t(lst.idx, gpu), _t(lst.rs, gpu), _t(lst.slots, gpu)
    ri, rr, ra = R.invert_ref(num_points, lst.idx, lst.rs, lst.slots)
    none = torch.empty(0, dtype=torch.uint8, device=gpu)
    calls = (("ops", lambda a: ops.invert_neighbors_list(num_points, idx, rs, a), None),
             ("open3d", lambda a: _facade().invert_neighbors_list(num_points, idx, rs, a), none))
    for name, call, no_attr in calls:
        gi, gr, ga = call(attr)
        assert gi.dtype == torch.int32 and gr.dtype == torch.int64 and ga.dtype == torch.uint8, name
        assert np.array_equal(_np(gi), ri) and np.array_equal(_np(gr), rr) and np.array_equal(_np(ga), ra), name
        hi, hr, ha = call(no_attr)
        assert np.array_equal(_np(hi), ri) and np.array_equal(_np(hr), rr) and ha.numel() == 0, name
        # the round trip
        bi, br, ba = ops.invert_neighbors_list(len(lst.rs) - 1, gi, gr, ga)
        si, sr, sa = R.rows_sorted_by_input(lst)
        assert np.array_equal(_np(bi), si) and np.array_equal(_np(br), sr) and np.array_equal(_np(ba), sa), name


# ---- C. reduce_subarrays_sum -----------------------------------------------------------------------------------------
def test_reduce_subarrays_sum_rows_of_0_to_20000_entries(gpu):
    """non-negative values within 1e-5 + 1e-5 |ref| of the float64 sum; signed values within n 2^-24 sum|x|, the bound
    of any sequential f32 sum (a relative tolerance means nothing next to a sum near 0); empty rows exactly 0"""
    from asr_hip import ops
    rs = R.reduce_row_splits()
    empty = np.diff(rs) == 0
    rng = np.random.default_rng(41)
    x = rng.uniform(0, 1, size=int(rs[-1])).astype(np.float32)
    ref, _ = R.reduce_ref(x, rs)
    for got in (ops.reduce_subarrays_sum(_t(x, gpu), _t(rs, gpu)), _facade().reduce_subarrays_sum(_t(x, gpu), _t(rs, gpu))):
        assert got.dtype == torch.float32
        print("reduce, uniform(0, 1): err / limit = %.3g" % R.err_over_limit(_np(got), ref))
        parity.assert_close(_np(got), ref)
        assert np.all(_np(got)[empty] == 0) and not np.signbit(_np(got)[empty]).any()
    x = rng.standard_normal(int(rs[-1])).astype(np.float32)
    ref, mags = R.reduce_ref(x, rs)
    got = _np(ops.reduce_subarrays_sum(_t(x, gpu), _t(rs, gpu)))
    bound = R.sequential_sum_bound(rs, mags)
    print("reduce, normal: |err| / bound = %s" % np.array2string(np.abs(got - ref)[~empty] / bound[~empty], precision=3))
    assert np.all(np.abs(got - ref) <= bound)
    assert np.all(got[empty] == 0)


def test_reduce_subarrays_sum_with_a_gather_index(gpu):
    from asr_hip import ops
    rs = R.reduce_row_splits()
    rng = np.random.default_rng(42)
    n = 100
    g = rng.integers(0, n, size=int(rs[-1])).astype(np.int32)  # repeated indices
    g[0], g[-1], g[int(rs[4])] = n - 1, n - 1, n - 1         # ... and the last value, first, last and inside
    for x in (rng.uniform(0, 1, size=n).astype(np.float32), rng.standard_normal(n).astype(np.float32)):
        ref, mags = R.reduce_ref(x, rs, g)
        got = _np(ops.reduce_subarrays_sum(_t(x, gpu), _t(rs, gpu), _t(g, gpu)))
        if x.min() >= 0:
            parity.assert_close(got, ref)
        assert np.all(np.abs(got - ref) <= R.sequential_sum_bound(rs, mags))
        assert np.array_equal(got, _np(ops.reduce_subarrays_sum(_t(x[g], gpu), _t(rs, gpu))))  # the same sum, same order


def test_reduce_subarrays_sum_without_rows_without_values_and_backward(gpu):
    from asr_hip import ops
    rs0 = torch.zeros(1, dtype=torch.int64, device=gpu)
    x0 = torch.empty(0, dtype=torch.float32, device=gpu)
    for f in (ops.reduce_subarrays_sum, _facade().reduce_subarrays_sum):
        out = f(x0, rs0)
        assert out.shape == (0,) and out.dtype == torch.float32
        out = f(x0, torch.zeros(8, dtype=torch.int64, device=gpu))  # seven empty rows
        assert out.shape == (7,) and not out.any()
    # backward on a list with empty rows: grad repeated by row length, exactly
    rs = R.reduce_row_splits((0, 3, 0, 0, 1, 700, 0))
    rng = np.random.default_rng(43)
    x = _t(rng.standard_normal(int(rs[-1])).astype(np.float32), gpu).requires_grad_(True)
    grad = rng.standard_normal(len(rs) - 1).astype(np.float32)
    _facade().reduce_subarrays_sum(x, _t(rs, gpu)).backward(_t(grad, gpu))
    assert np.array_equal(_np(x.grad), np.repeat(grad, np.diff(rs)))


# ---- D. decode_mlp ---------------------------------------------------------------------------------------------------
def _decode(ops, d, gpu, with_sizes, code=None):
    args = [_t(d[k], gpu) for k in ("w1", "b1", "w2", "b2", "w3")]
    code = _t(d["code"], gpu) if code is None else code
    return _np(ops.decode_mlp(code, *args, voxel_sizes=_t(d["sizes"], gpu) if with_sizes else None))


def _decode_ref(d, with_sizes):
    return R.decode_ref(*[d[k] for k in ("code", "w1", "b1", "w2", "b2", "w3")], d["sizes"] if with_sizes else None)


def _decode_case(ops, gpu, v, widths):
    """-> worst err / limit over with and without voxel_sizes, after asserting the tolerance"""
    d = R.decode_data(v, *widths)
    worst = 0.0
    for with_sizes in (False, True):
        got, ref = _decode(ops, d, gpu, with_sizes), _decode_ref(d, with_sizes)
        worst = max(worst, R.err_over_limit(got, ref))
        parity.assert_close(got, ref)
    return worst


@pytest.mark.parametrize("widths", R.DECODE_WIDTHS)
def test_decode_mlp_widths(gpu, widths):
    """(32, 32, 32) on the matrix cores, every other trio through the generic kernel; 1000 rows with a row of zeros (the
    bias path alone), with and without voxel_sizes, against the float64 restatement within 1e-5 + 1e-5 |ref|"""
    from asr_hip import ops
    print("decode %s: worst err / limit = %.3g" % (widths, _decode_case(ops, gpu, 1000, widths)))


@pytest.mark.parametrize("widths", R.DECODE_ROWS_WIDTHS)
@pytest.mark.parametrize("v", R.DECODE_ROWS)
def test_decode_mlp_row_counts(gpu, v, widths):
    """rows around the 16-row groups of a wave and the 64 rows of a block, for both kernels"""
    from asr_hip import ops
    print("decode %s, v = %d: worst err / limit = %.3g" % (widths, v, _decode_case(ops, gpu, v, widths)))


def test_decode_mlp_second_pass_of_the_matrix_core_kernel(gpu):
    """2048 blocks x 4 waves x 16 rows + 21: the first waves loop a second time, the others prefetch past the last group"""
    from asr_hip import ops
    v = R.DECODE_SECOND_PASS_ROWS
    assert v > 2048 * 4 * 16 and v % 16
    print("decode (32, 32, 32), v = %d: worst err / limit = %.3g" % (v, _decode_case(ops, gpu, v, (32, 32, 32))))


def test_decode_mlp_code_that_is_not_16_byte_aligned(gpu):
    """a contiguous (32, 32, 32) code that starts 4 bytes into a buffer cannot be read with 16-byte loads: the launcher
    takes the generic kernel for it; same tolerance, and the same values as the aligned call within that tolerance"""
    from asr_hip import ops
    for v in (65, 1000):
        d = R.decode_data(v, 32, 32, 32)
        buf = torch.zeros(v * 32 + 1, dtype=torch.float32, device=gpu)
        buf[1:] = _t(d["code"], gpu).reshape(-1)
        code = buf[1:].view(v, 32)
        assert code.is_contiguous() and code.data_ptr() % 16 == 4
        for with_sizes in (False, True):
            got, ref = _decode(ops, d, gpu, with_sizes, code=code), _decode_ref(d, with_sizes)
            parity.assert_close(got, ref)
            parity.assert_close(got, _decode(ops, d, gpu, with_sizes))
        assert code.data_ptr() % 16 == 4  # (the wrapper did not copy it to an aligned place either)


@pytest.mark.parametrize("bad", [65, 0])
def test_decode_mlp_refusals(gpu, bad):
    from asr_hip import ops
    from asr_hip._lib import AsrHipError
    for pos in range(3):
        widths = [8, 8, 8]
        widths[pos] = bad
        d = R.decode_data(4, *widths)
        with pytest.raises(AsrHipError, match="layer widths must be 1..64"):
            _decode(ops, d, gpu, False)
    d = R.decode_data(0, 32, 32, 32)
    for with_sizes in (False, True):
        assert _decode(ops, d, gpu, with_sizes).shape == (0, 2)


# ---- E. absmax and convert_f16 ---------------------------------------------------------------------------------------
def _absmax_raw(gpu, buf, rows, cols, ld, preload=0):
    """asr_hip_absmax_f32 on the first rows x cols elements of a buffer with row stride ld -> the int32 it wrote"""
    from asr_hip import ops
    from asr_hip._lib import ptr
    out = torch.full((1,), preload, dtype=torch.int32, device=gpu)
    ops.context(gpu).call("asr_hip_absmax_f32", ptr(buf), i64(rows), ctypes.c_int(cols), i64(ld), ptr(out))
    return int(out.item())


def _bits(x):
    return int(np.abs(np.asarray(x, np.float32)).max().view(np.int32)) if np.size(x) else 0


def test_absmax_f32_edges(gpu):
    """bit-exact np.abs(x).max(): padding columns ignored, a negative maximum, the last element of a matrix the grid
    walks twice, denormals, zeros of both signs, +inf, no rows; and the call overwrites what `out` held"""
    from asr_hip import ops
    rng = np.random.default_rng(51)
    big = 0x7f000000  # a preloaded value larger than every finite maximum below: the call must not accumulate
    # row stride larger than the width: 1e30 in the padding
    x = rng.standard_normal((37, 24)).astype(np.float32)
    x[:, 19:] = 1e30
    assert _absmax_raw(gpu, _t(x, gpu), 37, 19, 24, preload=big) == _bits(x[:, :19]) < _bits(x)
    # the largest magnitude is negative
    x = rng.uniform(-1, 1, size=(50, 7)).astype(np.float32)
    x[23, 5] = -3.25
    assert int(ops.absmax(_t(x, gpu)).item()) == _bits(x) == _bits(3.25)
    assert _absmax_raw(gpu, _t(x, gpu), 50, 7, 7, preload=big) == _bits(3.25)
    # 8192 blocks x 256 threads + 3 elements: the maximum sits in the last one
    n = 8192 * 256 + 3
    assert n % 5 == 0
    x = rng.uniform(-1, 1, size=(n // 5, 5)).astype(np.float32)
    x[-1, -1] = 1.5
    assert int(ops.absmax(_t(x, gpu)).item()) == _bits(1.5)
    x[-1, -1] = 0.25
    assert int(ops.absmax(_t(x, gpu)).item()) == _bits(x)
    # denormals only; zeros of both signs; +inf
    x = (rng.integers(1, 1 << 23, size=(9, 33)).astype(np.int32) | (rng.integers(0, 2, size=(9, 33)).astype(np.int32) << 31))
    x = x.astype(np.int32).view(np.float32)
    assert 0 < _bits(x) < (1 << 23) and _absmax_raw(gpu, _t(x, gpu), 9, 33, 33, preload=big) == _bits(x)
    z = np.zeros((4, 6), np.float32)
    z[1::2] = -0.0
    assert _absmax_raw(gpu, _t(z, gpu), 4, 6, 6, preload=big) == 0
    x = rng.standard_normal((5, 5)).astype(np.float32)
    x[2, 2] = np.inf
    assert _absmax_raw(gpu, _t(x, gpu), 5, 5, 5) == 0x7f800000
    # no rows: the maximum of nothing is 0, whatever `out` held
    assert _absmax_raw(gpu, _t(np.ones((3, 3), np.float32), gpu), 0, 3, 3, preload=big) == 0
    # ops.absmax(out=...) overwrites too
    out = torch.full((1,), big, dtype=torch.int32, device=gpu)
    assert int(ops.absmax(_t(np.full((2, 2), 0.5, np.float32), gpu), out=out).item()) == _bits(0.5)


def _convert(gpu, x, to_f16):
    from asr_hip import ops
    from asr_hip._lib import ptr
    n = len(x)
    src = _t(x, gpu)
    out = torch.full((n + 8,), -1, dtype=torch.int16 if to_f16 else torch.int32, device=gpu)  # 8 guard elements
    ops.context(gpu).call("asr_hip_convert_f16", ptr(src) if n else ctypes.c_void_p(0), i64(n), ptr(out), int(to_f16))
    got = _np(out)
    assert np.all(got[n:] == -1), "wrote past n"
    return got[:n].view(np.uint16 if to_f16 else np.float32)


def test_convert_f16_both_ways_bit_exact(gpu):
    """f32 -> f16 is numpy's round to nearest even on every f16 value, every midpoint, the overflow threshold and the
    denormal edge, NaN stays NaN; f16 -> f32 is exact on all 65536 bit patterns; n around the block size, and n = 0"""
    x = R.f16_probe()
    want = R.f16_bits_ref(x)
    got = _convert(gpu, x, True)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan]), np.flatnonzero(got != want)[:8]
    assert np.isnan(got[nan].view(np.float16)).all()
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    back = _convert(gpu, h.view(np.int16), False)
    ref = h.view(np.float16).astype(np.float32)
    nan = np.isnan(ref)
    assert np.array_equal(back[~nan].view(np.uint32), ref[~nan].view(np.uint32)) and np.isnan(back[nan]).all()
    shuffled = np.random.default_rng(52).permutation(x[~np.isnan(x)])
    for n in (1, 255, 256, 257, 100003, 0):
        assert np.array_equal(_convert(gpu, shuffled[:n], True), R.f16_bits_ref(shuffled[:n])), n
        hs = R.f16_bits_ref(shuffled[:n])
        assert np.array_equal(_convert(gpu, hs.view(np.int16), False).view(np.uint32),
                              hs.view(np.float16).astype(np.float32).view(np.uint32)), n


# ---- F. attributes and sums keep their dtype -------------------------------------------------------------------------
ATTRIBUTES = {
    "float32": lambda p: (np.arange(p) + 0.37).astype(np.float32),
    "int32": lambda p: (np.arange(p) * 70000 // max(p - 1, 1)).astype(np.int32),
    "int64": lambda p: (2 ** 31 + 5 + 3 * np.arange(p)).astype(np.int64),
    "float64": lambda p: np.arange(p) + 2.0 ** -30,
}


@pytest.mark.parametrize("dtype", sorted(ATTRIBUTES))
def test_inverted_attributes_come_back_exactly_in_their_own_dtype(gpu, dtype):
    """open3d::invert_neighbors_list carries attributes of any type: a float32 0.37 must not come back as 0.0 nor an
    int32 300 as 44 (a pass through uint8); through asr_hip.ops and through torch.ops.open3d"""
    from asr_hip import ops
    for lst in (R.from_sconv(L.tile_edges(129)), R.long_rows(), R.stored_twice()):
        attr = ATTRIBUTES[dtype](len(lst.idx))
        assert attr.dtype == np.dtype(dtype) and not np.array_equal(attr, attr.astype(np.uint8))
        ri, rr, ra = R.invert_ref(lst.num_inp, lst.idx, lst.rs, attr)
        for f in (ops.invert_neighbors_list, _facade().invert_neighbors_list):
            gi, gr, ga = f(lst.num_inp, _t(lst.idx, gpu), _t(lst.rs, gpu), _t(attr, gpu))
            assert _np(ga).dtype == np.dtype(dtype) and np.array_equal(_np(ga), ra), (lst.name, f)
            assert np.array_equal(_np(gi), ri) and np.array_equal(_np(gr), rr)


def test_sums_keep_the_dtype_of_the_values(gpu):
    """float64 and integer values are summed in their own type (never in float32 and cast back); what is not supported
    is refused"""
    from asr_hip import ops
    from asr_hip._lib import AsrHipError
    rs = R.reduce_row_splits((0, 1, 55, 1000, 0, 5000))
    n = int(rs[-1])
    # 1 + k 2^-30, k < 2^13: every partial sum is exact in float64, in any order, and no sum is a float32
    x = 1.0 + np.arange(1, n + 1) * 2.0 ** -30
    rows = lambda a: np.array([a[rs[q]:rs[q + 1]].sum() for q in range(len(rs) - 1)], a.dtype)  # noqa: E731
    ref = rows(x)
    assert np.all(ref[ref != 0] != ref[ref != 0].astype(np.float32))
    g = np.random.default_rng(61).integers(0, n, size=n).astype(np.int32)
    g[-1] = n - 1
    for f in (ops.reduce_subarrays_sum, _facade().reduce_subarrays_sum):
        got = f(_t(x, gpu), _t(rs, gpu))
        assert got.dtype == torch.float64 and np.array_equal(_np(got), ref), f
        for dt, hi in ((np.int32, 70000), (np.int64, 2 ** 40)):
            k = np.random.default_rng(62).integers(-hi, hi, size=n).astype(dt)
            got = f(_t(k, gpu), _t(rs, gpu))
            assert _np(got).dtype == dt and np.array_equal(_np(got), rows(k)), (f, dt)
    got = ops.reduce_subarrays_sum(_t(x, gpu), _t(rs, gpu), _t(g, gpu))
    assert got.dtype == torch.float64 and np.array_equal(_np(got), R.reduce_ref(x, rs, g)[0])
    with pytest.raises(AsrHipError, match="float32, float64, int32 or int64"):
        ops.reduce_subarrays_sum(_t(x, gpu).half(), _t(rs, gpu))
