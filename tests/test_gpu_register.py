"""GPU tests of the rigid registration (asr_hip_icp_step, asr_hip_register_points and the layers above them) against the
numpy restatement of the contract in tests/register_ref.py: the pairs exactly, the sums within the f64 summation bound,
the same bits on every run, the driver against the restatement's driver on motions with a known answer.

The shared inputs (a 20 000-point target on a surface without symmetries, 5 000 of its points moved by the inverse of a
known motion) and every reference result are computed once per module."""
import ctypes
import json

import numpy as np
import pytest
import torch

import crowded_inputs as CI
import register_ref as R
from asr_hip import _lib, ops
from asr_hip._lib import AsrHipError
from stream_helpers import late

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CAP = 0.3
MOTIONS = ((5, 0.05), (10, 0.1), (20, 0.2))
# Partial overlap: with the cap of the other tests, a seventh of the surface's side, the source points in a band that wide
# beyond the target's edge pair with the points of the edge, and that set changes from step to step: the restatement does
# not settle in 50 steps.  A cap of 0.1 leaves a band too narrow for that (the restatement converges in 5 steps).
PARTIAL_CAP = 0.1


def margin_frame(points):
    return _lib.frame_init(*CI.margin_box(np.asarray(points, np.float32)))


def dev(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.fixture(scope="module")
def cases():
    return {m: R.moved_pair(*m) for m in MOTIONS}


@pytest.fixture(scope="module")
def partial():
    """target over [-1, 1]^2, source over [0, 2] x [-1, 1], moved by the inverse of the 5 degree motion"""
    target, normals = R.surface(20000, 7)
    placed, _ = R.surface(5000, 9, (0.0, 2.0))
    return target, normals, placed, R.transform_f32(R.inverse(R.motion(5, 0.05)), placed)


def sqdist_f32(q, points):
    """the contract's f32 squared distance of one query to every point"""
    d = np.asarray(points, np.float32) - np.asarray(q, np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def check_step(gpu, target, normals, source, transform, cap, frame=None, origin=None, what="", sums=True):
    """icp_step against the restatement: index and pair count exactly, every sum within (pairs + 8) 2^-52 sum|term|"""
    frame = frame or margin_frame(target)
    origin = R.frame_origin(frame) if origin is None else np.asarray(origin, np.float64)
    got, index = ops.icp_step(frame, dev(gpu, target), dev(gpu, normals), dev(gpu, source), transform, origin, cap,
                              return_index=True)
    want, scale, ref_index = R.step(target, normals, source, transform, origin, cap)
    index = index.cpu().numpy()
    assert index.dtype == np.int32 and index.shape == (len(source),)
    bad = np.flatnonzero(index != ref_index)
    print("%s: n=%d m=%d pairs=%d (reference %d), %d rows differ%s"
          % (what, len(target), len(source), got["pairs"], want["pairs"], len(bad),
             "" if not len(bad) else " (first: row %d, got %d, want %d)" % (bad[0], index[bad[0]], ref_index[bad[0]])))
    assert np.array_equal(index, ref_index), what
    assert got["pairs"] == want["pairs"] == int((ref_index >= 0).sum()), what
    assert got["mode"] == int(normals is not None)
    if sums:
        factor = (want["pairs"] + 8) * EPS
        worst = 0.0
        for key in ("ata", "atb", "sq_residual", "sq_distance"):
            g, w, s = (np.atleast_1d(np.asarray(x[key], np.float64)) for x in (got, want, scale))
            assert g.shape == w.shape
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.nanmax(np.where(s > 0, np.abs(g - w) / (factor * s), 0.0))))
            assert np.all(np.abs(g - w) <= factor * s), (what, key, g, w, s)
        print("%s: largest |sum - reference| / bound = %.3g" % (what, worst))
    return got, index


# ---- 1. pairs, exactly; sums within the summation bound -----------------------------------------------------------------
@pytest.mark.parametrize("plane", (True, False), ids=("plane", "point"))
def test_surface_at_identity_and_at_the_small_motion(gpu, cases, plane):
    target, normals, source, _ = cases[MOTIONS[0]]
    for name, t in (("identity", R.identity()), ("5 degrees", R.motion(*MOTIONS[0]))):
        got, index = check_step(gpu, target, normals if plane else None, source, t, CAP, what="surface, " + name)
        if name == "5 degrees":  # the source is back on its own points
            assert got["pairs"] == len(source) and got["sq_distance"] < len(source) * 1e-12
        if not plane:
            assert got["sq_residual"] == got["sq_distance"]


@pytest.mark.parametrize("plane", (True, False), ids=("plane", "point"))
def test_sums_with_a_large_origin_offset(gpu, cases, plane):
    """the cloud shifted by 1000, the origin at its centre: the terms are as small as without the shift"""
    target, normals, source, _ = cases[MOTIONS[0]]
    shift = np.float32(1000.0)
    t = R.motion(2, 0.01)
    t[:, 3] += 1000.0 - t[:, :3] @ np.full(3, 1000.0)
    frame = margin_frame(target + shift)
    assert np.abs(R.frame_origin(frame) - 1000.0).max() < 0.01
    got, _ = check_step(gpu, target + shift, normals if plane else None, source + shift, t, CAP, frame, what="shifted by 1000")
    near, _ = check_step(gpu, target, normals if plane else None, source, R.motion(2, 0.01), CAP, what="not shifted")
    assert got["pairs"] == near["pairs"] == len(source)
    assert 0.5 < got["ata"][0] / near["ata"][0] < 2.0  # (an origin at 0 would give 10^6 times as much)


def test_lattice_ties_and_duplicates(gpu):
    """9^3 lattice in a shuffled order with queries on the points, the face centres (4-way ties) and the cell centres
    (8-way ties); then a cloud whose first 50 points are copies of the next 50"""
    g = np.arange(9, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts = np.ascontiguousarray(pts[np.random.default_rng(0).permutation(len(pts))])
    h = g[:-1] + np.float32(0.5)
    cells = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3)
    faces = np.concatenate([np.stack(np.meshgrid(*[g if a == ax else h for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
                            for ax in range(3)])
    queries = np.concatenate([pts, faces, cells]).astype(np.float32)
    up = np.tile(np.float32([0.6, 0.0, 0.8]), (len(pts), 1))
    for cap in (1.0, 0.75, np.sqrt(np.float32(0.75))):  # 0.75^2 < 0.75: the cell centres are out; sqrt(0.75): on the cap
        got, index = check_step(gpu, pts, up, queries, R.identity(), cap, what="lattice, cap %g" % cap)
        assert np.all(index[:len(pts) + len(faces)] >= 0)
    target, _ = R.surface(3000, 3)
    target[:50] = target[50:100]
    _, index = check_step(gpu, target, None, target.copy(), R.identity(), 0.05, what="duplicates")
    assert np.array_equal(index[:100], np.concatenate([np.arange(50), np.arange(50)]))


def test_one_target_point_and_queries_outside_the_frame(gpu, cases):
    one = np.float32([[0.25, -0.5, 0.125]])
    rng = np.random.default_rng(4)
    queries = np.concatenate([one + rng.normal(size=(300, 3)) * 0.2, one]).astype(np.float32)
    _, index = check_step(gpu, one, np.float32([[0, 0, 1]]), queries, R.identity(), 0.25, what="n = 1")
    assert index[-1] == 0 and (index == -1).any() and (index == 0).sum() > 10
    target, normals, source, _ = cases[MOTIONS[0]]
    lo, hi = target.min(0), target.max(0)
    outside = np.concatenate([rng.uniform(lo - 0.2, hi + 0.2, (2000, 3)),          # around the frame, many within the cap
                              rng.uniform(lo - 50, hi + 50, (500, 3)),             # far outside
                              [[1e30, 0, 0], [0, -3e38, 0], [1e-30, 1e-40, 0]]]).astype(np.float32)
    _, index = check_step(gpu, target, normals, outside, R.identity(), CAP, what="outside the frame")
    assert (index[:2000] >= 0).any() and (index[:2000] == -1).any() and np.all(index[-3:-1] == -1)


def test_nan_and_inf_source_points_take_no_part(gpu, cases):
    target, normals, source, _ = cases[MOTIONS[0]]
    source = source[:700].copy()
    source[3, 1] = np.nan
    source[64] = np.inf
    source[699, 2] = -np.inf
    got, index = check_step(gpu, target, normals, source, R.identity(), CAP, what="NaN and Inf source points")
    assert np.all(index[[3, 64, 699]] == -1) and got["pairs"] == int((index >= 0).sum())
    # a finite point that the transform sends to infinity is one of them
    big = R.identity()
    big[0, 3] = 1e300
    got, index = check_step(gpu, target, normals, source, big, CAP, what="q not finite")
    assert got["pairs"] == 0 and np.all(index == -1)


def test_cap_on_the_distance_of_a_pair_and_caps_without_pairs(gpu, cases):
    target, _, _, _ = cases[MOTIONS[0]]
    rng = np.random.default_rng(6)
    queries = (target[:1500] + rng.normal(size=(1500, 3)) * 0.01).astype(np.float32)
    d2 = np.sort(np.array([sqdist_f32(queries[i], target).min() for i in range(64)], np.float32))
    # a cap whose f32 square is exactly the f32 squared distance of one pair: d2 == cap2 is accepted
    caps = [c for c in np.sqrt(d2.astype(np.float64)).astype(np.float32) if np.float32(c) * np.float32(c) in d2]
    assert caps
    cap = caps[len(caps) // 2]
    got, index = check_step(gpu, target, None, queries, R.identity(), cap, what="cap on a pair's distance")
    on_cap = [i for i in np.flatnonzero(index >= 0)
              if sqdist_f32(queries[i], target[index[i]]) == np.float32(cap) * np.float32(cap)]
    assert on_cap, "no accepted pair lies on the cap"
    got, index = check_step(gpu, target, None, queries + np.float32(0.5), R.identity(), 1e-4, what="no pairs")
    assert got["pairs"] == 0 and np.all(index == -1)
    assert not got["ata"].any() and not got["atb"].any() and got["sq_distance"] == 0.0


def test_cap_larger_than_the_frame_equals_nearest_point(gpu, cases):
    target, _, source, _ = cases[MOTIONS[0]]
    rng = np.random.default_rng(8)
    queries = np.concatenate([source[:1000], rng.uniform(-3, 3, (500, 3))]).astype(np.float32)
    frame = margin_frame(target)
    _, index = check_step(gpu, target, None, queries, R.identity(), 100.0, frame, what="cap beyond the frame", sums=False)
    want, _ = ops.nearest_point(frame, dev(gpu, target), dev(gpu, queries))
    assert np.array_equal(index, want.cpu().numpy()) and np.all(index >= 0)


def test_crowded_cells(gpu):
    """eight cells with 1500 points each, beyond the crowding limit of the search (1024): their queries start on a finer
    level of the deepened index"""
    pts, _, _, box = CI.lattice_sites(2, 1500, 5, seed=3)
    frame = _lib.frame_init(*box)
    rng = np.random.default_rng(9)
    queries = np.concatenate([pts[:1500] + rng.normal(size=(1500, 3)) * 1e-3, rng.uniform(0, 0.3, (300, 3))]).astype(np.float32)
    nrm = rng.normal(size=pts.shape).astype(np.float32)
    _, index = check_step(gpu, pts, nrm, queries, R.identity(), 0.01, frame, what="crowded cells")
    assert (index >= 0).sum() > 1000 and (index == -1).any()


def test_zero_and_nan_target_normals_drop_the_pair(gpu, cases):
    target, normals, source, _ = cases[MOTIONS[0]]
    normals = normals.copy()
    normals[::7] = 0
    normals[3::7, 1] = np.nan
    normals[5::7, 2] = np.inf
    got, index = check_step(gpu, target, normals, source, R.motion(*MOTIONS[0]), CAP, what="bad normals, plane")
    _, plain = check_step(gpu, target, None, source, R.motion(*MOTIONS[0]), CAP, what="bad normals, point", sums=False)
    dropped = np.flatnonzero((index == -1) & (plain >= 0))
    assert len(dropped) > 1000 and np.all(np.isin(plain[dropped] % 7, (0, 3, 5)))
    assert np.array_equal(index[index >= 0], plain[index >= 0])


def test_no_source_points(gpu, cases):
    target, normals, _, _ = cases[MOTIONS[0]]
    frame = margin_frame(target)
    empty = torch.zeros((0, 3), dtype=torch.float32, device=gpu)
    for nrm in (normals, None):
        got, index = ops.icp_step(frame, dev(gpu, target), dev(gpu, nrm), empty, R.identity(), (0, 0, 0), CAP,
                                  return_index=True)
        assert got["pairs"] == 0 and not got["ata"].any() and not got["atb"].any() and index.shape == (0,)
        assert got["sq_residual"] == 0.0 and got["sq_distance"] == 0.0 and got["mode"] == int(nrm is not None)
    t, report = ops.register_points(frame, dev(gpu, target), dev(gpu, normals), empty, CAP)
    assert report["degenerate"] and not report["converged"] and report["iterations"] == 1 and report["fitness"] == 0.0
    assert np.array_equal(t, R.identity())


def test_partial_overlap_pairs(gpu, partial):
    target, normals, placed, _ = partial
    got, index = check_step(gpu, target, normals, placed, R.identity(), PARTIAL_CAP, what="partial overlap")
    assert 0.4 < got["pairs"] / len(placed) < 0.7
    assert np.all(index[placed[:, 0] > 1.0 + PARTIAL_CAP] == -1)


# ---- 2. the same bits on every run ------------------------------------------------------------------------------------
def _bits(sums):
    return np.concatenate([sums["ata"], sums["atb"], [sums["sq_residual"], sums["sq_distance"]]]).view(np.int64)


def test_sums_and_driver_are_bit_identical_across_runs_and_contexts(gpu, cases):
    target, normals, source, _ = cases[MOTIONS[1]]
    frame = margin_frame(target)
    args = (frame, dev(gpu, target), dev(gpu, normals), dev(gpu, source))

    def run():
        sums = ops.icp_step(*args, R.motion(3, 0.02), R.frame_origin(frame), CAP)
        point = ops.icp_step(args[0], args[1], None, args[3], R.motion(3, 0.02), R.frame_origin(frame), CAP)
        t, report = ops.register_points(*args, CAP)
        return np.concatenate([_bits(sums), _bits(point), t.reshape(-1).view(np.int64)]), (sums["pairs"], point["pairs"], report)

    first, info = run()
    again, info2 = run()
    assert np.array_equal(first, again) and info == info2
    with ops.fresh_context(gpu):
        fresh, info3 = run()
    assert np.array_equal(first, fresh) and info == info3


# ---- 3. the driver ----------------------------------------------------------------------------------------------------
def test_one_iteration_is_step_plus_update(gpu, cases):
    target, normals, source, _ = cases[MOTIONS[0]]
    frame = margin_frame(target)
    args = (frame, dev(gpu, target), dev(gpu, normals), dev(gpu, source))
    init = R.motion(1, 0.01)
    for nrm in (args[2], None):
        t, report = ops.register_points(args[0], args[1], nrm, args[3], CAP, init=init, max_iterations=1)
        sums = ops.icp_step(args[0], args[1], nrm, args[3], init, ops.icp_origin(frame), CAP)
        want, xi, degenerate = ops.icp_update(sums, ops.icp_origin(frame), init)
        assert not degenerate and np.array_equal(t.view(np.int64), want.view(np.int64))
        assert report["iterations"] == 1 and not report["converged"] and report["pairs"] == sums["pairs"]
        assert report["rmse"] == np.sqrt(sums["sq_distance"] / sums["pairs"]) and report["fitness"] == sums["pairs"] / len(source)


@pytest.mark.parametrize("motion, plane", [(m, True) for m in MOTIONS] + [(MOTIONS[0], False)],
                         ids=lambda v: ("%ddeg" % v[0]) if isinstance(v, tuple) else ("plane" if v else "point"))
def test_driver_recovers_the_motion(gpu, cases, motion, plane):
    """the maximum coordinate error of T source against the true positions is at most twice that of the restatement's
    driver on the same input plus 4 f32 ulp of the largest coordinate"""
    target, normals, source, truth = cases[motion]
    normals = normals if plane else None
    frame = margin_frame(target)
    iterations = 50 if plane else 200
    t, report = ops.register_points(frame, dev(gpu, target), dev(gpu, normals), dev(gpu, source), CAP,
                                    max_iterations=iterations, translation_tolerance=1e-7)
    ref_t, ref_report = R.driver(target, normals, source, R.frame_origin(frame), CAP, iterations)
    err, ref_err = R.coordinate_error(t, source, truth), R.coordinate_error(ref_t, source, truth)
    limit = 2 * ref_err + 4 * float(np.spacing(np.abs(truth).max()))
    print("motion %s plane %s: %s\n  reference %s\n  max coordinate error %.3e (reference %.3e, limit %.3e)"
          % (motion, plane, report, ref_report, err, ref_err, limit))
    assert ref_report["converged"]
    assert report["converged"] and not report["degenerate"]
    assert report["fitness"] == 1.0 and report["pairs"] == len(source)
    assert err <= limit


def test_driver_on_a_partial_overlap(gpu, partial):
    target, normals, placed, source = partial
    frame = margin_frame(target)
    t, report = ops.register_points(frame, dev(gpu, target), dev(gpu, normals), dev(gpu, source), PARTIAL_CAP,
                                    translation_tolerance=1e-7)
    ref_t, ref_report = R.driver(target, normals, source, R.frame_origin(frame), PARTIAL_CAP, 50)
    print("partial overlap: %s\n  reference %s" % (report, ref_report))
    assert ref_report["converged"] and report["converged"] and not report["degenerate"]
    assert abs(report["fitness"] - ref_report["fitness"]) <= 0.01 * ref_report["fitness"]
    assert 0.4 < report["fitness"] < 0.7
    assert np.abs(t - R.motion(5, 0.05)).max() < 5e-3  # (the pairs along the target's edge pull a little)


def test_planar_target_is_degenerate_in_plane_mode(gpu):
    rng = np.random.default_rng(5)
    flat = np.concatenate([rng.uniform(-1, 1, (4000, 2)), np.zeros((4000, 1))], 1).astype(np.float32)
    up = np.tile(np.float32([0, 0, 1]), (len(flat), 1))
    source = flat[:1000] + np.float32([0.003, -0.002, 0.01])
    frame = margin_frame(flat)
    init = R.motion(0.5, 0.002)
    t, report = ops.register_points(frame, dev(gpu, flat), dev(gpu, up), dev(gpu, source), 0.1, init=init)
    assert report["degenerate"] and not report["converged"] and report["iterations"] == 1
    assert report["pairs"] == len(source) and report["fitness"] == 1.0
    assert np.array_equal(t, init)
    t, report = ops.register_points(frame, dev(gpu, flat), None, dev(gpu, source), 0.1, init=init, max_iterations=3)
    assert not report["degenerate"] and report["iterations"] == 3  # point-to-point has all six directions


# ---- 4. scratch rule, streams -----------------------------------------------------------------------------------------
class _AfterCount:
    """a context stand-in that runs `between` right after the wrapper's *_count call"""

    def __init__(self, ctx, between):
        self.ctx, self.between = ctx, between

    def call(self, name, *args):
        self.ctx.call(name, *args)
        if "_count" in name:
            self.between()


@pytest.mark.parametrize("which", ("icp_step", "register_points"))
def test_a_pending_count_is_voided(gpu, cases, which):
    target, normals, source, _ = cases[MOTIONS[0]]
    frame = margin_frame(target)
    tp, tn, sp = dev(gpu, target[:500]), dev(gpu, normals[:500]), dev(gpu, source[:64])
    ctx = ops.context(gpu)
    want = ops.points_merge(frame, tp, tn, level=4, ctx=ctx)
    if which == "icp_step":
        between = lambda: ops.icp_step(frame, tp, tn, sp, R.identity(), (0, 0, 0), CAP)  # noqa: E731
    else:
        between = lambda: ops.register_points(frame, tp, tn, sp, CAP, max_iterations=2)  # noqa: E731
    with pytest.raises(AsrHipError, match="must follow"):
        ops.points_merge(frame, tp, tn, level=4, ctx=_AfterCount(ctx, between))
    again = ops.points_merge(frame, tp, tn, level=4, ctx=ctx)
    assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])


def test_on_a_side_stream(gpu, cases):
    """inputs that arrive late on a side stream: a kernel enqueued on another stream would read zeros"""
    target, normals, source, _ = cases[MOTIONS[0]]
    frame = margin_frame(target)
    args = [dev(gpu, target), dev(gpu, normals), dev(gpu, source)]
    init, origin = R.motion(2, 0.01), ops.icp_origin(frame)
    torch.cuda.synchronize()
    want, want_index = ops.icp_step(frame, *args, init, origin, CAP, return_index=True)
    want_t, want_report = ops.register_points(frame, *args, CAP, init=init)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    for run in ("step", "driver"):
        (lt, ln, ls), ev = late(side, *args)
        with torch.cuda.stream(side):
            if run == "step":
                got, index = ops.icp_step(frame, lt, ln, ls, init, origin, CAP, return_index=True)
            else:
                got_t, report = ops.register_points(frame, lt, ln, ls, CAP, init=init)
        side.synchronize()
        if run == "step":
            assert np.array_equal(_bits(got), _bits(want)) and got["pairs"] == want["pairs"] == len(source)
            assert torch.equal(index, want_index)
        else:
            assert np.array_equal(got_t.view(np.int64), want_t.view(np.int64)) and report == want_report


# ---- 5. the public surface --------------------------------------------------------------------------------------------
def test_register_transform_merge_gives_one_cloud(gpu):
    """two overlapping halves of a cloud, one moved: registered, moved back and merged they are the cloud again"""
    import adaptivesurfacereconstruction as asr
    cloud, normals = R.surface(20000, 7)
    left, right = cloud[:, 0] < 0.3, cloud[:, 0] > -0.3
    moved = R.transform_f32(R.inverse(R.motion(3, 0.02)), cloud[right])
    result = asr.register_points(moved, cloud[left], normals[left])
    assert result["converged"] and not result["degenerate"] and 0.4 < result["fitness"] < 0.7
    assert result["transform"].shape == (4, 4) and result["transform"].dtype == np.float64
    assert np.array_equal(result["transform"][3], [0, 0, 0, 1])
    assert np.abs(result["transform"][:3] - R.motion(3, 0.02)).max() < 5e-3
    back = asr.transform_points(moved, result["transform"])
    whole = asr.merge_points(cloud, cell_size=0.05)["report"]["clusters"]
    merged = asr.merge_points(np.concatenate([cloud[left], back]), cell_size=0.05)["report"]["clusters"]
    apart = asr.merge_points(np.concatenate([cloud[left], moved]), cell_size=0.05)["report"]["clusters"]
    print("clusters: the cloud %d, the registered halves %d, the halves as they came %d" % (whole, merged, apart))
    assert abs(merged - whole) <= 0.02 * whole < abs(apart - whole)


def test_public_error_paths(gpu):
    import adaptivesurfacereconstruction as asr
    cloud, normals = R.surface(2000, 7)
    bad = cloud.copy()
    bad[17, 2] = np.nan
    nan_init = np.eye(4)
    nan_init[1, 3] = np.nan
    for kwargs in (dict(target=bad), dict(max_distance=0.0), dict(max_distance=-1.0), dict(init=nan_init)):
        with pytest.raises(ValueError):
            asr.register_points(cloud[:100], **dict(dict(target=cloud, target_normals=normals), **kwargs))
    frame = margin_frame(cloud)
    with pytest.raises(AsrHipError, match="non-finite"):  # the library's own check of the target
        ops.icp_step(frame, dev(gpu, bad), None, dev(gpu, cloud[:100]), R.identity(), (0, 0, 0), CAP)
    ctx = ops.context(gpu)
    params, report = _lib.IcpParams(float("nan"), 10, 1e-7, 1e-7), _lib.IcpReport()
    t12 = (ctypes.c_double * 12)(*R.identity().reshape(-1))
    tp = dev(gpu, cloud)
    with pytest.raises(AsrHipError, match="max_distance"):  # ... and of the cap, behind the Python layer's
        ctx.call("asr_hip_register_points", ctypes.byref(frame), _lib.ptr(tp), ops.i64(len(cloud)), None,
                 _lib.ptr(tp), ops.i64(len(cloud)), ctypes.byref(params), t12,
                 ctypes.byref(report))


def test_asrtool_register(gpu, tmp_path, capsys):
    import asrtool
    from asr_hip import ply
    cloud, normals = R.surface(6000, 7)
    pick = np.random.default_rng(2).permutation(len(cloud))[:2000]
    source = R.transform_f32(R.inverse(R.motion(5, 0.05)), cloud[pick])
    source_normals = (normals[pick].astype(np.float64) @ R.motion(5, 0.05)[:, :3]).astype(np.float32)  # R^T n
    radii = np.linspace(0.01, 0.02, len(pick)).astype(np.float32)
    colors = np.random.default_rng(3).integers(0, 256, (len(pick), 3)).astype(np.uint8)
    src, tgt, out = (str(tmp_path / name) for name in ("source.ply", "target.ply", "out.ply"))
    ply.write_points(src, source, source_normals, radii, colors=colors)
    ply.write_points(tgt, cloud, normals)
    for extra, mode in (([], "point-to-plane"), (["--point-to-point", "--iterations", "200"], "point-to-point")):
        assert asrtool.main(["--register", src, tgt, out, "--max-distance", "0.3"] + extra) == 0
        result = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert result["mode"] == mode and result["converged"] and result["fitness"] == 1.0
        assert np.abs(np.array(result["transform"])[:3] - R.motion(5, 0.05)).max() < 1e-5
        points, got_normals, got_radii = ply.read_points(out)
        assert np.abs(points - cloud[pick]).max() < 1e-6
        assert np.abs(got_normals - normals[pick]).max() < 1e-5
        assert np.array_equal(got_radii, radii) and np.array_equal(ply.read_point_colors(out), colors)
