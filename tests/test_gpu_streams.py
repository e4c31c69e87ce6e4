"""The stream contract (include/asr_hip.h: "all kernels are enqueued on the context's hipStream_t"; asr_hip/ops.py: the
process-wide context works "on torch's current stream") on streams other than torch's default one.

  1. every operator family, called inside `with torch.cuda.stream(S)` with inputs whose bytes arrive LATE on S
     (stream_helpers.late), gives what it gives on the default stream: a kernel or copy enqueued anywhere but on S reads
     zeros, or is read before it ran;
  2. moving a context to another stream orders that stream behind the old one (asr_hip_context_set_stream);
  3. ops that alternate between two streams give single-stream results;
  4. ImplicitPipeline.get() copies on torch's current stream.

Limits are in DESIGN.md 4.10: the late inputs expose only what an op enqueues before its first host read-back, and
two host threads on one context stay unsupported."""
import numpy as np
import pytest
import torch

import parity
from asr_hip import _lib, ops, synth
from asr_hip.pipeline import ImplicitPipeline
from oracle import oracle as O
from stream_helpers import delay, late, late_inplace

pytestmark = pytest.mark.gpu

_close = parity.assert_close
DEC = ("dense_decoder1.weight", "dense_decoder1.bias", "dense_decoder2.weight", "dense_decoder2.bias",
       "dense_decoder3.weight")

# Ops whose result is NOT the same bits on every run (established on the default stream, see the test): they are compared
# at the absolute tolerance of their own oracle test instead.  Everything else must be bit-stable and bit-equal.
NOT_BIT_STABLE = {}


# ---- shared inputs, computed once ------------------------------------------------------------------------------------
class Env:
    def __init__(self, gpu):
        self.gpu = gpu
        self._memo = {}

    def t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.gpu)

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    @property
    def geo(self):
        """the 6 000-point scan cloud of test_gpu_network.geo with the oracle's structures"""
        def make():
            p, q = synth.scan_cloud(6000, seed=11, device="cpu")
            pts, nrm = p.numpy(), q.numpy()
            rad = synth.knn_radii(pts, 24)
            bb = synth.bounding_box(pts, 0.1)
            item = parity.oracle_geometry(pts, rad, *bb)
            d = dict(pts=pts, nrm=nrm, rad=rad, bb=bb, item=item, frame=_lib.frame_init(*bb))
            d["P"], d["N"], d["R"] = self.t(pts), self.t(nrm), self.t(rad)
            d["keys0"] = self.t(item["voxel_keys0"].view(np.int64))
            d["centers0"], d["sizes0"] = self.t(item["voxel_centers0"]), self.t(item["voxel_sizes0"])
            d["nb0"] = tuple(self.t(item[k + "0"]) for k in ("neighbors_index", "neighbors_kernel_index",
                                                            "neighbors_row_splits"))
            d["up0"] = tuple(self.t(item[k + "0"]) for k in ("up_neighbors_index", "up_neighbors_kernel_index",
                                                            "up_neighbors_row_splits"))
            d["v1"] = len(item["voxel_sizes1"])
            return d
        return self.memo("geo", make)

    @property
    def sphere(self):
        """parity.sphere_field(5000, 1, 0.3) with the oracle's mesh of it"""
        def make():
            g, du, values = parity.sphere_field(5000, 1, 0.3)
            pts, _ = synth.sphere_cloud(5000, 1)
            v, t = O.create_triangle_mesh(values, du, g["voxel_centers"], 1.0)
            return dict(values=values, du=du, centers=g["voxel_centers"], v=v, t=t,
                        frame=_lib.frame_init(*synth.bounding_box(pts, 0.1)), V=self.t(v), T=self.t(t),
                        VALUES=self.t(values), DU=self.t(du), CENTERS=self.t(g["voxel_centers"]))
        return self.memo("sphere", make)

    @property
    def weights(self):
        return self.memo("weights", lambda: synth.make_weights(channel_div=4, seed=3))

    def cconv(self, cin, cout, small=False):
        """a ragged neighbour list with one row above 256 pairs (the long-row kernels), rows of 0 pairs, several blocks"""
        def make():
            rng = np.random.default_rng(100 * cin + cout + small)
            n, v = (1500, 300) if small else (3000, 700)
            lens = rng.integers(0, 40, size=v)
            lens[0], lens[5], lens[v - 1] = 0, 300 if not small else 260, 0
            pos = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
            feat = rng.standard_normal((n, cin)).astype(np.float32)
            out_pos = rng.uniform(-0.3, 0.3, size=(v, 3)).astype(np.float32)
            ext = rng.uniform(1.5, 3.0, size=v).astype(np.float32)
            rs = np.zeros(v + 1, np.int64)
            rs[1:] = np.cumsum(lens)
            idx = np.concatenate([rng.choice(n, size=l, replace=False) for l in lens]).astype(np.int32)
            imp = rng.uniform(0.1, 1, size=rs[-1]).astype(np.float32)
            W = (rng.standard_normal((4, 4, 4, cin, cout)) * 0.5).astype(np.float32)
            b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
            ref = np.maximum(O.continuous_conv(W, out_pos, ext, pos, feat, idx, imp, rs, True) + b, 0)
            return [self.t(x) for x in (W, out_pos, ext, pos, feat, idx, imp, rs, b)], ref
        return self.memo(("cconv", cin, cout, small), make)

    def sconv(self, cin, cout, scale=1.0):
        """one 55-slot layer over grid 0 of the scan cloud -> ([W, f, idx, kidx, rs, b], oracle result)"""
        def make():
            item = self.geo["item"]
            idx, kidx, rs = (item[k + "0"] for k in ("neighbors_index", "neighbors_kernel_index", "neighbors_row_splits"))
            rng = np.random.default_rng(cin * 1000 + cout)
            f = (rng.standard_normal((len(rs) - 1, cin)) * scale).astype(np.float32)
            W = (rng.standard_normal((55, cin, cout)) * np.sqrt(2.0 / (8 * cin))).astype(np.float32)
            b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
            return [self.t(W), self.t(f)] + list(self.geo["nb0"]) + [self.t(b)], (W, f, idx, kidx, rs, b)
        return self.memo(("sconv", cin, cout, scale), make)

    def sconv_ref(self, cin, cout):
        def make():
            W, f, idx, kidx, rs, b = self.sconv(cin, cout)[1]
            return np.maximum(O.sparse_conv(W, f, idx, kidx, None, rs, False) + b, 0)
        return self.memo(("sconv_ref", cin, cout), make)

    def pipe(self, precision):
        return self.memo(("pipe", precision), lambda: ImplicitPipeline(self.weights, device=self.gpu, precision=precision))


@pytest.fixture(scope="module")
def env(gpu):
    return Env(gpu)


@pytest.fixture(scope="module")
def two_streams(gpu):
    """the two side streams of tests 2 and 3 (one pair for all of them: which streams share a hardware queue, and so run in
    order whatever the library does, is decided when a stream is first used)"""
    return torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)


# ---- comparing results -----------------------------------------------------------------------------------------------
def _flat(x):
    """the tensors / Python values of an op's result, in order"""
    if isinstance(x, (tuple, list)):
        return [y for e in x for y in _flat(e)]
    if isinstance(x, dict):
        return [x[k] for k in sorted(x)]
    return [x]


def _same_bits(a, b):
    if not isinstance(a, torch.Tensor):
        return a == b
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _assert_equal(name, got, ref, what):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        if name in NOT_BIT_STABLE and isinstance(a, torch.Tensor) and a.is_floating_point():
            _close(a.float().cpu().numpy(), b.float().cpu().numpy(), NOT_BIT_STABLE[name])
        else:
            assert _same_bits(a, b), "%s: output %d %s" % (name, i, what)


# ---- the operator table ----------------------------------------------------------------------------------------------
# name -> (build(env) -> (tensor arguments, run(*arguments) -> result[, check(flat result) against the oracle]),
#          asynchronous: the op reads no size back, so it returns while its stream is still busy,
#          options of the process-wide context during the case, inplace: the late bytes arrive in the arguments' own storage)
CASES = {}


def case(name, asynchronous=False, options=None, inplace=False):
    def deco(f):
        CASES[name] = (f, asynchronous, options or {}, inplace)
        return f
    return deco


# geometry
@case("octree_build")
def _(e):
    g = e.geo
    return [g["P"], g["R"]], lambda p, r: ops.octree_build(g["frame"], p, r)


@case("octree_build-grow1")
def _(e):
    g = e.geo
    return [g["P"], g["R"]], lambda p, r: ops.octree_build(g["frame"], p, r, grow_steps=1)


@case("octree_build_parts")
def _(e):
    g = e.geo
    extra = ops.octree_build_parts(g["frame"], g["P"][3000:].contiguous(), g["R"][3000:].contiguous(), balance=False)[0]
    return ([g["P"][:3000].contiguous(), g["R"][:3000].contiguous(), extra],
            lambda p, r, k: ops.octree_build_parts(g["frame"], p, r, extra_keys=k))


@case("dual_cells")
def _(e):
    g = e.geo
    nodes, leaves = ops.octree_build(g["frame"], g["P"], g["R"])
    return [nodes, leaves], lambda n, l: ops.dual_cells(e.gpu, nodes=n, leaves=l)


@case("grid_neighbors")
def _(e):
    return [e.geo["keys0"]], ops.grid_neighbors


@case("grid_neighbors_rows")
def _(e):
    keys = e.geo["keys0"]
    rows = torch.arange(1, keys.shape[0], 3, dtype=torch.int32, device=e.gpu)
    return [keys, rows], ops.grid_neighbors_rows


@case("grid_coarsen")
def _(e):
    return [e.geo["keys0"]], ops.grid_coarsen


@case("voxel_info", asynchronous=True)
def _(e):
    g = e.geo
    return [g["keys0"]], lambda k: ops.voxel_info(g["frame"], k)


@case("point_keys", asynchronous=True)
def _(e):
    g = e.geo
    return [g["P"], g["R"]], lambda p, r: ops.point_keys(g["frame"], p, r)


@case("multi_radius_search")
def _(e):
    g = e.geo
    item = g["item"]

    def check(out):  # tests/test_gpu_geometry.py test_multi_radius_search
        idx, dist, rs, compat = (x.cpu().numpy() for x in out)
        assert np.array_equal(rs, item["aggregation_row_splits"])
        assert np.array_equal(idx, item["aggregation_neighbors_index"])
        assert np.array_equal(dist, item["aggregation_neighbors_dist"])
        assert np.abs(compat - item["aggregation_scale_compat"]).max() <= 1e-6
    return ([g["P"], g["R"], g["centers0"], g["sizes0"]],
            lambda p, r, c, s: ops.multi_radius_search(g["frame"], p, r, c, s), check)


def _knn(e):
    g = e.geo
    return [g["P"], g["R"]], lambda p, r: ops.knn_radius(g["frame"], p, 24, radii=r, want_inlier=True)


case("knn_radius-cells")(_knn)
case("knn_radius-waves", options={"knn_cells": 0})(_knn)


@case("radius_neighbor_count")
def _(e):
    g = e.geo
    return [g["P"], g["R"]], lambda p, r: ops.radius_neighbor_count(g["frame"], p, r)


def _positions(e, m=3001):
    g = e.geo
    rng = np.random.default_rng(5)
    lo, hi = np.asarray(g["bb"][0], np.float32), np.asarray(g["bb"][1], np.float32)
    return e.t(rng.uniform(lo, hi, size=(m, 3)).astype(np.float32))


@case("nearest_point")
def _(e):
    g = e.geo
    return [g["P"], _positions(e)], lambda p, q: ops.nearest_point(g["frame"], p, q)


@case("leaf_locate")
def _(e):
    g = e.geo
    _, leaves = ops.octree_build(g["frame"], g["P"], g["R"])
    return [leaves, _positions(e)], lambda l, q: ops.leaf_locate(g["frame"], l, q)


@case("point_attributes_at")
def _(e):
    g = e.geo
    q, s = g["centers0"][:3001].contiguous(), g["sizes0"][:3001].contiguous()
    return ([g["P"], g["R"], g["N"], q, s],
            lambda p, r, a, q, s: ops.point_attributes_at(g["frame"], p, r, a, q, s, return_info=True))


@case("invert_neighbors_list")
def _(e):
    g = e.geo
    idx, kidx, rs = g["up0"]
    return [idx, rs, kidx], lambda i, r, k: ops.invert_neighbors_list(g["v1"], i, r, k)


@case("row_groups")
def _(e):
    _, kidx, rs = e.geo["nb0"]
    return [kidx, rs], lambda k, r: ops.row_groups(k, r, 256)


# network
@case("aggregation_importance", asynchronous=True)
def _(e):
    item = e.geo["item"]
    return [e.t(item["aggregation_scale_compat"]), e.t(item["aggregation_neighbors_dist"])], ops.aggregation_importance


def _cconv(cin, cout):
    def build(e):
        args, ref = e.cconv(cin, cout)

        def run(W, op, ext, ip, f, idx, imp, rs, b):
            return ops.continuous_conv(W, op, ext, ip, f, idx, imp, rs, True, bias=b, relu=True)
        # rows above 256 pairs: the tolerance of tests/test_gpu_network.py test_continuous_conv_ragged_and_long_rows
        return args, run, lambda out: _close(out[0].cpu().numpy(), ref, 2e-5)
    return build


case("continuous_conv-4to32", asynchronous=True)(_cconv(4, 32))   # matrix-core contraction
case("continuous_conv-7to33", asynchronous=True)(_cconv(7, 33))   # general kernel


@case("continuous_conv_basis", asynchronous=True)
def _(e):
    W, op, ext, ip, f, idx, imp, rs, b = e.cconv(4, 32)[0]
    return [op, ext, ip, f, idx, imp, rs], ops.continuous_conv_basis


def _sconv(algo):
    def build(e):
        args = e.sconv(32, 32)[0]

        def run(W, f, idx, kidx, rs, b):
            return ops.sparse_conv(W, f, idx, kidx, rs, bias=b, relu=True, algo=algo)
        return args, run, lambda out: _close(out[0].cpu().numpy(), e.sconv_ref(32, 32))
    return build


case("sparse_conv-algo1", asynchronous=True)(_sconv(1))
case("sparse_conv-algo2", asynchronous=True)(_sconv(2))

MODE_ID = {"f16": 1, "bf16x3": 2, "f16x2": 3, "bf16x3_2acc": 4}


def _run16(e, mode, cin, cout, plan, expect_plan, **kw):
    ctx = ops.context(e.gpu)

    def run(packed, f, idx, kidx, rs, b):
        ctx.sconv_variant_counts(reset=True)
        out = ops.sparse_conv16(mode, packed, 55, cin, cout, f, idx, kidx, rs, bias=b, relu=True, plan=plan,
                                out_dtype=torch.float32, **kw)  # f16x2: no inp_absmax, the maximum lives in the context
        keys = list(ctx.sconv_variant_counts())
        assert len(keys) == 1 and keys[0][6] == expect_plan, keys  # the plan-driven / the table-driven kernel
        return out
    return run


def _sconv16_plan(mode):
    """the smallest plan-driven bench instance (tests/sconv_instances.py: NT 2, KC 32, 8 waves) with a ConvPlan built
    beforehand: the call itself reads nothing back.  The late bytes arrive in place -- the plan points to these arrays."""
    def build(e):
        W, f, idx, kidx, rs, b = e.sconv(32, 32)[0]
        idx, kidx, rs = idx.clone(), kidx.clone(), rs.clone()
        f = f.half() if mode == "f16" else f.clone()
        packed = ops.pack_filters(W, mode)
        plan = ops.ConvPlan(55, idx, kidx, rs)
        return [packed, f, idx, kidx, rs, b.clone()], _run16(e, mode, 32, 32, plan, 1, force_nt=2, force_waves=8)
    return build


def _sconv16_table(mode):
    """cin = 8 fills no panel: the table-driven kernel (option sconv_plan 0: no temporary plan either)"""
    def build(e):
        W, f, idx, kidx, rs, b = e.sconv(8, 24)[0]
        return [ops.pack_filters(W, mode), f, idx, kidx, rs, b], _run16(e, mode, 8, 24, None, 0)
    return build


for _m in ("bf16x3", "bf16x3_2acc", "f16", "f16x2"):
    case("sparse_conv16-%s-plan" % _m, asynchronous=True, inplace=True)(_sconv16_plan(_m))
for _m in ("bf16x3", "f16x2"):
    case("sparse_conv16-%s-table" % _m, asynchronous=True, options={"sconv_plan": 0})(_sconv16_table(_m))


@case("conv_plan+sparse_conv16")
def _(e):
    """the plan itself built from late arrays (its build reads sizes back), then used"""
    W, f, idx, kidx, rs, b = e.sconv(32, 32)[0]
    packed = ops.pack_filters(W, "f16x2")

    def run(f, idx, kidx, rs, b):
        plan = ops.ConvPlan(55, idx, kidx, rs)
        return ops.sparse_conv16("f16x2", packed, 55, 32, 32, f, idx, kidx, rs, bias=b, relu=True, plan=plan)
    return [f, idx, kidx, rs, b], run


@case("pack_filters")
def _(e):
    W = e.sconv(32, 32)[0][0]
    # (f16x2: the last 8 bytes of the 16-byte trailer are spare and never written)
    return [W], lambda w: [ops.pack_filters(w, "f16"), ops.pack_filters(w, "bf16x3"), ops.pack_filters(w, "f16x2")[:-8]]


@case("absmax", asynchronous=True)
def _(e):
    return [e.sconv(32, 32)[0][1]], ops.absmax


@case("reduce_subarrays_sum", asynchronous=True)
def _(e):
    idx, _, rs = e.geo["nb0"]
    g = torch.Generator(device=e.gpu).manual_seed(1)
    pairs = torch.rand(idx.shape[0], device=e.gpu, generator=g)
    rows = torch.rand(rs.shape[0] - 1, device=e.gpu, generator=g)
    return ([pairs, rows, idx, rs],
            lambda p, v, i, r: (ops.reduce_subarrays_sum(p, r), ops.reduce_subarrays_sum(v, r, i)))


def _decoder(e):
    w = [e.t(e.weights[k]) for k in DEC]
    g = torch.Generator(device=e.gpu).manual_seed(2)
    v = e.geo["sizes0"].shape[0]
    code = torch.randn((v, w[0].shape[1] - 3), device=e.gpu, generator=g)
    return w, code


@case("decode_mlp", asynchronous=True)
def _(e):
    w, code = _decoder(e)
    return [code, e.geo["sizes0"]] + w, lambda c, s, *w: ops.decode_mlp(c, *w, voxel_sizes=s)


@case("decode_mlp_at", asynchronous=True)
def _(e):
    w, code = _decoder(e)
    g = torch.Generator(device=e.gpu).manual_seed(3)
    m = 3001
    shifts = torch.rand((m, 3), device=e.gpu, generator=g) - 0.5
    rows = torch.randint(0, code.shape[0], (m,), device=e.gpu, generator=g, dtype=torch.int32)
    return ([code, shifts, rows, e.geo["sizes0"]] + w,
            lambda c, sh, r, s, *w: ops.decode_mlp_at(c, sh, *w, rows=r, voxel_sizes=s, gradient=True))


# mesh
@case("contour")
def _(e):
    s = e.sphere

    def check(out):  # tests/test_gpu_geometry.py: the oracle's mesh, bit for bit
        assert np.array_equal(out[0].cpu().numpy().view(np.uint32), s["v"].view(np.uint32))
        assert np.array_equal(out[1].cpu().numpy(), s["t"])
    return [s["VALUES"], s["DU"], s["CENTERS"]], lambda v, d, c: ops.contour(v, d, c, 1.0), check


@case("remove_components")
def _(e):
    s = e.sphere
    return [s["V"], s["T"]], lambda v, t: ops.remove_components(v, t, 4, 3)


@case("mesh_simplify")
def _(e):
    s = e.sphere
    return [s["V"], s["T"]], lambda v, t: ops.mesh_simplify(s["frame"], v, t, level=4, return_map=True)


@case("mesh_edges")
def _(e):
    s = e.sphere
    return [s["T"]], lambda t: ops.mesh_edges(t, s["V"].shape[0])


@case("mesh_topology")
def _(e):
    s = e.sphere
    return [s["T"]], lambda t: ops.mesh_topology(t, s["V"].shape[0])


@case("mesh_smooth")
def _(e):
    s = e.sphere
    return [s["V"], s["T"]], lambda v, t: ops.mesh_smooth(v, t, iterations=3)


@case("mesh_sample")
def _(e):
    s = e.sphere
    return [s["V"], s["T"]], lambda v, t: ops.mesh_sample(v, t, 3001, seed=7, normals=True, return_triangle=True)


# whole path: forward (the auxiliary search stream then hangs off a side stream), query and mesh on the same stream
def _pipeline(precision):
    def build(e):
        g = e.geo
        pipe = e.pipe(precision)

        def run(p, n, r, q):
            values = pipe.forward(p, n, r, *g["bb"])
            return values, pipe.query(q, gradient=True, return_rows=True), pipe.mesh()
        return [g["P"], g["N"], g["R"], _positions(e)], run
    return build


case("pipeline-f32")(_pipeline("f32"))
case("pipeline-f16x2")(_pipeline("f16x2"))


# ---- 1. a side stream gives what the default stream gives ----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_side_stream_equals_default_stream(env, gpu, name):
    build, asynchronous, options, inplace = CASES[name]
    ctx = ops.context(gpu)
    before = {k: ctx.get_option(k) for k in options}
    for k, v in options.items():
        ctx.set_option(k, v)
    try:
        built = build(env)
        args, run, check = built if len(built) == 3 else built + (None,)
        torch.cuda.synchronize()
        ref = _flat(run(*args))
        torch.cuda.synchronize()
        again = _flat(run(*args))
        torch.cuda.synchronize()
        if name not in NOT_BIT_STABLE:
            _assert_equal(name, again, ref, "differs between two runs on the default stream")
        if check:
            check(ref)  # "both streams equally wrong" must not pass
        side = torch.cuda.Stream(device=gpu)
        if inplace:
            ev, keep = late_inplace(side, *args)
            largs = args
        else:
            largs, ev = late(side, *args)
        with torch.cuda.stream(side):
            got = _flat(run(*largs))
            window_open = not ev.query()
        if asynchronous:
            # the op returned while the delay in front of its inputs was still running: what it enqueued had to wait
            assert window_open, "%s returned after the delay had ended: it waited, or the delay is too short" % name
        side.synchronize()
        _assert_equal(name, got, ref, "on a side stream differs from the default stream")
        if check:
            check(got)
    finally:
        torch.cuda.synchronize()
        for k, v in before.items():
            ctx.set_option(k, v)


# ---- 2. a stream switch orders the new stream behind the old one ---------------------------------------------------
def _cc(args):
    W, op, ext, ip, f, idx, imp, rs, b = args
    return ops.continuous_conv(W, op, ext, ip, f, idx, imp, rs, True, bias=b, relu=True)


def test_stream_switch_orders_the_new_stream_behind_the_old_one(env, gpu, two_streams):
    """A: 50 ms of delay, then a continuous conv with a long row (its row list and counters live in the context's scratch
    arena).  B, at once: another conv on a smaller geometry, which rewinds that arena.  B's op may not finish before A's
    work.  (Without the ordering nothing overlaps here: B is done while A still sleeps.)"""
    big, small = env.cconv(4, 32)[0], env.cconv(4, 32, small=True)[0]
    torch.cuda.synchronize()
    want_x, want_y = _cc(big), _cc(small)
    torch.cuda.synchronize()
    a, b = two_streams
    ea, eb = torch.cuda.Event(), torch.cuda.Event()
    delay(a, 50.0)
    with torch.cuda.stream(a):
        x = _cc(big)
        ea.record(a)
    with torch.cuda.stream(b):
        y = _cc(small)
        eb.record(b)
    eb.synchronize()
    ordered = ea.query()
    torch.cuda.synchronize()
    assert ordered, "the op on stream B finished before the work of stream A that shares the context's scratch memory"
    _assert_equal("continuous_conv-4to32", [x], [want_x], "on stream A differs from the default stream")
    _assert_equal("continuous_conv-4to32", [y], [want_y], "on stream B differs from the default stream")


def test_stream_switch_of_a_pipeline_orders_query_behind_forward(env, gpu, two_streams):
    """forward on A behind a delay, query on B: the query reads the forward's code and may not pass it"""
    g = env.geo
    pipe = ImplicitPipeline(env.weights, device=gpu)
    q = _positions(env)
    pipe.forward(g["P"], g["N"], g["R"], *g["bb"])
    want = pipe.query(q)
    torch.cuda.synchronize()
    a, b = two_streams
    ea, eb = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(a):
        pipe.forward(g["P"], g["N"], g["R"], *g["bb"])  # (reads sizes back: the delay goes behind it)
    delay(a, 50.0)
    ea.record(a)
    with torch.cuda.stream(b):
        got = pipe.query(q)
        eb.record(b)
    eb.synchronize()
    ordered = ea.query()
    torch.cuda.synchronize()
    assert ordered, "the query on stream B finished before stream A, which the pipeline's context had just left"
    assert _same_bits(got, want)


# ---- 3. alternating streams ----------------------------------------------------------------------------------------
def test_alternating_streams_give_single_stream_results(env, gpu, two_streams):
    """twenty ops, no delays, two side streams in turn; shapes and ops change from call to call"""
    g, s = env.geo, env.sphere
    big, small = env.cconv(4, 32)[0], env.cconv(4, 32, small=True)[0]
    W, f, idx, kidx, rs, b = env.sconv(8, 24)[0]
    packed = ops.pack_filters(W, "f16x2")
    f_huge = (f * 1e6).contiguous()  # the input maximum of f16x2 lives in the context: two inputs 1e6 apart
    ctx = ops.context(gpu)
    before = ctx.get_option("sconv_plan")

    def conv16(x):
        return ops.sparse_conv16("f16x2", packed, 55, 8, 24, x, idx, kidx, rs, bias=b, relu=True)
    cc, search = "continuous_conv-4to32", "multi_radius_search"
    jobs = [(cc, lambda: _cc(big)), ("sparse_conv16-f16x2-table", lambda: conv16(f)), (cc, lambda: _cc(small)),
            ("sparse_conv16-f16x2-table", lambda: conv16(f_huge)),
            (search, lambda: ops.multi_radius_search(g["frame"], g["P"], g["R"], g["centers0"], g["sizes0"])),
            (cc, lambda: _cc(big)), ("contour", lambda: ops.contour(s["VALUES"], s["DU"], s["CENTERS"], 1.0)),
            ("sparse_conv16-f16x2-table", lambda: conv16(f_huge)), (cc, lambda: _cc(small)),
            ("sparse_conv16-f16x2-table", lambda: conv16(f))]
    try:
        ctx.set_option("sconv_plan", 0)  # the table-driven kernel: nothing is read back between the maximum and its use
        torch.cuda.synchronize()
        want = []
        for _, job in jobs:
            want.append(_flat(job()))
            torch.cuda.synchronize()
        streams = two_streams
        got = []
        for i in range(20):
            with torch.cuda.stream(streams[i % 2]):
                got.append(_flat(jobs[i % len(jobs)][1]()))
        torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        ctx.set_option("sconv_plan", before)
    for i, out in enumerate(got):
        _assert_equal(jobs[i % len(jobs)][0], out, want[i % len(jobs)],
                      "of alternating call %d differs from the default stream" % i)


# ---- 4. Pipeline.get() follows torch's current stream ---------------------------------------------------------------
def test_pipeline_get_follows_the_current_stream(env, gpu):
    g = env.geo
    pipe = ImplicitPipeline(env.weights, device=gpu)
    pipe.forward(g["P"], g["N"], g["R"], *g["bb"])
    torch.cuda.synchronize()
    want = {k: pipe.get(k).cpu() for k in ("voxel_centers0", "values")}
    verts = env.sphere["V"]
    want_levels = pipe.simplify_levels(verts, 1).cpu()
    a = torch.cuda.Stream(device=gpu)

    def poison():
        # blocks of the sizes get() is about to ask for, filled with 0xFF and freed: the caching allocator hands them
        # back, so that a copy that has not run yet shows as wrong content instead of a lucky old copy
        v0 = want["values"].shape[0]
        for nbytes in (12 * v0, 8 * v0, 8 * v0):  # voxel_centers0, values, voxel_keys0
            junk = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu)
            del junk
        torch.cuda.synchronize()

    for what in ("get", "simplify_levels"):
        poison()
        with torch.cuda.stream(a):
            pipe.forward(g["P"], g["N"], g["R"], *g["bb"])
        delay(a, 30.0)
        # torch's current stream is the default one again
        if what == "get":
            got = {k: pipe.get(k).cpu() for k in want}
        else:
            got_levels = pipe.simplify_levels(verts, 1).cpu()
        torch.cuda.synchronize()
        if what == "get":
            for k in want:
                assert _same_bits(got[k], want[k]), "get(%r) on the default stream was read before it had been written" % k
        else:
            assert _same_bits(got_levels, want_levels), "simplify_levels read voxel_keys0 before get() had written it"
