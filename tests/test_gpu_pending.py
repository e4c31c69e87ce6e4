"""GPU tests of the count / fill protocol (include/asr_hip.h "Count / fill pairs", csrc/asr_pending.h): a _fill completes
the most recent successful _count of the same operator and is refused, on the host and before any launch, once another
call has recycled the context's scratch arena -- its parked pointers would lead into that call's memory.

Every pair runs through its ordinary wrapper of asr_hip.ops on a context proxy that sees the wrapper's own ctx.call
sequence and can run an unrelated operator right after the _count, or stop the wrapper there.  Inputs are the smallest
that reach the fill kernels of a pair: the cube without its top of tests/mesh_fill_ref.py, a ring of six hand-made dual
cells (tests/contour_cells.py), 64 points with normals in one frame, and their octree, whose leaves lie on two levels."""
import numpy as np
import pytest
import torch

import contour_cells as C
import mesh_fill_ref as F
from asr_hip import _lib, ops
from asr_hip._lib import AsrHipError

pytestmark = pytest.mark.gpu

PAIRS = ("multi_radius_search", "dual_cells", "contour", "components", "mesh_simplify", "mesh_edges", "mesh_fill_holes",
         "points_merge")


class _Stop(Exception):
    pass


class Proxy:
    """stands in for the context: hands every ctx.call on and keeps it in .calls; after a *_count, `between` runs (its
    own calls are not kept), then `stop` ends the wrapper"""

    def __init__(self, ctx, between=None, stop=False):
        self.ctx, self.between, self.stop, self.calls = ctx, between, stop, []

    def call(self, name, *args):
        self.ctx.call(name, *args)
        if self.calls is None:
            return
        self.calls.append((name,) + args)
        if "_count" in name:
            if self.between:
                kept, self.calls = self.calls, None
                try:
                    self.between()
                finally:
                    self.calls = kept + [("between",)]
            if self.stop:
                raise _Stop(name)


@pytest.fixture(scope="module")
def pairs(gpu):
    """({pair: wrapper(ctx)} on fixed inputs, the unrelated operator)"""
    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    rng = np.random.default_rng(12)
    frame = _lib.frame_init((-0.5,) * 3, (1.5,) * 3)
    pts = rng.uniform(0.0, 1.0, (64, 3)).astype(np.float32)
    nrm = rng.standard_normal((64, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tp, tn, tr = t(pts), t(nrm), t(np.where(np.arange(64) % 2 == 0, 0.25, 0.03).astype(np.float32))
    nodes, leaves = ops.octree_build(frame, tp, tr)
    levels = {(int(k).bit_length() - 1) // 3 for k in leaves.cpu().numpy()}
    assert len(levels) >= 2, levels
    centers, sizes = ops.voxel_info(frame, leaves)
    mv, mt = F.open_cube()
    tv, tt = t(mv), t(mt)
    cv, cd, cp = (t(a) for a in C.ring(6, pad=3))

    def radius_search(ctx):  # the one wrapper without a ctx argument: it asks ops.context
        real = ops.context
        ops.context = lambda device=None: ctx
        try:
            return ops.multi_radius_search(frame, tp, tr, centers, sizes)
        finally:
            ops.context = real

    wrappers = {
        "multi_radius_search": radius_search,
        "dual_cells": lambda ctx: (ops.dual_cells(gpu, ctx=ctx, nodes=nodes, leaves=leaves),),
        "contour": lambda ctx: ops.contour(cv, cd, cp, 1.0, ctx=ctx),
        "components": lambda ctx: ops.remove_components(tv, tt, 1, ctx=ctx),
        "mesh_simplify": lambda ctx: ops.mesh_simplify(frame, tv, tt, level=3, return_map=True, ctx=ctx),
        "mesh_edges": lambda ctx: ops.mesh_edges(tt, len(mv), ctx=ctx),
        "mesh_fill_holes": lambda ctx: ops.mesh_fill_holes(tv, tt, 4, ctx=ctx),
        "points_merge": lambda ctx: ops.points_merge(frame, tp, tn, tr, level=2, split_sides=True, return_map=True,
                                                     return_counts=True, ctx=ctx),
    }
    assert set(wrappers) == set(PAIRS)
    return wrappers, lambda: ops.nearest_point(frame, tp, tp[:8])  # 8 queries: recycles the scratch arena


def _same(got, want):
    assert len(got) == len(want)
    for x, y in zip(got, want):
        if y is None:
            assert x is None
            continue
        assert x.dtype == y.dtype and x.shape == y.shape and y.numel() > 0
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) if y.dtype == torch.float32 else torch.equal(x, y)


@pytest.mark.parametrize("name", PAIRS)
def test_fill_refused_after_scratch_reuse(gpu, pairs, name):
    wrappers, between = pairs
    ctx = ops.context(gpu)
    want = wrappers[name](ctx)
    spy = Proxy(ctx, between)
    with pytest.raises(AsrHipError, match="must follow"):
        wrappers[name](spy)
    seen = [c[0] for c in spy.calls]  # (the refused fill raised inside ctx.call: it is not kept)
    assert len(seen) == 2 and "_count" in seen[0] and seen[1] == "between", seen
    _same(wrappers[name](ctx), want)  # the context still works: the same bits as before


@pytest.mark.parametrize("a, b", list(zip(PAIRS, PAIRS[1:] + PAIRS[:1])))
def test_fill_refused_after_another_pairs_count(gpu, pairs, a, b):
    wrappers, _ = pairs
    ctx = ops.context(gpu)
    fills, want = {}, {}
    for name in (a, b):  # an ordinary run: the result, and the fill call with its arguments (they point into `want`)
        spy = Proxy(ctx)
        want[name] = wrappers[name](spy)
        fills[name] = spy.calls[-1]
        assert fills[name][0].endswith("_fill")
    with pytest.raises(_Stop):
        wrappers[a](Proxy(ctx, stop=True))  # a's count is pending
    with pytest.raises(AsrHipError, match="must follow"):
        ctx.call(*fills[b])
    with pytest.raises(AsrHipError, match="must follow"):
        ctx.call(*fills[a])  # the refused fill took a's count with it
    for name in (a, b):
        _same(wrappers[name](ctx), want[name])
