"""hip-event timing of asr_hip_point_attributes_at (ops.point_attributes_at) against the composition of the
ops that did its job before it existed -- multi_radius_search -> squared distance / size^2 -> aggregation_importance ->
gather, multiply, reduce_subarrays_sum -> divide; for max_widen = 3 the same again, with twice the size, on the rows still
below min_weight -- on the seeded C3 cloud of bench.py with the mesh vertices of its
forward as queries, C = 3.  The two sides alternate inside one process; per side the best of --reps after a warm-up, and
the spread (max / min - 1) of those repetitions, which is the only margin a comparison of the two may use.  Also: the
peak extra device memory of each side (torch allocations + growth of the library's arena, each side on a context of its
own) and the bytes per query the fused call has to move (position, size, output, its members' 16 + 4 + 4 C bytes)
against what its time at the HBM rate would move.  Prints one JSON line.

    python scripts/attr_time.py [--points 10000000] [--reps 5] [--channels 3]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "adaptive-surface-reconstruction_amd"), REPO]

from asr_hip import _lib, ops, synth  # noqa: E402
from asr_hip.pipeline import ImplicitPipeline  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth


def composition(frame, points, radii, attr, positions, sizes):
    """max_widen = 0 from the ops of the search and the aggregation block -> (A [M,C], weight [M], pairs)"""
    idx, dist, rs, compat = ops.multi_radius_search(frame, points, radii, positions, sizes)
    cnt = rs[1:] - rs[:-1]
    row = torch.repeat_interleave(torch.arange(cnt.shape[0], device=cnt.device), cnt)
    imp = ops.aggregation_importance(compat, dist / (sizes * sizes)[row])
    den = ops.reduce_subarrays_sum(imp, rs)
    num = torch.stack([ops.reduce_subarrays_sum(imp * attr[idx.long(), ch], rs) for ch in range(attr.shape[1])], 1)
    return num / den[:, None], den, idx.numel()


def composition_widened(frame, points, radii, attr, positions, sizes, max_widen, min_weight=1e-2):
    """the same job as the fused call with max_widen > 0: the composition again on the rows still below min_weight, with
    twice the size each time -> A [M,C] (0 where no k qualifies)"""
    out = torch.zeros((positions.shape[0], attr.shape[1]), device=positions.device)
    todo = torch.arange(positions.shape[0], device=positions.device)
    for k in range(max_widen + 1):
        if not todo.numel():
            break
        a, den, _ = composition(frame, points, radii, attr, positions[todo].contiguous(), (sizes[todo] * 2.0 ** k).contiguous())
        done = den >= min_weight
        out[todo[done]] = a[done]
        todo = todo[~done]
    return out


def once(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def peak_extra(fn, index):
    """peak device bytes `fn` needs beyond what is live now: torch's allocator plus the arena of a fresh context"""
    keep = ops._ctx.pop(index, None)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base + ops._ctx[index].reserved_bytes()
    ops._ctx.pop(index).close()
    if keep is not None:
        ops._ctx[index] = keep
    return extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--channels", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pts, nrm = synth.scan_cloud(args.points, seed=0, device=dev)
    rad = synth.knn_radii_gpu(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    pipe = ImplicitPipeline(synth.make_weights(1, seed=2), device=dev)
    pipe.forward(pts, nrm, rad, bb[0], bb[1])
    verts, _ = pipe.mesh()
    queries = "mesh_vertices"
    if verts.shape[0] < 1000:  # (a seeded net need not have a surface: say so in the output)
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        verts = (pts + 0.5 * rad[:, None] * torch.randn(pts.shape, device=dev, generator=g)).contiguous()
        queries = "displaced_points"
    frame = _lib.frame_init(*bb)
    rows = ops.leaf_locate(frame, pipe.get("voxel_keys0"), verts).long()
    sizes = torch.where(rows >= 0, pipe.get("voxel_sizes0")[rows.clamp(min=0)], torch.zeros((), device=dev)).contiguous()
    del pipe, nrm, rows
    torch.cuda.empty_cache()
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    attr = (255 * torch.rand((args.points, args.channels), device=dev, generator=g)).contiguous()
    m, c = verts.shape[0], args.channels
    out = torch.empty((m, c), device=dev)
    weight = torch.empty(m, device=dev)
    widen = torch.empty(m, dtype=torch.int8, device=dev)
    ctx = ops.context(dev)

    def fused(max_widen):
        ctx.call("asr_hip_point_attributes_at", ctypes.byref(frame), _lib.ptr(pts), _lib.ptr(rad), ops.i64(args.points),
                 _lib.ptr(attr), c, _lib.ptr(verts), _lib.ptr(sizes), ops.i64(m), max_widen, ctypes.c_float(1e-2),
                 ctypes.c_float(0.0), _lib.ptr(out), _lib.ptr(weight), _lib.ptr(widen))

    sides = {"fused_widen0": lambda: fused(0), "composition": lambda: composition(frame, pts, rad, attr, verts, sizes),
             "fused_widen3": lambda: fused(3),
             "composition_widen3": lambda: composition_widened(frame, pts, rad, attr, verts, sizes, 3)}
    failed = {}
    for k in list(sides):  # warm-up: code objects, arena slabs, torch's allocator
        try:
            sides[k]()
            torch.cuda.synchronize()
        except (RuntimeError, _lib.AsrHipError) as e:  # e.g. the widened composition's pair arrays do not fit
            if not k.startswith("composition"):
                raise
            failed[k] = str(e)[:200]
            del sides[k]
            torch.cuda.empty_cache()
    ms = {k: [] for k in sides}
    for _ in range(args.reps):  # alternating
        for k, fn in sides.items():
            ms[k].append(once(fn))
    res = {"points": args.points, "queries": queries, "m": m, "channels": c, "reps": args.reps,
           "ms_best": {k: round(min(v), 3) for k, v in ms.items()},
           "spread": {k: round(max(v) / min(v) - 1, 4) for k, v in ms.items()}}
    # the two sides agree (same rows hit, values to rounding)
    fused(0)
    comp, den, pairs = composition(frame, pts, rad, attr, verts, sizes)
    hit = widen >= 0
    res["pairs"] = pairs
    res["hit_share_widen0"] = round(hit.float().mean().item(), 5)
    res["max_abs_diff_on_hits"] = float((out - comp)[hit].abs().max()) if hit.any() else 0.0
    fused(3)
    if "composition_widen3" in sides:
        comp3 = composition_widened(frame, pts, rad, attr, verts, sizes, 3)
        res["max_abs_diff_widen3"] = float((out - comp3).abs().max())  # (rows at the threshold may differ in k)
        del comp3
    res["failed"] = failed
    res["widen_histogram"] = torch.bincount(widen.long() + 1, minlength=5).tolist()  # -1, 0, 1, 2, 3
    del comp, den
    torch.cuda.empty_cache()
    index = dev.index or 0
    res["peak_extra_bytes"] = {
        "fused_widen0": peak_extra(lambda: ops.point_attributes_at(frame, pts, rad, attr, verts, sizes, 0), index),
        "composition": peak_extra(lambda: composition(frame, pts, rad, attr, verts, sizes), index),
        "fused_widen3": peak_extra(lambda: ops.point_attributes_at(frame, pts, rad, attr, verts, sizes, 3), index)}
    if "composition_widen3" in sides:
        res["peak_extra_bytes"]["composition_widen3"] = peak_extra(
            lambda: composition_widened(frame, pts, rad, attr, verts, sizes, 3), index)
    # compulsory traffic of the fused call: every query's position, size and output, its members' point, radius and attributes
    compulsory = m * (12 + 4 + 4 * c) + pairs * (16 + 4 + 4 * c)
    res["compulsory_bytes_per_query"] = round(compulsory / max(m, 1), 1)
    res["bytes_per_query_at_hbm_rate"] = round(res["ms_best"]["fused_widen0"] * 1e-3 * HBM_BYTES_PER_S / max(m, 1), 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
