"""hip-event timing of the point merge (asr_hip_points_merge_count + _fill) on the seeded C3 cloud of
bench.py with its 24-NN radii and three attribute channels, at the octree level of the cloud's margin frame whose cells
come closest to halving the cloud.  Sides, alternating inside one process:

  merge         ops.points_merge(points, normals, radii, attributes, level=L) with map and counts: count + fill
  merge_split   the same with split_sides=True
  count         asr_hip_points_merge_count alone (keys, sort, heads, scan, one read-back), its fill with every output NULL
  torch         the same result composed from torch operators: cell keys from the frame arithmetic, torch.unique(keys,
                return_inverse=True, return_counts=True), f64 index_add_ of the ten columns, divisions, casts

Per side the median and the best of --reps after a warm-up and the spread (max / min - 1).  Every side reads sizes back,
so its time includes those host round trips.  Prints one JSON line; "agree" compares the two results (counts equal,
largest difference of a mean in f32 ulps of the larger value).

    python scripts/merge_time.py [--points 10000000] [--reps 7] [--level L] [--sides merge,torch]

--level skips the search for the halving level and --sides restricts the sides: under `rocprofv3 --kernel-trace --stats`
with one side and a fixed level the trace holds that side's kernels only, each launched 2 + reps + 2 times after the set-up.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "adaptive-surface-reconstruction_amd"), REPO]

from asr_hip import _lib, ops, synth  # noqa: E402


def once(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def torch_merge(frame, level, pts, nrm, rad, att):
    """one point per cell of `level` with torch operators; clusters in ascending (x, y, z) cell order"""
    inv, shift = float(frame.inv_voxel_size[21]), 21 - level
    off = torch.tensor(list(frame.offset), dtype=torch.int64, device=pts.device)
    cell = (torch.floor(pts * inv).to(torch.int64) + off) >> shift
    keys = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    ukeys, inverse, counts = torch.unique(keys, return_inverse=True, return_counts=True)
    cols = torch.cat([pts, nrm, rad[:, None], att], 1).to(torch.float64)
    sums = torch.zeros((ukeys.shape[0], cols.shape[1]), dtype=torch.float64, device=pts.device)
    sums.index_add_(0, inverse, cols)
    mean = sums / counts[:, None]
    normal = sums[:, 3:6] / torch.sqrt((sums[:, 3:6] ** 2).sum(1, keepdim=True))
    return (mean[:, 0:3].float(), normal.float(), mean[:, 6].float(), mean[:, 7:].float(), counts.to(torch.int32), ukeys)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--level", type=int, default=None)
    ap.add_argument("--sides", default="merge,merge_split,count,torch")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pts, nrm = synth.scan_cloud(args.points, seed=0, device=dev)
    n = pts.shape[0]
    rad = synth.knn_radii_gpu(pts, 24)
    att = torch.rand((n, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 255.0
    lo, hi = pts.min(0).values.cpu().numpy(), pts.max(0).values.cpu().numpy()
    margin = max(1e-3, 1e-3 * float((hi - lo).max()))
    frame = _lib.frame_init(lo - margin, hi + margin)
    ctx = ops.context(dev)
    clusters = {}
    for level in range(4, 17) if args.level is None else ():
        clusters[level] = ops.points_merge(frame, pts, level=level, return_report=True)[4]["clusters"]
        if clusters[level] > 0.75 * n:
            break
    level = min(clusters, key=lambda l: abs(clusters[l] - 0.5 * n)) if args.level is None else args.level

    def count_only():
        m = ctypes.c_int64(0)
        ctx.call("asr_hip_points_merge_count", ctypes.byref(frame), _lib.ptr(pts), ctypes.c_int64(n), _lib.ptr(nrm),
                 _lib.ptr(rad), _lib.ptr(att), 3, None, level, 0, ctypes.byref(m), None)
        ctx.call("asr_hip_points_merge_fill", None, None, None, None, None, None)

    sides = {
        "merge": lambda: ops.points_merge(frame, pts, nrm, rad, att, level=level, return_map=True, return_counts=True),
        "merge_split": lambda: ops.points_merge(frame, pts, nrm, rad, att, level=level, split_sides=True, return_map=True,
                                                return_counts=True),
        "count": count_only,
        "torch": lambda: torch_merge(frame, level, pts, nrm, rad, att),
    }
    sides = {name: sides[name] for name in args.sides.split(",")}
    for fn in sides.values():  # warm-up: code objects, arena slabs, torch's allocator
        fn()
        torch.cuda.synchronize()
    ms = {name: [] for name in sides}
    for _ in range(args.reps):  # alternating
        for name, fn in sides.items():
            ms[name].append(once(fn))
    a = ops.points_merge(frame, pts, nrm, rad, att, level=level, return_counts=True, return_report=True)
    b = ops.points_merge(frame, pts, nrm, rad, att, level=level, return_counts=True, return_report=True)
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[:5], b[:5]))
    t = torch_merge(frame, level, pts, nrm, rad, att)
    # the two cluster orders differ (location code / cell triple): compare through a sort of each side on its cell triple
    cell = (torch.floor(a[0] * float(frame.inv_voxel_size[21])).to(torch.int64)
            + torch.tensor(list(frame.offset), dtype=torch.int64, device=dev)) >> (21 - level)
    order = torch.argsort((cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2])
    agree = {"clusters": [int(a[0].shape[0]), int(t[0].shape[0])]}
    if a[0].shape[0] == t[0].shape[0]:
        agree["counts_equal"] = bool(torch.equal(a[4][order], t[4]))
        for name, x, y in (("points", a[0], t[0]), ("radii", a[2], t[2]), ("attributes", a[3], t[3])):
            x, y = x[order].double(), y.double()
            ulp = torch.maximum(x.abs(), y.abs()) * 2.0 ** -23
            agree[name + "_max_ulp"] = round(float(((x - y).abs() / ulp.clamp_min(1e-300)).max()), 3)
    report = a[5]
    res = {"points": n, "level": level, "cell_size": float(frame.voxel_size[level]), "clusters_per_level": clusters,
           "report": report, "reps": args.reps, "same_bits_twice": bool(same), "agree": agree,
           "ms_median": {name: round(statistics.median(v), 3) for name, v in ms.items()},
           "ms_best": {name: round(min(v), 3) for name, v in ms.items()},
           "spread": {name: round(max(v) / min(v) - 1, 4) for name, v in ms.items()}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
