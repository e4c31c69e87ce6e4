"""hip-event timing of the normal estimation (asr_hip_knn_index, asr_hip_point_normals, asr_hip_normals_orient, DESIGN.md
4.15) on the seeded C3 cloud of bench.py, in the margin frame estimate_normals uses.  Sides, alternating inside one
process:

  knn_radius        ops.knn_radius(k): the same index and level walk without the lists (the yardstick of knn_index)
  knn_index         ops.knn_index(k)
  point_normals     ops.point_normals over those lists, with eigenvalues and ok
  orient_propagate  ops.orient_normals over those lists and normals (Boruvka rounds; the number of rounds is reported)
  orient_viewpoint  ops.orient_normals towards one viewpoint above the scene

Per side the median and the best of --reps after a warm-up and the spread (max / min - 1).  Every side but
orient_viewpoint reads flags back, so its time includes those host round trips.  Prints one JSON line.

    python scripts/normals_time.py [--points 10000000] [--k 16] [--reps 5] [--sides knn_radius,knn_index]

--sides restricts the sides: under `rocprofv3 --kernel-trace --stats` with one side the trace holds that side's kernels
(and the set-up's: the lists and normals the later sides read are always computed once).
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "adaptive-surface-reconstruction_amd"), REPO]

from asr_hip import _lib, ops, synth  # noqa: E402

SIDES = "knn_radius,knn_index,point_normals,orient_propagate,orient_viewpoint"


def once(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sides", default=SIDES)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pts, true_normals = synth.scan_cloud(args.points, seed=0, device=dev)
    n, k = pts.shape[0], args.k
    lo, hi = pts.min(0).values.cpu().numpy(), pts.max(0).values.cpu().numpy()
    margin = max(1e-3, 1e-3 * float((hi - lo).max()))
    frame = _lib.frame_init(lo - margin, hi + margin)
    index, _ = ops.knn_index(frame, pts, k)
    normals, ok = ops.point_normals(pts, index, return_ok=True)
    view = torch.tensor([0.0, 0.0, float(hi[2]) + 10.0], device=dev)
    oriented, report = ops.orient_normals(pts, normals, index, return_report=True)
    sides = {
        "knn_radius": lambda: ops.knn_radius(frame, pts, k),
        "knn_index": lambda: ops.knn_index(frame, pts, k),
        "point_normals": lambda: ops.point_normals(pts, index, return_eigenvalues=True, return_ok=True),
        "orient_propagate": lambda: ops.orient_normals(pts, normals, index),
        "orient_viewpoint": lambda: ops.orient_normals(pts, normals, viewpoints=view),
    }
    sides = {name: sides[name] for name in args.sides.split(",")}
    for fn in sides.values():  # warm-up: code objects, arena slabs, torch's allocator
        fn()
        torch.cuda.synchronize()
    ms = {name: [] for name in sides}
    for _ in range(args.reps):  # alternating
        for name, fn in sides.items():
            ms[name].append(once(fn))
    again, _ = ops.knn_index(frame, pts, k)
    # how the estimate compares with the normals the synthetic scan knows (not a check: a description of the cloud)
    dot = (oriented * true_normals).sum(1)[ok]
    res = {"points": n, "k": k, "reps": args.reps, "report": report, "ok": int(ok.sum()),
           "same_lists_twice": bool(torch.equal(again, index)),
           "agrees_with_scan_normals": round(float((dot > 0).float().mean()), 4),
           "ms_median": {name: round(statistics.median(v), 3) for name, v in ms.items()},
           "ms_best": {name: round(min(v), 3) for name, v in ms.items()},
           "spread": {name: round(max(v) / min(v) - 1, 4) for name, v in ms.items()}}
    if "knn_index" in ms and "knn_radius" in ms:
        res["knn_index_over_knn_radius"] = round(statistics.median(ms["knn_index"]) / statistics.median(ms["knn_radius"]), 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
