"""hip-event timing of the three entry points of the global registration on the seeded C3 cloud of
bench.py: the cloud merged to about 50 k and about 200 k points is the target, a DIFFERENT merge of it (the same level in a
frame whose cells lie elsewhere), moved by 140 degrees, the source.

  point_fpfh        asr_hip_point_fpfh on the target with the lists of knn_index(k) (the lists are not timed)
  feature_match     asr_hip_feature_match source -> target on the 33-bin descriptors; priced against the vector-f32 rate it
                    needs: m n dim 3 operations (a subtraction, a product, a sum per entry, none of them fused)
  ransac_transform  asr_hip_ransac_transform on the mutual matches, --hypotheses hypotheses, cap = 1.5 cells

Per entry point the median of --reps after a warm-up and the spread (max / min - 1) of those repetitions.  Also prints what
the search found (the angle between its rotation and the true one).  One JSON line.

    python scripts/global_register_time.py [--points 10000000] [--sizes 50000,200000] [--k 48] [--hypotheses 100000] [--reps 5]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "adaptive-surface-reconstruction_amd"), REPO]

from asr_hip import _lib, ops, synth  # noqa: E402

F32_OPS_PER_SECOND = 256 * 4 * 16 * 2.4e9  # one unfused, unpacked f32 operation per lane and clock: 39.3 T/s


def once(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def motion(degrees, d):
    axis = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
    a = math.radians(degrees)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    r = np.eye(3) + math.sin(a) * k + (1 - math.cos(a)) * (k @ k)
    t = np.array([d, -d / 2, d / 3])
    return np.hstack([r, t[:, None]]), np.hstack([r.T, -(r.T @ t)[:, None]])


def merged(frame, pts, nrm, want):
    """the merge whose number of clusters is closest to `want` -> (points, normals, level)"""
    best = None
    for level in range(3, 13):
        p, n, _, _ = ops.points_merge(frame, pts, nrm, level=level, split_sides=True)
        if best is None or abs(p.shape[0] - want) < abs(best[0].shape[0] - want):
            best = (p, n, level)
        if p.shape[0] > want:
            break
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--sizes", default="50000,200000")
    ap.add_argument("--k", type=int, default=48)
    ap.add_argument("--hypotheses", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pts, nrm = synth.scan_cloud(args.points, seed=0, device=dev)
    lo, hi = synth.bounding_box(pts, 0.1)
    frame = _lib.frame_init(lo, hi)
    shift = 0.37 * (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)).max() / 64  # the other merge's cells lie elsewhere
    other = _lib.frame_init(np.asarray(lo, np.float32) - np.float32(shift), np.asarray(hi, np.float32) + np.float32(0.21 * shift))
    truth, inverse = motion(140.0, 1.0)
    inv = torch.from_numpy(inverse).to(dev)
    out = {"points": args.points, "k": args.k, "hypotheses": args.hypotheses, "reps": args.reps, "sizes": {}}
    for want in (int(s) for s in args.sizes.split(",")):
        tp, tn, level = merged(frame, pts, nrm, want)
        sp, sn, _ = ops.points_merge(other, pts, nrm, level=level, split_sides=True)[:3]
        sp = (sp.double() @ inv[:, :3].T + inv[:, 3]).float().contiguous()
        sn = (sn.double() @ inv[:, :3].T).float().contiguous()
        cell = float(frame.voxel_size[level])
        t_frame = _lib.frame_init(*synth.bounding_box(tp, 0.01))
        s_frame = _lib.frame_init(*synth.bounding_box(sp, 0.01))
        t_index, _ = ops.knn_index(t_frame, tp, args.k)
        s_index, _ = ops.knn_index(s_frame, sp, args.k)
        tf, t_ok = ops.point_fpfh(tp, tn, t_index, return_ok=True)
        sf, s_ok = ops.point_fpfh(sp, sn, s_index, return_ok=True)
        forth = ops.feature_match(sf, tf)[0].cpu().numpy()
        back = ops.feature_match(tf, sf)[0].cpu().numpy()
        rows = np.nonzero(forth >= 0)[0]
        corr = np.stack([rows, forth[rows]], 1).astype(np.int32)
        corr = corr[back[corr[:, 1]] == corr[:, 0]]
        corr_dev = torch.from_numpy(np.ascontiguousarray(corr)).to(dev)
        sides = {
            "point_fpfh": lambda: ops.point_fpfh(tp, tn, t_index),
            "feature_match": lambda: ops.feature_match(sf, tf),
            "ransac_transform": lambda: ops.ransac_transform(sp, tp, corr_dev, 1.5 * cell, 0.9, args.hypotheses, 0),
        }
        for fn in sides.values():  # warm-up: code objects, arena slabs, torch's allocator
            fn()
            torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        for _ in range(args.reps):  # alternating
            for k, fn in sides.items():
                ms[k].append(once(fn))
        transform, report = ops.ransac_transform(sp, tp, corr_dev, 1.5 * cell, 0.9, args.hypotheses, 0)
        angle = None
        if transform is not None:
            r = transform[:, :3] @ truth[:, :3].T
            angle = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(r) - 1.0) / 2.0))))
        median = {k: statistics.median(v) for k, v in ms.items()}
        operations = float(sf.shape[0]) * float(tf.shape[0]) * 33 * 3
        out["sizes"][str(want)] = {
            "target": int(tp.shape[0]), "source": int(sp.shape[0]), "level": level, "cell": cell,
            "descriptors_ok": [int(s_ok.sum()), int(t_ok.sum())], "mutual_matches": int(len(corr)),
            "ms_median": {k: round(v, 3) for k, v in median.items()},
            "spread": {k: round(max(v) / min(v) - 1, 4) for k, v in ms.items()},
            "fpfh_ns_per_point": round(median["point_fpfh"] * 1e6 / tp.shape[0], 1),
            "match_operations": operations,
            "match_operations_per_second": operations / (median["feature_match"] * 1e-3),
            "match_share_of_the_unfused_f32_rate": round(operations / (median["feature_match"] * 1e-3) / F32_OPS_PER_SECOND, 3),
            "ransac": dict(report, degrees_from_the_truth=angle),
        }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
