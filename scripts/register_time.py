"""hip-event timing of the rigid registration on the seeded C3 cloud of bench.py, the cloud with its
normals as the target:

  nearest_near_1m / _10m  asr_hip_nearest_point with a jittered subset of the cloud / the whole jittered cloud as the
                  queries (half a point radius of noise): the yardstick, the same call as before the registration existed
  step_near_1m / _10m  asr_hip_icp_step, point-to-plane, identity transform, the same queries as the source: over the
                  yardstick it pays for the transform, the normals, the terms and the reduction
  step_point_near_1m  the same, point-to-point
  nearest_far_1m  asr_hip_nearest_point with --samples samples of the forward's mesh as the queries: the set of DESIGN.md
                  4.7 that lies far from the cloud (a seeded net's surface; the output says what it was and how far)
  step_far_1m     asr_hip_icp_step on that set with the same cap: most of the set still has a counterpart within it
  step_far_tight_1m  the same with a tenth of the cap, which most of the set lies beyond: the cap ends the search of a
                  source point without a counterpart at the first level whose cells are wider than the cap
  index_only      nearest_point with ONE query: the point index that every call above builds first
  driver          asr_hip_register_points on a subset of the cloud moved by the inverse of a 2 degree motion; the output
                  has its iterations, so (driver - index_only) / iterations is the cost of an iteration on a built index,
                  to be held against step_near_1m - index_only
  driver_noisy    the same on the jittered subset: the pairs of a noisy source keep changing, the updates settle at the
                  size the noise allows and the default tolerances may not be reached (the report says)

The cap is 5 % of the diagonal of the cloud's bounding box, the default of adaptivesurfacereconstruction.register_points.
The sides alternate inside one process; per side the best of --reps after a warm-up and the spread (max / min - 1) of
those repetitions, the only margin a comparison may use.  Prints one JSON line.

    python scripts/register_time.py [--points 10000000] [--samples 1000000] [--reps 5] [--no-forward]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
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


def small_motion(degrees, shift):
    """rotation about (0.3, 0.5, 0.8) by `degrees`, translation (shift, -shift/2, shift/3) -> f64 [3,4] and its inverse"""
    axis = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
    a = math.radians(degrees)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    r = np.eye(3) + math.sin(a) * k + (1 - math.cos(a)) * (k @ k)
    t = np.array([shift, -shift / 2, shift / 3])
    return np.hstack([r, t[:, None]]), np.hstack([r.T, -(r.T @ t)[:, None]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-forward", action="store_true", help="skip the network forward: the far set is uniform in the box")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pts, nrm = synth.scan_cloud(args.points, seed=0, device=dev)
    rad = synth.knn_radii_gpu(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    far, kind = None, "uniform_in_box"
    if not args.no_forward:
        from asr_hip.pipeline import ImplicitPipeline
        pipe = ImplicitPipeline(synth.make_weights(1, seed=2), device=dev)
        pipe.forward(pts, nrm, rad, bb[0], bb[1])
        verts, tris = pipe.mesh()
        del pipe
        torch.cuda.empty_cache()
        if verts.shape[0] >= 1000 and tris.shape[0] >= 1:
            far, kind = ops.mesh_sample(verts, tris, args.samples, seed=0), "mesh_samples"
    if far is None:
        lo, hi = (torch.as_tensor(b, dtype=torch.float32, device=dev) for b in bb)
        far = (lo + (hi - lo) * torch.rand((args.samples, 3), device=dev, generator=g)).contiguous()
    frame = _lib.frame_init(*bb)
    origin = ops.icp_origin(frame)
    cap = 0.05 * float(torch.linalg.norm((pts.max(0).values - pts.min(0).values).double()))
    identity = np.hstack([np.eye(3), np.zeros((3, 1))])
    pick = torch.randperm(args.points, device=dev, generator=g)[:args.samples]
    near = (pts[pick] + 0.5 * rad[pick, None] * torch.randn((pick.shape[0], 3), device=dev, generator=g)).contiguous()
    near_all = (pts + 0.5 * rad[:, None] * torch.randn((args.points, 3), device=dev, generator=g)).contiguous()
    motion, inverse = small_motion(2.0, 0.2 * cap)
    inv = torch.from_numpy(inverse).to(dev)
    moved = (pts[pick].double() @ inv[:, :3].T + inv[:, 3]).float().contiguous()
    moved_noisy = (near.double() @ inv[:, :3].T + inv[:, 3]).float().contiguous()
    first = pts[:1].contiguous()
    sides = {
        "nearest_near_1m": lambda: ops.nearest_point(frame, pts, near),
        "step_near_1m": lambda: ops.icp_step(frame, pts, nrm, near, identity, origin, cap),
        "step_point_near_1m": lambda: ops.icp_step(frame, pts, None, near, identity, origin, cap),
        "nearest_near_10m": lambda: ops.nearest_point(frame, pts, near_all),
        "step_near_10m": lambda: ops.icp_step(frame, pts, nrm, near_all, identity, origin, cap),
        "nearest_far_1m": lambda: ops.nearest_point(frame, pts, far),
        "step_far_1m": lambda: ops.icp_step(frame, pts, nrm, far, identity, origin, cap),
        "step_far_tight_1m": lambda: ops.icp_step(frame, pts, nrm, far, identity, origin, 0.1 * cap),
        "index_only": lambda: ops.nearest_point(frame, pts, first),
        "driver": lambda: ops.register_points(frame, pts, nrm, moved, cap),
        "driver_noisy": lambda: ops.register_points(frame, pts, nrm, moved_noisy, cap),
    }
    for fn in sides.values():  # warm-up: code objects, arena slabs, torch's allocator
        fn()
        torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(args.reps):  # alternating
        for k, fn in sides.items():
            ms[k].append(once(fn))
    best = {k: min(v) for k, v in ms.items()}
    transform, report = ops.register_points(frame, pts, nrm, moved, cap)
    noisy_transform, noisy_report = ops.register_points(frame, pts, nrm, moved_noisy, cap)
    far_sums = ops.icp_step(frame, pts, nrm, far, identity, origin, cap)
    tight_sums = ops.icp_step(frame, pts, nrm, far, identity, origin, 0.1 * cap)
    near_sums = ops.icp_step(frame, pts, nrm, near, identity, origin, cap)
    _, sq_far = ops.nearest_point(frame, pts, far)
    m, m_all = near.shape[0], near_all.shape[0]
    per = lambda k, count: round((best[k] - best["index_only"]) * 1e6 / count, 1)  # noqa: E731
    res = {"points": args.points, "m": m, "far_queries": kind, "reps": args.reps, "cap": cap,
           "ms_best": {k: round(v, 3) for k, v in best.items()},
           "spread": {k: round(max(v) / min(v) - 1, 4) for k, v in ms.items()},
           "ns_per_query_beyond_the_index": {"nearest_near_1m": per("nearest_near_1m", m), "step_near_1m": per("step_near_1m", m),
                                             "step_point_near_1m": per("step_point_near_1m", m),
                                             "nearest_near_10m": per("nearest_near_10m", m_all),
                                             "step_near_10m": per("step_near_10m", m_all),
                                             "nearest_far_1m": per("nearest_far_1m", far.shape[0]),
                                             "step_far_1m": per("step_far_1m", far.shape[0]),
                                             "step_far_tight_1m": per("step_far_tight_1m", far.shape[0])},
           "far_mean_distance": float(torch.sqrt(sq_far).double().mean()),
           "far_fitness": far_sums["pairs"] / far.shape[0], "far_tight_fitness": tight_sums["pairs"] / far.shape[0],
           "near_fitness": near_sums["pairs"] / m,
           "driver": dict(report, ms_per_iteration_beyond_the_index=round((best["driver"] - best["index_only"])
                                                                          / max(1, report["iterations"]), 3),
                          transform_error=float(np.abs(transform - motion).max())),
           "driver_noisy": dict(noisy_report, ms_per_iteration_beyond_the_index=round(
               (best["driver_noisy"] - best["index_only"]) / max(1, noisy_report["iterations"]), 3),
               transform_error=float(np.abs(noisy_transform - motion).max()))}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
