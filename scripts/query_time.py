"""hip-event timing of asr_hip_implicit_query (ImplicitPipeline.query) on the seeded C3 cloud of bench.py: one forward,
then three query sets, each without and with the gradient -- the V0 grid-0 centres, the input points and as many
uniform random points in the bounding box.  Prints one JSON line.

    python scripts/query_time.py [--points 10000000] [--reps 5]

For the kernel breakdown run it under `rocprofv3 --kernel-trace --stats -- python scripts/query_time.py --reps 2`.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "adaptive-surface-reconstruction_amd"), REPO]

from asr_hip import synth  # noqa: E402
from asr_hip._lib import ptr  # noqa: E402
from asr_hip.pipeline import ImplicitPipeline  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        start.record()
        fn()
        end.record()
        end.synchronize()
        best = min(best, start.elapsed_time(end))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pts, nrm = synth.scan_cloud(args.points, seed=0, device=dev)
    rad = synth.knn_radii_gpu(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    pipe = ImplicitPipeline(synth.make_weights(1, seed=2), device=dev)
    pipe.forward(pts, nrm, rad, bb[0], bb[1])
    torch.cuda.synchronize()
    stage = pipe.stage_ms()
    centres = pipe.get("voxel_centers0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    lo, hi = torch.tensor(bb[0], device=dev), torch.tensor(bb[1], device=dev)
    rand = (lo + (hi - lo) * torch.rand((args.points, 3), device=dev, generator=g)).contiguous()
    out = {"points": args.points, "v0": int(centres.shape[0]), "forward_decode_ms": stage["decode"], "ms": {}}
    for name, q in (("centres", centres), ("input_points", pts), ("random_in_bbox", rand)):
        m = q.shape[0]
        values = torch.empty((m, 2), device=dev)
        grad = torch.empty((m, 3), device=dev)
        for with_grad in (False, True):
            # the context call alone (no per-call allocation): the same entry point ImplicitPipeline.query uses
            args_c = (ptr(q), ctypes.c_int64(m), pipe._table, len(pipe._weights), ptr(values),
                      ptr(grad if with_grad else None), ctypes.c_void_p(0))
            ms = timed(lambda: pipe.ctx.call("asr_hip_implicit_query", *args_c), args.reps)
            out["ms"]["%s%s" % (name, "_grad" if with_grad else "")] = round(ms, 3)
        out["inside_%s" % name] = float(torch.isfinite(values[:, 0]).float().mean())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
