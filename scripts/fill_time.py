"""hip-event timing of hole filling on the mesh of the seeded C3 cloud of bench.py:
ImplicitPipeline.mesh() of the forward, then

  topology      ops.mesh_topology: the yardstick -- it builds the same edge table and the same boundary forest, counts and
                reads back once
  fill          ops.mesh_fill_holes(max_edges): edge table, boundary forest, degrees, rim statistics, selection and three
                scans, the key sort over the vertices, one read-back; then the two output allocations, the copies of the
                input arrays, hubs and fans
  fill_none     the same with max_edges = 3: (nearly) nothing is filled, what is left is the analysis and the copies

Whole calls between two events, the allocation of the outputs included.  The sides alternate inside one process; per
side the best of --reps after a warm-up and the spread (max / min - 1).  Prints one JSON line with the report's counts
and the topology before and after.

    python scripts/fill_time.py [--points 10000000] [--reps 5] [--max-edges 64]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "adaptive-surface-reconstruction_amd"), REPO]

from asr_hip import ops, synth  # noqa: E402
from asr_hip.pipeline import ImplicitPipeline  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-edges", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pts, nrm = synth.scan_cloud(args.points, seed=0, device=dev)
    rad = synth.knn_radii_gpu(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    pipe = ImplicitPipeline(synth.make_weights(1, seed=2), device=dev)
    pipe.forward(pts, nrm, rad, bb[0], bb[1])
    verts, tris = pipe.mesh()
    del pts, nrm, rad
    ctx = pipe.ctx
    nv = int(verts.shape[0])
    sides = {"topology": lambda: ops.mesh_topology(tris, nv, ctx=ctx),
             "fill": lambda: ops.mesh_fill_holes(verts, tris, args.max_edges, ctx=ctx),
             "fill_none": lambda: ops.mesh_fill_holes(verts, tris, 3, ctx=ctx)}
    for fn in sides.values():  # warm-up: code objects, arena slabs, torch's allocator
        fn()
        torch.cuda.synchronize()
    ms = {name: [] for name in sides}
    for _ in range(args.reps):  # alternating
        for name, fn in sides.items():
            ms[name].append(once(fn))
    best = {name: min(v) for name, v in ms.items()}
    a = ops.mesh_fill_holes(verts, tris, args.max_edges, return_report=True, ctx=ctx)
    b = ops.mesh_fill_holes(verts, tris, args.max_edges, ctx=ctx)
    res = {"points": args.points, "mesh_vertices": nv, "mesh_triangles": int(tris.shape[0]), "max_edges": args.max_edges,
           "report": a[2], "report_max_edges_3": ops.mesh_fill_holes(verts, tris, 3, return_report=True, ctx=ctx)[2],
           "topology_before": ops.mesh_topology(tris, nv, ctx=ctx),
           "topology_after": ops.mesh_topology(a[1], int(a[0].shape[0]), ctx=ctx), "reps": args.reps,
           "same_bits_twice": bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])),
           "ms_best": {name: round(v, 3) for name, v in best.items()},
           "spread": {name: round(max(v) / min(v) - 1, 4) for name, v in ms.items()},
           "fill_over_topology": round(best["fill"] / best["topology"], 3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
