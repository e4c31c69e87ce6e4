"""hip-event timing of the mesh adjacency entry points on the mesh of the seeded C3 cloud of bench.py:
ImplicitPipeline.mesh() of the forward, then

  edges         ops.mesh_edges (asr_hip_mesh_edges_count + _fill: side keys, sort, runs, the three output arrays)
  topology      ops.mesh_topology (the edge table, the fused counts, two union-find runs, one read-back)
  smooth_1      ops.mesh_smooth, 1 iteration with mu = 0: edge table + vertex -> neighbour rows + check pass + ONE step
  smooth_21     the same with 21 iterations: 21 steps
  torch_20      20 steps of the composition a user of the parent commit can write on the same GPU: index_add_ of the f64
                positions over the directed edge list (built beforehand, not timed), divide by the degree, update

  free_1/_21    smooth_1 / smooth_21 with boundary "free", the mode the torch composition computes (when --boundary differs)

and, derived (ms):  step = (smooth_21 - smooth_1) / 20;  csr_build = smooth_1 - step - edges (what smoothing builds on top
of the edge table: the neighbour rows, the long-row list, the f64 positions and their check; `edges` also writes three
output arrays smoothing does not need, so this is a lower estimate).

bytes_per_step is ALGORITHMIC, not counter-measured: V (24 read + 24 written + 8 row split + 1 feature flag) +
2 E (4 entry + 24 gathered position), as if no gathered position came from a cache; gb_per_s = bytes_per_step / step.

The sides alternate inside one process; per side the best of --reps after a warm-up and the spread (max / min - 1).
Prints one JSON line.

    python scripts/smooth_time.py [--points 10000000] [--reps 5] [--boundary along]
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
    ap.add_argument("--boundary", default="along")
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
    edges, uses, _ = ops.mesh_edges(tris, nv, ctx=ctx)
    ne = int(edges.shape[0])
    topo = ops.mesh_topology(tris, nv, ctx=ctx)
    # the torch composition: directed edge list and degrees, built outside the timed region
    src = torch.cat([edges[:, 0], edges[:, 1]]).long()
    dst = torch.cat([edges[:, 1], edges[:, 0]]).long()
    deg = torch.bincount(src, minlength=nv)
    degf = deg.clamp(min=1).to(torch.float64)[:, None]
    moves = (deg > 0)[:, None]
    p64 = verts.to(torch.float64)
    del edges, uses

    def torch_steps(n, f=0.5):
        p = p64
        for _ in range(n):
            acc = torch.zeros_like(p)
            acc.index_add_(0, src, p[dst])
            p = torch.where(moves, p + f * (acc / degf - p), p)
        return p

    def smooth(n, boundary=args.boundary):
        return ops.mesh_smooth(verts, tris, iterations=n, mu=0.0, boundary=boundary, ctx=ctx)

    sides = {"edges": lambda: ops.mesh_edges(tris, nv, ctx=ctx), "topology": lambda: ops.mesh_topology(tris, nv, ctx=ctx),
             "torch_20": lambda: torch_steps(20)}
    sides["smooth_1"] = lambda: smooth(1)
    sides["smooth_21"] = lambda: smooth(21)
    if args.boundary != "free":  # what the torch composition computes: every vertex uses all of its neighbours
        sides["free_1"] = lambda: smooth(1, "free")
        sides["free_21"] = lambda: smooth(21, "free")
    for fn in sides.values():  # warm-up: code objects, arena slabs, torch's allocator
        fn()
        torch.cuda.synchronize()
    ms = {name: [] for name in sides}
    for _ in range(args.reps):  # alternating
        for name, fn in sides.items():
            ms[name].append(once(fn))
    best = {name: min(v) for name, v in ms.items()}
    a, b = smooth(3), smooth(3)
    free = smooth(20, "free")
    bytes_per_step = nv * (24 + 24 + 8 + 1) + 2 * ne * (4 + 24)
    step = (best["smooth_21"] - best["smooth_1"]) / 20
    derived = {"torch_step": best["torch_20"] / 20, "step": step, "csr_build": best["smooth_1"] - step - best["edges"],
               "gb_per_s": bytes_per_step / step / 1e6}
    if args.boundary != "free":
        derived["free_step"] = (best["free_21"] - best["free_1"]) / 20
    res = {"points": args.points, "mesh_vertices": nv, "mesh_triangles": int(tris.shape[0]), "mesh_edges": ne,
           "max_row": int(deg.max()), "rows_over_128": int((deg > 128).sum()), "boundary": args.boundary,
           "topology": topo, "reps": args.reps, "bytes_per_step_algorithmic": bytes_per_step,
           "same_bits_twice": bool(torch.equal(a.view(torch.int32), b.view(torch.int32))),
           "torch_vs_hip_max_abs_diff_free_20": float((torch_steps(20).to(torch.float32) - free).abs().max()),
           "ms_best": {name: round(v, 3) for name, v in best.items()},
           "spread": {name: round(max(v) / min(v) - 1, 4) for name, v in ms.items()},
           "derived": {name: round(v, 4) for name, v in derived.items()}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
