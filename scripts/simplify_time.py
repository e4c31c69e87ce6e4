"""hip-event timing of the mesh simplification (asr_hip_mesh_simplify_count + _fill) on the mesh of the
seeded C3 cloud of bench.py: ImplicitPipeline.mesh() of the forward, then per k in --levels

  simplify_k<k>   ops.mesh_simplify with levels = max(0, leaf level - k), the per-vertex levels computed beforehand
                  (what ImplicitPipeline.mesh(simplify=k) runs after the component filter)
  levels_k<k>     ImplicitPipeline.simplify_levels alone (leaf_locate + the level arithmetic in torch), for scale

The sides alternate inside one process; per side the best of --reps after a warm-up and the spread (max / min - 1) of
those repetitions.  Both calls read sizes back, so a side's time includes those host round trips.  Prints one JSON
line with the input and output sizes.

    python scripts/simplify_time.py [--points 10000000] [--levels 1,2] [--reps 5]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "adaptive-surface-reconstruction_amd"), REPO]

from asr_hip import _lib, ops, synth  # noqa: E402
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
    ap.add_argument("--levels", default="1,2")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ks = [int(k) for k in args.levels.split(",")]
    dev = torch.device("cuda:0")
    pts, nrm = synth.scan_cloud(args.points, seed=0, device=dev)
    rad = synth.knn_radii_gpu(pts, 24)
    bb = synth.bounding_box(pts, 0.1)
    pipe = ImplicitPipeline(synth.make_weights(1, seed=2), device=dev)
    pipe.forward(pts, nrm, rad, bb[0], bb[1])
    verts, tris = pipe.mesh()
    del nrm, rad
    frame = _lib.frame_init(*bb)
    levels = {k: pipe.simplify_levels(verts, k) for k in ks}
    sides = {}
    for k in ks:
        sides["simplify_k%d" % k] = lambda k=k: ops.mesh_simplify(frame, verts, tris, levels=levels[k], ctx=pipe.ctx)
        sides["levels_k%d" % k] = lambda k=k: pipe.simplify_levels(verts, k)
    for fn in sides.values():  # warm-up: code objects, arena slabs, torch's allocator
        fn()
        torch.cuda.synchronize()
    ms = {name: [] for name in sides}
    for _ in range(args.reps):  # alternating
        for name, fn in sides.items():
            ms[name].append(once(fn))
    out = {}
    for k in ks:
        v, t = ops.mesh_simplify(frame, verts, tris, levels=levels[k], ctx=pipe.ctx)
        again = ops.mesh_simplify(frame, verts, tris, levels=levels[k], ctx=pipe.ctx)
        out["k%d" % k] = {"vertices": int(v.shape[0]), "triangles": int(t.shape[0]),
                          "same_bits_twice": bool(torch.equal(v.view(torch.int32), again[0].view(torch.int32)) and
                                                  torch.equal(t, again[1]))}
    res = {"points": args.points, "mesh_vertices": int(verts.shape[0]), "mesh_triangles": int(tris.shape[0]),
           "reps": args.reps, "output": out,
           "ms_best": {name: round(min(v), 3) for name, v in ms.items()},
           "spread": {name: round(max(v) / min(v) - 1, 4) for name, v in ms.items()}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
