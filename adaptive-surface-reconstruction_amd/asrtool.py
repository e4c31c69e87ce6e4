"""`asrtool` for the MI355X path: point cloud PLY in, triangle mesh PLY out -- the command line of the
reference (cpp/bin/main.cpp:114-177: `asrtool --in point_cloud.ply --out mesh.ply`, `--version`,
`--third-party-notices`) on top of adaptivesurfacereconstruction.reconstruct_surface.

    python adaptive-surface-reconstruction_amd/asrtool.py --in scan.ply --out mesh.ply [--weights model.pt] [--precision NAME]
                                                          [--normals] [--colors] [--simplify K] [--smooth N] [--fill-holes N]
                                                          [--thin SIZE] [--estimate-normals K [--viewpoint x,y,z]]
    python adaptive-surface-reconstruction_amd/asrtool.py --thin-cloud scan.ply out.ply --cell SIZE
    python adaptive-surface-reconstruction_amd/asrtool.py --orient-cloud raw.ply out.ply [--k K] [--viewpoint x,y,z]
    python adaptive-surface-reconstruction_amd/asrtool.py --register source.ply target.ply out.ply [--max-distance D] [--iterations N] [--point-to-point]
    python adaptive-surface-reconstruction_amd/asrtool.py --register source.ply target.ply out.ply --global [--voxel S] [--hypotheses N] [--seed K] [--max-distance D]
    python adaptive-surface-reconstruction_amd/asrtool.py --compare mesh.ply reference.ply [--samples N] [--thresholds a,b,...] [--seed S]
    python adaptive-surface-reconstruction_amd/asrtool.py --decimate mesh.ply out.ply --cell SIZE
    python adaptive-surface-reconstruction_amd/asrtool.py --smooth-mesh mesh.ply out.ply [--iterations N] [--boundary free|pinned|along]
    python adaptive-surface-reconstruction_amd/asrtool.py --fill-mesh mesh.ply out.ply --max-edges N
    python adaptive-surface-reconstruction_amd/asrtool.py --topology mesh.ply

The reference bundles its network as <resource dir>/model.pt (cpp/lib/asr.cpp:138-139); here the weights come
from --weights (a TorchScript archive with the same tensor names, a pickled state dict or an .npz) or from
$ASR_RESOURCE_DIR/{model_weights.npz, model_weights.pt, model.pt}.
"""
import os
import sys

HELP = """usage: asrtool --in point_cloud.ply --out mesh.ply

Arguments:
    in      Input point cloud with normal information in PLY format.
    out     Output mesh in PLY format.

Options:
    --weights FILE  Network weights (TorchScript model.pt, state dict .pt or .npz); default $ASR_RESOURCE_DIR
    --precision NAME  Arithmetic of the network's sparse convolutions: f32 (default), bf16x3_2acc, bf16x3, f16x2, f16
    --normals  Writes per-vertex normals (nx ny nz): the unit gradient of the network's field at each vertex
    --colors  Carries the input's point colours (red green blue) onto the mesh vertices, blended at each vertex's own scale
    --simplify K  Merges the mesh vertices inside one octree cell K levels above the leaf that contains them (1 <= K <= 21);
              normals and colours then describe the simplified vertices
    --smooth N  Taubin smoothing of the mesh, N iterations (1 <= N <= 1000), after --simplify; normals and colours then
              describe the smoothed vertices
    --fill-holes N  Closes every simple boundary rim of at most N edges (3 <= N <= 1048576) with a fan around the mean of its
              vertices, after --simplify and before --smooth; longer rims, the outer border of an open scan among them, stay open
    --thin SIZE  Merges the input points inside one cell of a regular grid (and on one side of it: normals that point against
              each other stay apart) into their mean before anything else.  The cell used is the voxel size of the octree
              level around the cloud that is >= SIZE and < 2 SIZE.  Radii and colours are averaged with the points
    --estimate-normals K  For scans without (oriented) normals: estimates them from the K nearest neighbours of each point
              (3 <= K <= 64; PCA plane, signs propagated along the minimum spanning forest of the neighbour graph), after
              --thin.  Normals in the file are then ignored; points without a usable estimate are dropped
    --viewpoint x,y,z  --estimate-normals / --orient-cloud: turns every normal towards this position (the scanner's)
              instead of propagating the signs
    --orient-cloud IN.ply OUT.ply [--k K]  Instead of reconstructing: writes the cloud with normals estimated as
              --estimate-normals K does (default 16), radii and colours carried over unchanged, points without a usable
              estimate dropped; prints one JSON line with the report (components, flipped, skipped, rounds, points, dropped)
    --register SOURCE.ply TARGET.ply OUT.ply  Instead of reconstructing: aligns SOURCE to TARGET by ICP (a local method: the
              two scans must overlap and be roughly aligned already) and writes the moved SOURCE, its normals rotated (zero
              ones when it has none), radii and colours carried over unchanged; prints one JSON line with the report
              (fitness, rmse, iterations, converged, degenerate, pairs, mode) and the 4x4 transform.  Point-to-plane when
              TARGET has normals, else point-to-point (said on stderr)
    --max-distance D  --register: pairs further apart than D are ignored (default: 5 % of TARGET's bounding-box diagonal)
    --iterations N  --register: at most N iterations (default 50, 1 <= N <= 1000)
    --point-to-point  --register: ignores TARGET's normals
    --global  --register: for scans that are NOT roughly aligned: first searches the pose by FPFH descriptors and RANSAC on
              both clouds thinned to --voxel, then refines it by ICP with its defaults; the JSON line gains "global"
              (cell_size, correspondences, mutual_used, normals_flipped, evaluated, best_hypothesis, inliers and RANSAC's
              transform).  Normals of the files are used where present, else estimated (the search then also runs with
              SOURCE's negated and keeps the better pose).  Does not resolve near-symmetric shapes
    --voxel S  --register --global: cell of the thinning (default: 1.5 % of TARGET's bounding-box diagonal);
              --max-distance D is then RANSAC's inlier distance (default: 1.5 x the cell used)
    --hypotheses N  --register --global: RANSAC hypotheses (default 100000, 1 <= N <= 16777216)
    --seed K  --register --global: seed of the draws (default 0); the result is a function of the inputs and K alone
    --thin-cloud IN.ply OUT.ply --cell SIZE  Instead of reconstructing: writes the cloud merged as --thin SIZE does, with its
              normals and, where the input has them, radii and colours; prints the cell size used
    --fill-mesh MESH.ply OUT.ply --max-edges N  Instead of reconstructing: closes the holes of at most N edges of an existing
              mesh and prints one JSON line with the counts (rims, filled, too_long, not_simple, new_vertices, new_triangles).
              Each new hub vertex gets the mean of the normals and colours of its rim
    --smooth-mesh MESH.ply OUT.ply  Instead of reconstructing: Taubin smoothing of an existing mesh (lambda 0.5, mu -0.53).
              Vertex normals and colours are carried over unchanged
    --iterations N  --smooth-mesh: iterations (default 10, 0 <= N <= 1000)
    --boundary MODE  --smooth-mesh: what the vertices of open rims and non-manifold seams do: free (move like all others),
              pinned (stay) or along (move along their own rim or seam only; default)
    --topology MESH.ply  Instead of reconstructing: prints one JSON line with the mesh's vertex, triangle and edge counts,
              boundary / non-manifold / inconsistently oriented edges, components, boundary loops, Euler characteristic,
              and whether it is edge manifold, oriented and watertight (then also its genus)
    --decimate MESH.ply OUT.ply --cell SIZE  Instead of reconstructing: simplifies an existing mesh by merging the vertices
              inside one cell of a regular grid.  The cell used is the voxel size of the octree level around the mesh that is
              >= SIZE and < 2 SIZE (printed).  Vertex colours are averaged per merged vertex, normals are dropped
    --compare MESH.ply REFERENCE.ply  Instead of reconstructing: prints one JSON line with the distance between the mesh
              and the reference (accuracy, completeness, Chamfer, Hausdorff, precision / recall / F-score, normal consistency).
              A REFERENCE with faces is a mesh; without faces it is a point cloud (nx ny nz are used if present)
    --samples N  --compare: points sampled on each mesh (default 1000000)
    --thresholds a,b,...  --compare: F-score distances (default: 0.5 % and 1 % of the reference's bounding-box diagonal)
    --seed S  --compare: seed of the sampling (default 0)
    --version  Prints the version information
    --third-party-notices  Prints third-party software notices
"""


def _option(argv, name):
    """value following `name` (Open3D's GetProgramOptionAsString, main.cpp:150-153) or None"""
    if name in argv:
        i = argv.index(name)
        if i + 1 < len(argv):
            return argv[i + 1]
    return None


def _compare(argv):
    """--compare MESH.ply REFERENCE.ply: one JSON line, 0; a message on stderr and 1 when something is wrong"""
    import json
    i = argv.index("--compare")
    paths = argv[i + 1:i + 3]
    if len(paths) < 2 or any(p.startswith("--") for p in paths):
        sys.stderr.write("asrtool: --compare needs two files: MESH.ply REFERENCE.ply\n")
        return 1
    for p in paths:
        if not os.path.isfile(p):
            sys.stderr.write("asrtool: --compare: no such file: %s\n" % p)
            return 1
    try:
        samples = int(_option(argv, "--samples") or 1000000)
        seed = int(_option(argv, "--seed") or 0)
        thresholds = _option(argv, "--thresholds")
        thresholds = None if thresholds is None else tuple(float(t) for t in thresholds.split(","))
        if samples < 1 or seed < 0 or (thresholds is not None and not all(t > 0 for t in thresholds)):
            raise ValueError("out of range")
    except ValueError:
        sys.stderr.write("asrtool: --compare: --samples and --seed take integers (N >= 1, S >= 0), --thresholds positive numbers a,b,...\n")
        return 1
    from asr_hip import ply
    try:
        v, t, _ = ply.read_surface(paths[0])
        rv, rt, rn = ply.read_surface(paths[1])
    except (ValueError, IndexError, OSError) as e:
        sys.stderr.write("asrtool: --compare: %s\n" % e)
        return 1
    if t is None:
        sys.stderr.write("asrtool: --compare: %s has no faces (the first file must be a mesh)\n" % paths[0])
        return 1
    import adaptivesurfacereconstruction as asr
    ref = {"reference_mesh": (rv, rt)} if rt is not None else {"reference_points": rv, "reference_normals": rn}
    result = asr.evaluate_mesh(v, t, num_samples=samples, thresholds=thresholds, seed=seed, **ref)
    print(json.dumps(result))
    return 0


def _decimate(argv):
    """--decimate MESH.ply OUT.ply --cell SIZE: 0, or a message on stderr and 1 (before any GPU work) when something is wrong"""
    i = argv.index("--decimate")
    paths = argv[i + 1:i + 3]
    if len(paths) < 2 or any(p.startswith("--") for p in paths):
        sys.stderr.write("asrtool: --decimate needs two files: MESH.ply OUT.ply\n")
        return 1
    cell = _option(argv, "--cell")
    try:
        cell = float(cell) if cell is not None else None
    except ValueError:
        cell = None
    if cell is None or not (0 < cell < float("inf")):
        sys.stderr.write("asrtool: --decimate needs --cell SIZE, a positive number\n")
        return 1
    if not os.path.isfile(paths[0]):
        sys.stderr.write("asrtool: --decimate: no such file: %s\n" % paths[0])
        return 1
    from asr_hip import ply
    try:
        v, t, colors = ply.read_mesh(paths[0], with_colors=True)
    except (ValueError, IndexError, OSError) as e:
        sys.stderr.write("asrtool: --decimate: cannot read %s as a mesh: %s\n" % (paths[0], e))
        return 1
    if len(v) == 0:
        sys.stderr.write("asrtool: --decimate: %s has no vertices\n" % paths[0])
        return 1
    import adaptivesurfacereconstruction as asr
    result = asr.simplify_mesh(v, t, cell, return_map=colors is not None)
    if colors is not None:
        colors = ply.average_colors(colors, result["vertex_map"], len(result["vertices"]))
    ply.write_mesh(paths[1], result["vertices"], result["triangles"], colors=colors)
    print("wrote %s: %d -> %d vertices, %d -> %d triangles, cell size %g (level %d)"
          % (paths[1], len(v), len(result["vertices"]), len(t), len(result["triangles"]), result["cell_size"],
             result["level"]))
    return 0


def _size(text):
    """the SIZE of --thin / --cell, or None when it is no positive finite number"""
    try:
        size = float(text)
    except (TypeError, ValueError):
        return None
    return size if 0 < size < float("inf") else None


def _thin_cloud(argv):
    """--thin-cloud IN.ply OUT.ply --cell SIZE: 0, or a message on stderr and 1 (before any GPU work) when something is
    wrong"""
    i = argv.index("--thin-cloud")
    paths = argv[i + 1:i + 3]
    if len(paths) < 2 or any(p.startswith("--") for p in paths):
        sys.stderr.write("asrtool: --thin-cloud needs two files: IN.ply OUT.ply\n")
        return 1
    cell = _size(_option(argv, "--cell"))
    if cell is None:
        sys.stderr.write("asrtool: --thin-cloud needs --cell SIZE, a positive number\n")
        return 1
    if not os.path.isfile(paths[0]):
        sys.stderr.write("asrtool: --thin-cloud: no such file: %s\n" % paths[0])
        return 1
    from asr_hip import ply
    try:
        points, normals, radii = ply.read_points(paths[0])
        colors = ply.read_point_colors(paths[0])
    except (ValueError, IndexError, OSError) as e:
        sys.stderr.write("asrtool: --thin-cloud: cannot read %s as a point cloud: %s\n" % (paths[0], e))
        return 1
    if len(points) == 0:
        sys.stderr.write("asrtool: --thin-cloud: %s has no points\n" % paths[0])
        return 1
    import numpy as np
    import adaptivesurfacereconstruction as asr
    result = asr.merge_points(points, normals, radii if len(radii) else None,
                              None if colors is None else colors.astype(np.float32), cell_size=cell)
    if colors is not None:
        colors = np.rint(np.clip(result["attributes"], 0, 255)).astype(np.uint8)
    ply.write_points(paths[1], result["points"], result["normals"], result["radii"], colors=colors)
    print("wrote %s: %d -> %d points (%d dropped), cell size %g"
          % (paths[1], len(points), len(result["points"]), result["report"]["dropped"], result["cell_size"]))
    return 0


def _normal_k(text):
    """the K of --estimate-normals / --k, or None when it is no integer in 3..64"""
    try:
        k = int(text)
    except (TypeError, ValueError):
        return None
    return k if 3 <= k <= 64 else None


def _viewpoint(text):
    """the x,y,z of --viewpoint as three finite floats, or None"""
    try:
        v = tuple(float(c) for c in text.split(","))
    except (AttributeError, ValueError):
        return None
    return v if len(v) == 3 and all(abs(c) < float("inf") for c in v) else None


def _orient_cloud(argv):
    """--orient-cloud IN.ply OUT.ply [--k K] [--viewpoint x,y,z]: one JSON line, 0; a message on stderr and 1 (before any
    GPU work) when something is wrong"""
    import json
    i = argv.index("--orient-cloud")
    paths = argv[i + 1:i + 3]
    if len(paths) < 2 or any(p.startswith("--") for p in paths):
        sys.stderr.write("asrtool: --orient-cloud needs two files: IN.ply OUT.ply\n")
        return 1
    k = _normal_k(_option(argv, "--k")) if "--k" in argv else 16
    if k is None:
        sys.stderr.write("asrtool: --orient-cloud: --k takes a number of neighbours K, 3 <= K <= 64\n")
        return 1
    viewpoint = None
    if "--viewpoint" in argv:
        viewpoint = _viewpoint(_option(argv, "--viewpoint"))
        if viewpoint is None:
            sys.stderr.write("asrtool: --orient-cloud: --viewpoint takes three numbers x,y,z\n")
            return 1
    if not os.path.isfile(paths[0]):
        sys.stderr.write("asrtool: --orient-cloud: no such file: %s\n" % paths[0])
        return 1
    from asr_hip import ply
    import numpy as np
    try:
        points, _, radii = ply.read_points(paths[0], require_normals=False)
        colors = ply.read_point_colors(paths[0])
    except (ValueError, IndexError, OSError) as e:
        sys.stderr.write("asrtool: --orient-cloud: cannot read %s as a point cloud: %s\n" % (paths[0], e))
        return 1
    if len(points) == 0:
        sys.stderr.write("asrtool: --orient-cloud: %s has no points\n" % paths[0])
        return 1
    if not np.isfinite(points).all():
        sys.stderr.write("asrtool: --orient-cloud: %s has points that are not finite\n" % paths[0])
        return 1
    import adaptivesurfacereconstruction as asr
    est = asr.estimate_normals(points, k, viewpoint)
    ok = est["ok"]
    ply.write_points(paths[1], points[ok], est["normals"][ok], radii[ok] if len(radii) else None,
                     colors=None if colors is None else colors[ok])
    print(json.dumps(dict(est["report"], points=int(ok.sum()), dropped=int((~ok).sum()))))
    return 0


def _register(argv):
    """--register SOURCE.ply TARGET.ply OUT.ply [--max-distance D] [--iterations N] [--point-to-point], or with --global
    [--voxel S] [--hypotheses N] [--seed K] [--max-distance D]: one JSON line, 0; a message on stderr and 1 (before any GPU
    work) when something is wrong"""
    import json
    i = argv.index("--register")
    paths = argv[i + 1:i + 4]
    if len(paths) < 3 or any(p.startswith("--") for p in paths):
        sys.stderr.write("asrtool: --register needs three files: SOURCE.ply TARGET.ply OUT.ply\n")
        return 1
    max_distance = None
    if "--max-distance" in argv:
        max_distance = _size(_option(argv, "--max-distance"))
        if max_distance is None:
            sys.stderr.write("asrtool: --register: --max-distance takes a positive number D\n")
            return 1
    iterations = 50
    if "--iterations" in argv:
        try:
            iterations = int(_option(argv, "--iterations"))
        except (TypeError, ValueError):
            iterations = 0
        if not 1 <= iterations <= 1000:
            sys.stderr.write("asrtool: --register: --iterations takes a number N, 1 <= N <= 1000\n")
            return 1
    search = "--global" in argv
    voxel, hypotheses, seed = None, 100000, 0
    if search:
        for name in ("--iterations", "--point-to-point"):
            if name in argv:
                sys.stderr.write("asrtool: --register --global: %s does not apply (the refinement runs with its defaults)\n"
                                 % name)
                return 1
        if "--voxel" in argv:
            voxel = _size(_option(argv, "--voxel"))
            if voxel is None:
                sys.stderr.write("asrtool: --register --global: --voxel takes a positive number S\n")
                return 1
        if "--hypotheses" in argv:
            try:
                hypotheses = int(_option(argv, "--hypotheses"))
            except (TypeError, ValueError):
                hypotheses = 0
            if not 1 <= hypotheses <= 2 ** 24:
                sys.stderr.write("asrtool: --register --global: --hypotheses takes a number N, 1 <= N <= 16777216\n")
                return 1
        if "--seed" in argv:
            try:
                seed = int(_option(argv, "--seed"))
            except (TypeError, ValueError):
                seed = -1
            if not 0 <= seed < 2 ** 64:
                sys.stderr.write("asrtool: --register --global: --seed takes a number K, 0 <= K < 2^64\n")
                return 1
    for p in paths[:2]:
        if not os.path.isfile(p):
            sys.stderr.write("asrtool: --register: no such file: %s\n" % p)
            return 1
    from asr_hip import ply
    import numpy as np
    clouds = []
    for p in paths[:2]:
        try:
            clouds.append(ply.read_points(p, require_normals=False) + (ply.read_point_colors(p),))
        except (ValueError, IndexError, OSError) as e:
            sys.stderr.write("asrtool: --register: cannot read %s as a point cloud: %s\n" % (p, e))
            return 1
        if len(clouds[-1][0]) == 0:
            sys.stderr.write("asrtool: --register: %s has no points\n" % p)
            return 1
    (source, source_normals, radii, colors), (target, target_normals, _, _) = clouds
    if not np.isfinite(target).all():
        sys.stderr.write("asrtool: --register: %s has points that are not finite\n" % paths[1])
        return 1
    has = lambda a: a is not None and len(a) == len(target)  # noqa: E731
    plane = has(target_normals) and "--point-to-point" not in argv
    if search and min(len(source), len(target)) < 3:
        sys.stderr.write("asrtool: --register --global: both clouds need at least 3 points\n")
        return 1
    if not plane and "--point-to-point" not in argv:
        sys.stderr.write("asrtool: --register: %s has no normals, using point-to-point\n" % paths[1])
    import adaptivesurfacereconstruction as asr
    if search:
        own = source_normals if source_normals is not None and len(source_normals) == len(source) else None
        try:
            result = asr.register_points_global(source, target, own, target_normals if plane else None, voxel_size=voxel,
                                                max_distance=max_distance, hypotheses=hypotheses, seed=seed)
        except (RuntimeError, ValueError) as e:
            sys.stderr.write("asrtool: --register --global: %s\n" % e)
            return 1
        info = result.pop("global")
        result["global"] = dict(info, transform=[[float(x) for x in row] for row in info["transform"]])
    else:
        result = asr.register_points(source, target, target_normals if plane else None, max_distance=max_distance,
                                     max_iterations=iterations)
    transform = result.pop("transform")
    if source_normals is not None and len(source_normals) == len(source):
        moved, moved_normals = asr.transform_points(source, transform, source_normals)
    else:
        # (the cloud layout has nx ny nz: a source without normals gets zero ones)
        moved, moved_normals = asr.transform_points(source, transform), np.zeros_like(source)
    ply.write_points(paths[2], moved, moved_normals, radii if radii is not None and len(radii) else None, colors=colors)
    print(json.dumps(dict(result, mode="point-to-plane" if plane else "point-to-point",
                          transform=[[float(x) for x in row] for row in transform])))
    return 0


def _smooth_mesh(argv):
    """--smooth-mesh MESH.ply OUT.ply [--iterations N] [--boundary MODE]: 0, or a message on stderr and 1 (before any GPU
    work) when something is wrong"""
    i = argv.index("--smooth-mesh")
    paths = argv[i + 1:i + 3]
    if len(paths) < 2 or any(p.startswith("--") for p in paths):
        sys.stderr.write("asrtool: --smooth-mesh needs two files: MESH.ply OUT.ply\n")
        return 1
    iterations = 10
    if "--iterations" in argv:
        try:
            iterations = int(_option(argv, "--iterations"))
        except (TypeError, ValueError):
            iterations = -1
        if not 0 <= iterations <= 1000:
            sys.stderr.write("asrtool: --smooth-mesh: --iterations takes an integer N, 0 <= N <= 1000\n")
            return 1
    boundary = "along"
    if "--boundary" in argv:
        boundary = _option(argv, "--boundary")
        if boundary not in ("free", "pinned", "along"):
            sys.stderr.write("asrtool: --smooth-mesh: --boundary is one of free, pinned, along\n")
            return 1
    if not os.path.isfile(paths[0]):
        sys.stderr.write("asrtool: --smooth-mesh: no such file: %s\n" % paths[0])
        return 1
    from asr_hip import ply
    try:
        v, t, normals, colors = ply.read_mesh(paths[0], with_normals=True, with_colors=True)
    except (ValueError, IndexError, OSError) as e:
        sys.stderr.write("asrtool: --smooth-mesh: cannot read %s as a mesh: %s\n" % (paths[0], e))
        return 1
    import adaptivesurfacereconstruction as asr
    result = asr.smooth_mesh(v, t, iterations=iterations, boundary=boundary)
    ply.write_mesh(paths[1], result["vertices"], t, normals=normals, colors=colors)
    print("wrote %s: %d vertices, %d triangles, %d iterations, boundary %s" % (paths[1], len(v), len(t), iterations, boundary))
    return 0


def _max_edges(text):
    """the N of --fill-holes / --max-edges, or None when it is no integer in 3..2^20"""
    try:
        n = int(text)
    except (TypeError, ValueError):
        return None
    return n if 3 <= n <= 1 << 20 else None


def _fill_mesh(argv):
    """--fill-mesh MESH.ply OUT.ply --max-edges N: one JSON line, 0; a message on stderr and 1 (before any GPU work) when
    something is wrong"""
    import json
    i = argv.index("--fill-mesh")
    paths = argv[i + 1:i + 3]
    if len(paths) < 2 or any(p.startswith("--") for p in paths):
        sys.stderr.write("asrtool: --fill-mesh needs two files: MESH.ply OUT.ply\n")
        return 1
    max_edges = _max_edges(_option(argv, "--max-edges"))
    if max_edges is None:
        sys.stderr.write("asrtool: --fill-mesh needs --max-edges N, an integer, 3 <= N <= 1048576\n")
        return 1
    if not os.path.isfile(paths[0]):
        sys.stderr.write("asrtool: --fill-mesh: no such file: %s\n" % paths[0])
        return 1
    from asr_hip import ply
    try:
        v, t, normals, colors = ply.read_mesh(paths[0], with_normals=True, with_colors=True)
    except (ValueError, IndexError, OSError) as e:
        sys.stderr.write("asrtool: --fill-mesh: cannot read %s as a mesh: %s\n" % (paths[0], e))
        return 1
    import adaptivesurfacereconstruction as asr
    result = asr.fill_mesh_holes(v, t, max_edges)
    v2, t2 = result.pop("vertices"), result.pop("triangles")
    if normals is not None:
        normals = ply.hub_attributes(normals, t2, len(v), len(v2))
    if colors is not None:
        colors = ply.hub_attributes(colors, t2, len(v), len(v2))
    ply.write_mesh(paths[1], v2, t2, normals=normals, colors=colors)
    print(json.dumps(result))
    return 0


def _topology(argv):
    """--topology MESH.ply: one JSON line, 0; a message on stderr and 1 (before any GPU work) when something is wrong"""
    import json
    path = _option(argv, "--topology")
    if path is None or path.startswith("--"):
        sys.stderr.write("asrtool: --topology needs a file: MESH.ply\n")
        return 1
    if not os.path.isfile(path):
        sys.stderr.write("asrtool: --topology: no such file: %s\n" % path)
        return 1
    from asr_hip import ply
    try:
        v, t = ply.read_mesh(path)
    except (ValueError, IndexError, OSError) as e:
        sys.stderr.write("asrtool: --topology: cannot read %s as a mesh: %s\n" % (path, e))
        return 1
    import adaptivesurfacereconstruction as asr
    print(json.dumps(asr.mesh_topology(t, len(v))))
    return 0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if "--version" in argv:
        import adaptivesurfacereconstruction as asr
        print("asrtool version " + asr.get_version_str())
        return 0
    if "--third-party-notices" in argv:
        import adaptivesurfacereconstruction as asr
        print(asr.get_third_party_notices())
        return 0
    if "--register" in argv:
        return _register(argv)
    if "--compare" in argv:
        return _compare(argv)
    if "--decimate" in argv:
        return _decimate(argv)
    if "--smooth-mesh" in argv:
        return _smooth_mesh(argv)
    if "--fill-mesh" in argv:
        return _fill_mesh(argv)
    if "--topology" in argv:
        return _topology(argv)
    if "--thin-cloud" in argv:
        return _thin_cloud(argv)
    if "--orient-cloud" in argv:
        return _orient_cloud(argv)
    inp, out = _option(argv, "--in"), _option(argv, "--out")
    if inp is None or out is None:
        sys.stdout.write(HELP)
        return 1
    precision = _option(argv, "--precision") or "f32"
    from asr_hip import _lib
    if precision not in _lib.PRECISIONS:
        sys.stderr.write("asrtool: unknown precision '%s' (one of %s)\n" % (precision, ", ".join(sorted(_lib.PRECISIONS))))
        return 1
    simplify = 0
    if "--simplify" in argv:  # before any GPU work
        try:
            simplify = int(_option(argv, "--simplify"))
        except (TypeError, ValueError):
            simplify = 0
        if not 1 <= simplify <= 21:
            sys.stderr.write("asrtool: --simplify takes a number of octree levels K, 1 <= K <= 21\n")
            return 1
    smooth = 0
    if "--smooth" in argv:  # before any GPU work
        try:
            smooth = int(_option(argv, "--smooth"))
        except (TypeError, ValueError):
            smooth = 0
        if not 1 <= smooth <= 1000:
            sys.stderr.write("asrtool: --smooth takes a number of iterations N, 1 <= N <= 1000\n")
            return 1
    fill_holes = 0
    if "--fill-holes" in argv:  # before any GPU work
        fill_holes = _max_edges(_option(argv, "--fill-holes"))
        if fill_holes is None:
            sys.stderr.write("asrtool: --fill-holes takes a number of rim edges N, 3 <= N <= 1048576\n")
            return 1
    thin = 0.0
    if "--thin" in argv:  # before any GPU work
        thin = _size(_option(argv, "--thin"))
        if thin is None:
            sys.stderr.write("asrtool: --thin takes a cell size SIZE, a positive number\n")
            return 1
    normal_k, viewpoint = 0, None
    if "--estimate-normals" in argv:  # before any GPU work
        normal_k = _normal_k(_option(argv, "--estimate-normals"))
        if normal_k is None:
            sys.stderr.write("asrtool: --estimate-normals takes a number of neighbours K, 3 <= K <= 64\n")
            return 1
    if "--viewpoint" in argv:  # before any GPU work
        viewpoint = _viewpoint(_option(argv, "--viewpoint"))
        if viewpoint is None or not normal_k:
            sys.stderr.write("asrtool: --viewpoint takes three numbers x,y,z and goes with --estimate-normals K\n")
            return 1
    from asr_hip import ply
    colors = None
    if "--colors" in argv:  # before any GPU work: a cloud without colours is an error
        colors = ply.read_point_colors(inp)
        if colors is None:
            sys.stderr.write("asrtool: --colors, but %s has no red/green/blue vertex properties\n" % inp)
            return 1
    import adaptivesurfacereconstruction as asr
    print("reading points")
    points, normals, radii = ply.read_points(inp, require_normals=not normal_k)
    print("%d / %d" % (len(points), len(points)))
    extra = {} if colors is None else {"point_attributes": colors.astype("float32")}
    if simplify:
        extra["simplify"] = simplify
    if smooth:
        extra["smooth"] = smooth
    if fill_holes:
        extra["fill_holes"] = fill_holes
    if thin:
        extra["thin"] = thin
    if normal_k:
        normals = None
        extra["normal_k"] = normal_k
        extra["viewpoint"] = viewpoint
    result = asr.reconstruct_surface(points, normals, radii, weights=_option(argv, "--weights"), precision=precision,
                                     vertex_normals="--normals" in argv, **extra)
    if colors is not None:
        import numpy as np
        colors = np.rint(np.clip(result["vertex_attributes"], 0, 255)).astype(np.uint8)
    ply.write_mesh(out, result["vertices"], result["triangles"], normals=result.get("vertex_normals"), colors=colors)
    print("wrote %s: %d vertices, %d triangles" % (out, len(result["vertices"]), len(result["triangles"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
