"""numpy reference of the ICP contract (include/asr_hip.h: asr_hip_icp_step, asr_hip_icp_update,
asr_hip_register_points) and the inputs of tests/test_register.py and tests/test_gpu_register.py.

Pairs: brute force in f32 with the contract's arithmetic, ties to the smallest index.  Terms, sums, solve and update in
f64.  step() also returns the sum of the absolute values of the terms behind every entry: the scale of the f64 summation
bound the GPU sums are held to."""
import numpy as np

F32_NAN = np.float32(np.nan)
TRIANGLE = [(i, j) for i in range(6) for j in range(i, 6)]  # ata's order


# ---- inputs -------------------------------------------------------------------------------------------------------
def surface(n, seed, x_range=(-1.0, 1.0)):
    """n points of z = 0.3 sin(2.5 x) cos(1.7 y) + 0.15 x y over x_range x [-1, 1] with their analytic unit normals, f32:
    a surface without symmetries (no rigid motion maps it onto itself)"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(x_range[0], x_range[1], n), rng.uniform(-1.0, 1.0, n)
    z = 0.3 * np.sin(2.5 * x) * np.cos(1.7 * y) + 0.15 * x * y
    zx = 0.75 * np.cos(2.5 * x) * np.cos(1.7 * y) + 0.15 * y
    zy = -0.51 * np.sin(2.5 * x) * np.sin(1.7 * y) + 0.15 * x
    nrm = np.stack([-zx, -zy, np.ones(n)], 1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.stack([x, y, z], 1).astype(np.float32), nrm.astype(np.float32)


def rodrigues(w):
    """the rotation matrix of the rotation vector w (asr_hip_icp_update's formula)"""
    w = np.asarray(w, np.float64)
    th = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if th < 1e-300:
        return np.eye(3)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    h = np.sin(0.5 * th) / th
    return np.eye(3) + (np.sin(th) / th) * K + (2.0 * h * h) * (K @ K)


def motion(degrees, d):
    """the known motion of the tests: a rotation about (0.3, 0.5, 0.8) and the translation (d, -d/2, d/3) -> f64 [3,4]"""
    axis = np.array([0.3, 0.5, 0.8])
    axis /= np.linalg.norm(axis)
    return np.hstack([rodrigues(axis * np.deg2rad(degrees)), np.array([[d], [-d / 2], [d / 3]])])


def inverse(t):
    r = t[:, :3].T
    return np.hstack([r, -(r @ t[:, 3:4])])


def identity():
    return np.hstack([np.eye(3), np.zeros((3, 1))])


def transform_f32(t, p):
    """the step's transform arithmetic: f64, one rounding to f32; rows with a non-finite coordinate become NaN"""
    t = np.asarray(t, np.float64).reshape(3, 4)
    p64 = np.asarray(p, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (((t[:, 0] * p64[:, 0:1] + t[:, 1] * p64[:, 1:2]) + t[:, 2] * p64[:, 2:3]) + t[:, 3]).astype(np.float32)
    q[~np.isfinite(p64).all(1)] = F32_NAN
    return q


def moved_pair(degrees, d, n_target=20000, n_source=5000, seed=7):
    """-> target, normals, source, truth: the source is n_source of the target's own points moved by the inverse of
    motion(degrees, d); truth are their positions in the target"""
    target, normals = surface(n_target, seed)
    pick = np.random.default_rng(seed + 1).permutation(n_target)[:n_source]
    truth = target[pick]
    return target, normals, transform_f32(inverse(motion(degrees, d)), truth), truth


def frame_origin(frame):
    """asr_hip_register_points' origin: the centre of the frame's root cube"""
    return np.array([float((1 << 20) - frame.offset[a]) * float(frame.voxel_size[21]) for a in range(3)])


# ---- the contract -------------------------------------------------------------------------------------------------
def pairs_brute(target, q, cap, chunk=256):
    """index int32 [M] of the nearest target point within cap of each q, -1 for none: f32 brute force"""
    target = np.asarray(target, np.float32)
    q = np.asarray(q, np.float32)
    cap2 = np.float32(cap) * np.float32(cap)
    out = np.full(len(q), -1, np.int32)
    tx, ty, tz = target[:, 0][None], target[:, 1][None], target[:, 2][None]
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(q), chunk):
            c = q[s:s + chunk]
            dx, dy, dz = tx - c[:, 0:1], ty - c[:, 1:2], tz - c[:, 2:3]
            d2 = (dx * dx + dy * dy) + dz * dz
            d2[np.isnan(d2)] = np.float32(np.inf)
            best = d2.argmin(1)  # the first of equal minima
            ok = np.isfinite(c).all(1) & (d2[np.arange(len(c)), best] <= cap2)
            out[s:s + chunk] = np.where(ok, best, -1)
    return out


def pairs_tree(target, q, cap, k=8):
    """pairs_brute through a k-d tree: k candidates per query in f64, then the f32 rule among them.  For the drivers of
    the tests, where a tie between more than k points does not occur."""
    from scipy.spatial import cKDTree
    target = np.asarray(target, np.float32)
    q = np.asarray(q, np.float32)
    cap2 = np.float32(cap) * np.float32(cap)
    out = np.full(len(q), -1, np.int32)
    fin = np.isfinite(q).all(1)
    if not fin.any():
        return out
    k = min(k, len(target))
    _, cand = cKDTree(target.astype(np.float64)).query(q[fin].astype(np.float64), k=k)
    cand = np.sort(cand.reshape(-1, k), 1)  # ascending index: argmin then takes the smallest of equal distances
    d = target[cand] - q[fin][:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    best = d2.argmin(1)
    rows = np.arange(len(cand))
    out[fin] = np.where(d2[rows, best] <= cap2, cand[rows, best], -1)
    return out


def _rows(u, d, n):
    """e[0..5] = (u x n, n), e[6] = r for every pair -> f64 [7,P]"""
    ux, uy, uz = u.T
    dx, dy, dz = d.T
    nx, ny, nz = n.T
    return np.stack([uy * nz - uz * ny, uz * nx - ux * nz, ux * ny - uy * nx, nx, ny, nz,
                     (nx * dx + ny * dy) + nz * dz])


def step(target, normals, source, transform, origin, cap, find=pairs_brute):
    """-> (sums, abs_sums, index): sums as asr_icp_sums (dict: ata [21], atb [6], sq_residual, sq_distance, pairs, mode),
    abs_sums the same entries summed over |term|, index int32 [M] (-1: no pair)"""
    target = np.asarray(target, np.float32)
    o = np.asarray(origin, np.float64)
    q = transform_f32(transform, source)
    index = find(target, q, cap)
    if normals is not None:
        n32 = np.asarray(normals, np.float32)[np.maximum(index, 0)]
        index = np.where(np.isfinite(n32).all(1) & (n32 != 0).any(1), index, -1).astype(np.int32)
    hit = index >= 0
    u = q[hit].astype(np.float64) - o
    v = target[index[hit]].astype(np.float64) - o
    d = u - v
    pick = lambda e: np.stack([e[i] * e[j] for i, j in TRIANGLE] + [e[i] * e[6] for i in range(6)] + [e[6] * e[6]])  # noqa
    if normals is not None:
        terms = pick(_rows(u, d, np.asarray(normals, np.float32)[index[hit]].astype(np.float64)))
        absolute = np.abs(terms)
    else:
        t = [pick(_rows(u, d, np.broadcast_to(np.eye(3)[k], u.shape))) for k in range(3)]
        terms = (t[0] + t[1]) + t[2]  # the three rows of a pair first, in order
        absolute = np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2])
    sqd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    total, atotal = terms.sum(1), absolute.sum(1)
    make = lambda s, sq: {"ata": s[:21].copy(), "atb": s[21:27].copy(), "sq_residual": float(s[27]),  # noqa: E731
                          "sq_distance": float(sq), "pairs": int(hit.sum()), "mode": int(normals is not None)}
    return make(total, sqd.sum()), make(atotal, sqd.sum()), index


def matrix(sums):
    a = np.zeros((6, 6))
    for k, (i, j) in enumerate(TRIANGLE):
        a[i, j] = a[j, i] = sums["ata"][k]
    return a


def apply_update(transform, xi, origin):
    """R <- Rw R, t <- Rw (t - o) + v + o"""
    t = np.asarray(transform, np.float64).reshape(3, 4)
    o = np.asarray(origin, np.float64)
    rw = rodrigues(xi[:3])
    return np.hstack([rw @ t[:, :3], (rw @ (t[:, 3] - o) + xi[3:] + o)[:, None]])


def update(sums, origin, transform):
    """-> (transform, xi, degenerate): numpy's solve in the place of the library's Cholesky"""
    a, b = matrix(sums), np.asarray(sums["atb"], np.float64)
    if sums["pairs"] < (6 if sums["mode"] else 3) or np.linalg.matrix_rank(a) < 6:
        return np.asarray(transform, np.float64).reshape(3, 4).copy(), np.zeros(6), True
    xi = np.linalg.solve(a, -b)
    return apply_update(transform, xi, origin), xi, False


def driver(target, normals, source, origin, cap, max_iterations, rotation_tolerance=1e-7, translation_tolerance=1e-7,
           init=None, find=pairs_tree):
    """asr_hip_register_points -> (transform, report dict)"""
    t = identity() if init is None else np.asarray(init, np.float64).reshape(3, 4).copy()
    report = {"iterations": 0, "converged": False, "degenerate": False, "pairs": 0, "rmse": 0.0, "fitness": 0.0}
    for it in range(1, max_iterations + 1):
        sums, _, _ = step(target, normals, source, t, origin, cap, find)
        report.update(iterations=it, pairs=sums["pairs"],
                      rmse=float(np.sqrt(sums["sq_distance"] / sums["pairs"])) if sums["pairs"] else 0.0,
                      fitness=sums["pairs"] / len(source) if len(source) else 0.0)
        t, xi, degenerate = update(sums, origin, t)
        if degenerate:
            report["degenerate"] = True
            break
        if np.linalg.norm(xi[:3]) <= rotation_tolerance and np.linalg.norm(xi[3:]) <= translation_tolerance:
            report["converged"] = True
            break
    return t, report


def coordinate_error(transform, source, truth):
    return float(np.abs(transform_f32(transform, source).astype(np.float64) - truth.astype(np.float64)).max())
