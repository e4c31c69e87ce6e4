"""numpy restatement of the global-registration contracts (include/asr_hip.h: asr_hip_point_fpfh, asr_hip_feature_match,
asr_hip_ransac_transform) and the inputs of tests/test_global_register.py and
tests/test_gpu_global_register.py.

Every expression is spelled out in the contract's order: sums of three products are (a + b) + c, no `@`, no BLAS; the
loops run over slots and over the feature dimension, vectorised over the points.  The GPU results are compared with
these bit for bit."""
import numpy as np

import register_ref as RR

# (cos beta_b, sin beta_b), beta_b = -pi + 2 pi b / 11, b = 1..10: the borders of the theta bins.  The same literals as
# ASR_FPFH_THETA_TABLE in include/asr_hip.h (tests/test_global_register.py compares the two).
THETA_TABLE = (
    (-0.84125353283118109, -0.54064081745559778),
    (-0.41541501300188632, -0.90963199535451844),
    (0.14231483827328512, -0.98982144188093268),
    (0.6548607339452851, -0.75574957435425827),
    (0.95949297361449748, -0.2817325568414295),
    (0.95949297361449748, 0.2817325568414295),
    (0.6548607339452851, 0.75574957435425827),
    (0.14231483827328512, 0.98982144188093268),
    (-0.41541501300188616, 0.90963199535451855),
    (-0.84125353283118132, 0.54064081745559744),
)
BINS = 11
FPFH_DIM = 3 * BINS


# ---- inputs -------------------------------------------------------------------------------------------------------
def bumpy(n, seed, x_range=(-1.0, 1.0)):
    """n points of z = 0.3 sin(2.5x) cos(1.7y) + 0.15xy + 0.08 sin(9x+1) sin(7y) + 0.05 cos(13xy + 2y) over
    x_range x [-1, 1] with the unit normals of the analytic gradient, f32.  register_ref.surface is too smooth for
    descriptors: on a partial overlap the search returned its 180-degree flip."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(x_range[0], x_range[1], n), rng.uniform(-1.0, 1.0, n)
    a = 13.0 * x * y + 2.0 * y
    z = (0.3 * np.sin(2.5 * x) * np.cos(1.7 * y) + 0.15 * x * y + 0.08 * np.sin(9.0 * x + 1.0) * np.sin(7.0 * y)
         + 0.05 * np.cos(a))
    zx = (0.75 * np.cos(2.5 * x) * np.cos(1.7 * y) + 0.15 * y + 0.72 * np.cos(9.0 * x + 1.0) * np.sin(7.0 * y)
          - 0.05 * np.sin(a) * 13.0 * y)
    zy = (-0.51 * np.sin(2.5 * x) * np.sin(1.7 * y) + 0.15 * x + 0.56 * np.sin(9.0 * x + 1.0) * np.cos(7.0 * y)
          - 0.05 * np.sin(a) * (13.0 * x + 2.0))
    nrm = np.stack([-zx, -zy, np.ones(n)], 1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.stack([x, y, z], 1).astype(np.float32), nrm.astype(np.float32)


MOTION = (140.0, 1.0)  # register_ref.motion: 140 degrees about (0.3, 0.5, 0.8) and the translation (1, -0.5, 0.33...)


def bumpy_pair(partial, n_source=3000, n_target=2500, seed=11):
    """-> source, source_normals, target, target_normals, truth: two DIFFERENT samples of the bumpy surface; the source is
    moved by the inverse of `truth` = register_ref.motion(*MOTION), so truth maps it back onto the target.  partial: the
    source covers x in [-1, 0.4], the target x in [-0.4, 1]."""
    src, src_n = bumpy(n_source, seed, (-1.0, 0.4) if partial else (-1.0, 1.0))
    tgt, tgt_n = bumpy(n_target, seed + 1, (-0.4, 1.0) if partial else (-1.0, 1.0))
    truth = RR.motion(*MOTION)
    inv = RR.inverse(truth)
    moved = RR.transform_f32(inv, src)
    n64 = src_n.astype(np.float64)
    moved_n = ((inv[:, 0] * n64[:, 0:1] + inv[:, 1] * n64[:, 1:2]) + inv[:, 2] * n64[:, 2:3]).astype(np.float32)
    return moved, moved_n, tgt, tgt_n, truth


def knn_brute(points, k):
    """asr_hip_knn_index's lists by brute force: the k smallest (d2, j) per row in f32, the point itself included, ties
    to the smaller index; -1 behind the end of a cloud with fewer than k points -> int32 [N,k]"""
    p = np.asarray(points, np.float32)
    n = len(p)
    out = np.full((n, k), -1, np.int32)
    for s in range(0, n, 512):
        c = p[s:s + 512]
        dx, dy, dz = c[:, 0:1] - p[:, 0][None], c[:, 1:2] - p[:, 1][None], c[:, 2:3] - p[:, 2][None]
        d2 = (dx * dx + dy * dy) + dz * dz
        order = np.argsort(d2, axis=1, kind="stable")[:, :k]
        out[s:s + 512, :order.shape[1]] = order
    return out


# ---- asr_hip_point_fpfh -------------------------------------------------------------------------------------------
def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def theta_bin(x, y):
    """the bin of atan2(y, x) among 11 equal parts of [-pi, pi] without a transcendental function: the number of borders
    beta_b the angle has reached.  y' = y cos(beta) - x sin(beta) is |(x, y)| sin(angle - beta)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    upper = y >= 0.0
    bins = np.zeros(x.shape, np.int32)
    for b in range(1, BINS):
        c, s = THETA_TABLE[b - 1]
        turned = (y * c - x * s) >= 0.0
        bins += (upper | turned) if b <= 5 else (upper & turned)
    return bins


def _unit_bin(f):
    # (NaN only where the pair is not valid: such a bin is never counted)
    return np.nan_to_num(np.clip(np.floor((f + 1.0) * 5.5), 0.0, 10.0)).astype(np.int32)


def usable_normals(normals):
    """-> (unit normals f64 [N,3] (zero rows where not usable), usable bool [N]): n / sqrt(n.n)"""
    n = np.asarray(normals, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nn = _dot(n[:, 0], n[:, 1], n[:, 2], n[:, 0], n[:, 1], n[:, 2])
        ok = np.isfinite(n).all(1) & (nn > 0.0)
        length = np.sqrt(np.where(ok, nn, 1.0))
        unit = np.where(ok[:, None], n / length[:, None], 0.0)
    return unit, ok


def pair_features(points, normals, index):
    """The Darboux-frame features of every (point, slot) -> dict of [N,k] arrays: `near` (a neighbour that counts for the
    FPFH sum: not -1, not the point itself, a usable normal, 0 < dist < inf), `valid` (near and |d x u| > 0: counts for
    the SPFH), d2 f64, alpha, phi, x, y f64 (meaningless where not valid)."""
    p = np.asarray(points, np.float32).astype(np.float64)
    idx = np.asarray(index, np.int64)
    n, k = idx.shape
    unit, ok = usable_normals(normals)
    out = {name: np.zeros((n, k)) for name in ("d2", "alpha", "phi", "x", "y")}
    out["near"], out["valid"] = np.zeros((n, k), bool), np.zeros((n, k), bool)
    rows = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for s in range(k):
            j = idx[:, s]
            jj = np.where((j >= 0) & (j < n), j, 0)
            dx, dy, dz = p[jj, 0] - p[:, 0], p[jj, 1] - p[:, 1], p[jj, 2] - p[:, 2]
            d2 = _dot(dx, dy, dz, dx, dy, dz)
            dist = np.sqrt(d2)
            near = (j >= 0) & (j < n) & (j != rows) & ok & ok[jj] & (dist > 0.0) & np.isfinite(dist)
            nix, niy, niz = unit[:, 0], unit[:, 1], unit[:, 2]
            njx, njy, njz = unit[jj, 0], unit[jj, 1], unit[jj, 2]
            a1 = _dot(nix, niy, niz, dx, dy, dz)
            a2 = _dot(njx, njy, njz, dx, dy, dz)
            swap = np.abs(a1) < np.abs(a2)
            ux, uy, uz = np.where(swap, njx, nix), np.where(swap, njy, niy), np.where(swap, njz, niz)
            tx, ty, tz = np.where(swap, nix, njx), np.where(swap, niy, njy), np.where(swap, niz, njz)
            ex, ey, ez = np.where(swap, -dx, dx), np.where(swap, -dy, dy), np.where(swap, -dz, dz)
            phi = np.where(swap, -a2, a1) / dist
            cx, cy, cz = ey * uz - ez * uy, ez * ux - ex * uz, ex * uy - ey * ux
            cn = np.sqrt(_dot(cx, cy, cz, cx, cy, cz))
            valid = near & (cn > 0.0)
            vx, vy, vz = cx / cn, cy / cn, cz / cn
            wx, wy, wz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
            out["near"][:, s], out["valid"][:, s], out["d2"][:, s], out["phi"][:, s] = near, valid, d2, phi
            out["alpha"][:, s] = _dot(vx, vy, vz, tx, ty, tz)
            out["x"][:, s] = _dot(ux, uy, uz, tx, ty, tz)
            out["y"][:, s] = _dot(wx, wy, wz, tx, ty, tz)
    return out


def point_fpfh(points, normals, index):
    """asr_hip_point_fpfh -> (fpfh f32 [N,33], spfh f32 [N,33], ok bool [N])"""
    idx = np.asarray(index, np.int64)
    n, k = idx.shape
    if ((idx != -1) & ((idx < 0) | (idx >= n))).any():
        raise ValueError("point_fpfh: a neighbour index is neither -1 nor in [0, n)")
    f = pair_features(points, normals, idx)
    _, usable = usable_normals(normals)
    valid = f["valid"]
    bins = np.stack([theta_bin(f["x"], f["y"]), BINS + _unit_bin(f["alpha"]), 2 * BINS + _unit_bin(f["phi"])])
    count = np.zeros((n, FPFH_DIM), np.int64)
    rows = np.arange(n)
    for s in range(k):
        for part in range(3):
            np.add.at(count, (rows[valid[:, s]], bins[part][valid[:, s], s]), 1)
    m = valid.sum(1)
    spfh = np.zeros((n, FPFH_DIM), np.float32)
    has = m > 0
    spfh[has] = ((100.0 * count[has].astype(np.float64)) / m[has, None].astype(np.float64)).astype(np.float32)
    acc = np.zeros((n, FPFH_DIM))
    for s in range(k):
        near = f["near"][:, s]
        j = np.where(near, idx[:, s], 0)
        acc[near] = acc[near] + spfh[j[near]].astype(np.float64) / f["d2"][near, s][:, None]
    fpfh = np.zeros((n, FPFH_DIM), np.float32)
    for part in range(3):
        a = acc[:, part * BINS:(part + 1) * BINS]
        total = np.zeros(n)
        for b in range(BINS):
            total = total + a[:, b]
        some = total > 0.0
        scaled = np.zeros((n, BINS))
        scaled[some] = (100.0 * a[some]) / total[some, None]
        fpfh[:, part * BINS:(part + 1) * BINS] = (scaled + spfh[:, part * BINS:(part + 1) * BINS].astype(np.float64)
                                                  ).astype(np.float32)
    fpfh[~usable] = 0.0
    return fpfh, spfh, usable & has


# ---- asr_hip_feature_match ----------------------------------------------------------------------------------------
def feature_match(a, b, chunk=1024):
    """asr_hip_feature_match -> (index int32 [M], squared distance f32 [M]): s = 0; s = s + (a_c - b_c)^2 over c
    ascending in f32; the smallest (s, j); -1 / +inf for a row of `a` that is not finite or when no row of `b` is"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    m, dim = a.shape
    index = np.full(m, -1, np.int32)
    sq = np.full(m, np.inf, np.float32)
    b_ok = np.isfinite(b).all(1)
    a_ok = np.isfinite(a).all(1)
    if not b_ok.any():
        return index, sq
    cols = np.nonzero(b_ok)[0]
    bb = b[cols]
    with np.errstate(over="ignore", invalid="ignore"):
        for s0 in range(0, m, chunk):
            rows = np.nonzero(a_ok[s0:s0 + chunk])[0] + s0
            if len(rows) == 0:
                continue
            s = np.zeros((len(rows), len(bb)), np.float32)
            for c in range(dim):
                t = a[rows, c][:, None] - bb[:, c][None]
                s = s + t * t
            best = s.argmin(1)  # the first of equal minima: the smallest index
            index[rows] = cols[best]
            sq[rows] = s[np.arange(len(rows)), best]
    return index, sq


def mutual_pairs(a, b):
    """-> (corr int32 [C,2] of the rows that choose each other, ascending source row; all int32 [M',2]: every source row's
    choice)"""
    ab, _ = feature_match(a, b)
    ba, _ = feature_match(b, a)
    rows = np.nonzero(ab >= 0)[0]
    every = np.stack([rows, ab[rows]], 1).astype(np.int32)
    keep = ba[every[:, 1]] == every[:, 0]
    return every[keep], every


# ---- asr_hip_ransac_transform -------------------------------------------------------------------------------------
def splitmix_draw(seed, h, r, c):
    """draw r (0..2) of hypothesis h among c correspondences: splitmix64 of seed + (3h + r + 1) golden, u64 wrap-around"""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = u(seed) + (u(3) * np.asarray(h, u) + u(r) + u(1)) * u(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
        return (((z >> u(32)) * u(c)) >> u(32)).astype(np.int64)


def _frame(p0, p1, p2):
    """-> (e1, e2, e3 as [H,3] each, good bool [H])"""
    ax, ay, az = p1[:, 0] - p0[:, 0], p1[:, 1] - p0[:, 1], p1[:, 2] - p0[:, 2]
    bx, by, bz = p2[:, 0] - p0[:, 0], p2[:, 1] - p0[:, 1], p2[:, 2] - p0[:, 2]
    la = np.sqrt(_dot(ax, ay, az, ax, ay, az))
    e1x, e1y, e1z = ax / la, ay / la, az / la
    gx, gy, gz = e1y * bz - e1z * by, e1z * bx - e1x * bz, e1x * by - e1y * bx
    lg = np.sqrt(_dot(gx, gy, gz, gx, gy, gz))
    e3x, e3y, e3z = gx / lg, gy / lg, gz / lg
    e2x, e2y, e2z = e3y * e1z - e3z * e1y, e3z * e1x - e3x * e1z, e3x * e1y - e3y * e1x
    return (np.stack([e1x, e1y, e1z], 1), np.stack([e2x, e2y, e2z], 1), np.stack([e3x, e3y, e3z], 1),
            (la > 0.0) & (lg > 0.0))


def hypotheses(source, target, corr, edge_ratio, num_hypotheses, seed):
    """-> (h int64 [E] ascending: the hypotheses that pass, transforms f64 [E,3,4])"""
    corr = np.asarray(corr, np.int64)
    c = len(corr)
    s = np.asarray(source, np.float32).astype(np.float64)[corr[:, 0]]
    t = np.asarray(target, np.float32).astype(np.float64)[corr[:, 1]]
    finite = np.isfinite(s).all(1) & np.isfinite(t).all(1)
    h = np.arange(num_hypotheses, dtype=np.int64)
    d = [splitmix_draw(seed, h, r, c) for r in range(3)]
    good = (d[0] != d[1]) & (d[0] != d[2]) & (d[1] != d[2]) & finite[d[0]] & finite[d[1]] & finite[d[2]]
    h, d = h[good], [x[good] for x in d]
    ratio = np.float64(edge_ratio)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        good = np.ones(len(h), bool)
        for i, j in ((0, 1), (0, 2), (1, 2)):
            ex, ey, ez = s[d[j], 0] - s[d[i], 0], s[d[j], 1] - s[d[i], 1], s[d[j], 2] - s[d[i], 2]
            ls = np.sqrt(_dot(ex, ey, ez, ex, ey, ez))
            ex, ey, ez = t[d[j], 0] - t[d[i], 0], t[d[j], 1] - t[d[i], 1], t[d[j], 2] - t[d[i], 2]
            lt = np.sqrt(_dot(ex, ey, ez, ex, ey, ez))
            good &= (ls >= ratio * lt) & (lt >= ratio * ls)
        fs = _frame(s[d[0]], s[d[1]], s[d[2]])
        ft = _frame(t[d[0]], t[d[1]], t[d[2]])
        good &= fs[3] & ft[3]
    keep = np.nonzero(good)[0]
    out = np.zeros((len(keep), 3, 4))
    for a in range(3):
        for b in range(3):
            out[:, a, b] = ((ft[0][keep, a] * fs[0][keep, b] + ft[1][keep, a] * fs[1][keep, b])
                            + ft[2][keep, a] * fs[2][keep, b])
    s0, t0 = s[d[0][keep]], t[d[0][keep]]
    for a in range(3):
        out[:, a, 3] = t0[:, a] - ((out[:, a, 0] * s0[:, 0] + out[:, a, 1] * s0[:, 1]) + out[:, a, 2] * s0[:, 2])
    return h[keep], out


def ransac_transform(source, target, corr, max_distance, edge_ratio=0.9, num_hypotheses=100000, seed=0):
    """asr_hip_ransac_transform -> (transform f64 [3,4] or None when no hypothesis passed,
    dict(evaluated, best_hypothesis, inliers))"""
    source, target = np.asarray(source, np.float32), np.asarray(target, np.float32)
    corr = np.asarray(corr, np.int64)
    if (corr[:, 0] < 0).any() or (corr[:, 0] >= len(source)).any() or (corr[:, 1] < 0).any() \
            or (corr[:, 1] >= len(target)).any():
        raise ValueError("ransac_transform: a correspondence is out of range")
    h, transforms = hypotheses(source, target, corr, edge_ratio, num_hypotheses, seed)
    if len(h) == 0:
        return None, {"evaluated": 0, "best_hypothesis": -1, "inliers": 0}
    cap2 = np.float32(max_distance) * np.float32(max_distance)
    s, t = source[corr[:, 0]], target[corr[:, 1]]
    fine = np.isfinite(s).all(1) & np.isfinite(t).all(1)
    s, t = s[fine], t[fine]
    counts = np.zeros(len(h), np.int64)
    s64 = s.astype(np.float64)
    chunk = max(1, (1 << 21) // max(1, len(s)))
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(0, len(h), chunk):
            x = transforms[e:e + chunk]
            # register_ref.transform_f32's arithmetic for a block of transforms: [hypothesis, pair]
            d = []
            for a in range(3):
                q = (((x[:, a, 0:1] * s64[:, 0][None] + x[:, a, 1:2] * s64[:, 1][None]) + x[:, a, 2:3] * s64[:, 2][None])
                     + x[:, a, 3:4]).astype(np.float32)
                d.append(q - t[:, a][None])
            counts[e:e + chunk] = (((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) <= cap2).sum(1)
    best = int(np.argmax(counts))  # the first of equal maxima: the smallest h
    return transforms[best], {"evaluated": len(h), "best_hypothesis": int(h[best]), "inliers": int(counts[best])}


# ---- the chain ----------------------------------------------------------------------------------------------------
def global_search(source, source_normals, target, target_normals, feature_k, max_distance, hypotheses_count, seed,
                  mutual=True, edge_ratio=0.9):
    """steps 3 to 5 of register_points_global on clouds that are taken as they are (no merge)
    -> (transform or None, report, corr)"""
    f_src = point_fpfh(source, source_normals, knn_brute(source, feature_k))[0]
    f_tgt = point_fpfh(target, target_normals, knn_brute(target, feature_k))[0]
    corr, every = mutual_pairs(f_src, f_tgt)
    used = mutual and len(corr) >= 3
    if not used:
        corr = every
    transform, report = ransac_transform(source, target, corr, max_distance, edge_ratio, hypotheses_count, seed)
    report["mutual_used"] = bool(used)
    report["correspondences"] = len(corr)
    return transform, report, corr


def rotation_angle(a, b):
    """the angle in degrees between the rotations of two [3,4] transforms"""
    r = np.asarray(a)[:, :3] @ np.asarray(b)[:, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(r) - 1.0) / 2.0, -1.0, 1.0))))
