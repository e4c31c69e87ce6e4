"""NumPy restatement of the three normal-estimation stages (include/asr_hip.h).  No GPU.

  knn_lists       brute force with d2 = ((dx*dx + dy*dy) + dz*dz) in float32, rows ordered by (d2, index)
  covariances     float64, two passes: the mean of the valid neighbours, then the centred sums divided by their number
  point_normals   numpy.linalg.eigh of those covariances, the sign convention and the ok rule
  orient          Kruskal over the keys (weight bits << 32 | slot) with a signed union-find, then the top-point rule
  orient_viewpoint

Every function follows the definitions of the header literally; speed does not matter at the sizes of the tests."""
import numpy as np


def knn_lists(points, k):
    """-> (index int32 [n,k], sqdist f32 [n,k]); rows of a cloud with n < k are padded with -1 / +inf"""
    points = np.ascontiguousarray(points, np.float32)
    n = len(points)
    kk = min(n, k)
    idx = np.full((n, k), -1, np.int32)
    sq = np.full((n, k), np.inf, np.float32)
    px, py, pz = (np.ascontiguousarray(points[:, c])[None, :] for c in range(3))
    step = max(1, (1 << 22) // max(1, n))
    for s in range(0, n, step):
        q = points[s:s + step]
        dx, dy, dz = px - q[:, 0:1], py - q[:, 1:2], pz - q[:, 2:3]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        # non-negative floats order like their bit patterns: one 64-bit key per pair, ties to the smaller index
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
        if kk < n:
            key = np.partition(key, kk - 1, axis=1)[:, :kk]
        key = np.sort(key, axis=1)[:, :kk]
        idx[s:s + step, :kk] = (key & np.uint64(0xffffffff)).astype(np.int32)
        sq[s:s + step, :kk] = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, sq


def covariances(points, index):
    """-> (C float64 [n,3,3], m int [n]): two-pass covariance of the valid (!= -1) entries of each row"""
    p = np.asarray(points, np.float32).astype(np.float64)
    index = np.asarray(index)
    valid = index >= 0
    m = valid.sum(1)
    nb = p[np.where(valid, index, 0)] * valid[:, :, None]
    mean = nb.sum(1) / np.maximum(m, 1)[:, None]
    d = (p[np.where(valid, index, 0)] - mean[:, None, :]) * valid[:, :, None]
    C = np.einsum("nki,nkj->nij", d, d) / np.maximum(m, 1)[:, None, None]
    return C, m


def sign_convention(normals):
    """the component of largest magnitude positive, ties to the lowest axis (float32 in, float32 out)"""
    nrm = np.array(normals, np.float32)
    lead = np.abs(nrm).argmax(1)  # the first maximum
    neg = nrm[np.arange(len(nrm)), lead] < 0
    nrm[neg] = -nrm[neg]
    return nrm


def point_normals(points, index):
    """-> (normals f32 [n,3], eigenvalues f32 [n,3], ok bool [n], C, m)"""
    C, m = covariances(points, index)
    w, v = np.linalg.eigh(C)
    w = np.maximum(w, 0.0)
    ok = (m >= 3) & (w[:, 1] > 1e-10 * w[:, 2])
    nrm = sign_convention(v[:, :, 0].astype(np.float32))
    nrm[~ok] = 0
    return nrm, w.astype(np.float32), ok, C, m


def _dot(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    assert d.dtype == np.float32
    return d


def orient(points, normals, index):
    """propagation mode -> (normals_out f32 [n,3], flips bool [n], report dict(components, flipped, skipped))"""
    points = np.asarray(points, np.float32)
    normals = np.asarray(normals, np.float32)
    index = np.asarray(index, np.int64)
    n, k = index.shape
    zero = (normals == 0).all(1)
    i = np.repeat(np.arange(n), k)
    j = index.reshape(-1)
    e = np.arange(n * k, dtype=np.uint64)
    use = (j >= 0) & (j != i)
    use[use] &= ~zero[i[use]] & ~zero[j[use]]
    i, j, e = i[use], j[use], e[use]
    dot = _dot(normals[i], normals[j])
    w = np.maximum(np.float32(0), np.float32(1) - np.abs(dot)).astype(np.float32)
    key = (w.view(np.uint32).astype(np.uint64) << np.uint64(32)) | e
    assert len(np.unique(key)) == len(key)
    order = np.argsort(key)
    parent = np.arange(n)
    par = np.zeros(n, np.int64)  # parity against the parent

    def find(x):
        path = []
        while parent[x] != x:
            path.append(x)
            x = parent[x]
        p = 0  # compress: parities against the root, from the root's side down
        for y in reversed(path):
            p ^= par[y]
            par[y] = p
            parent[y] = x
        return x

    for t in order:
        a, b = int(i[t]), int(j[t])
        ra, rb = find(a), find(b)
        if ra == rb:
            continue
        parent[ra] = rb
        par[ra] = par[a] ^ par[b] ^ int(dot[t] < 0)
    root = np.array([find(x) for x in range(n)])
    rel = par.copy()
    rel[root == np.arange(n)] = 0
    flips = np.zeros(n, bool)
    comps = 0
    z = points[:, 2] + np.float32(0)
    for r in np.unique(root[~zero]):
        mem = np.flatnonzero((root == r) & ~zero)
        comps += 1
        top = mem[np.flatnonzero(z[mem] == z[mem].max())[0]]  # ties: the smallest index
        nz = -normals[top, 2] if rel[top] else normals[top, 2]
        flips[mem] = (rel[mem] != 0) != bool(nz < 0)
    out = normals.copy()
    out[flips] = -out[flips]
    return out, flips, {"components": comps, "flipped": int(flips.sum()), "skipped": int(zero.sum())}


def orient_viewpoint(points, normals, viewpoints):
    """-> (normals_out, flips, report): flip iff n . (v - p) < 0 in float32, zero normals skipped"""
    points = np.asarray(points, np.float32)
    normals = np.asarray(normals, np.float32)
    v = np.broadcast_to(np.asarray(viewpoints, np.float32).reshape(-1, 3), points.shape)
    zero = (normals == 0).all(1)
    flips = (_dot(normals, v - points) < 0) & ~zero
    out = normals.copy()
    out[flips] = -out[flips]
    return out, flips, {"components": 0, "flipped": int(flips.sum()), "skipped": int(zero.sum())}


def lattice_plane(m=20, z=3.0, seed=0):
    """m x m integer lattice in the plane z, shuffled"""
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2)
    pts = np.concatenate([g, np.full((len(g), 1), z)], 1).astype(np.float32)
    return np.ascontiguousarray(pts[np.random.default_rng(seed).permutation(len(pts))])


def two_spheres(n, seed=0, gap=3.0):
    """two disjoint unit spheres of n points each -> (points, centres of each point)"""
    from asr_hip import synth
    a, _ = synth.sphere_cloud(n, seed=seed)
    b, _ = synth.sphere_cloud(n, seed=seed + 1)
    c = np.zeros((2 * n, 3), np.float32)
    c[n:, 0] = gap
    return np.ascontiguousarray(np.concatenate([a, b]).astype(np.float32) + c), c
