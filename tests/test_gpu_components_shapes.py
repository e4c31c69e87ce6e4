"""The component filter (k_uf_* / k_comp_* of csrc/asr_mesh.hip) on the shapes a contoured sphere never gives it: a long
chain (deep union-find trees before path halving), a hub in every triangle (one contended root), thousands of components
of equal size (the tie rule of k_comp_keys and keep_n cutting through a tie), isolated vertices, waves of k_comp_sizes
whose 64 lanes carry 64 labels, repeated and degenerate triangles.  Bit for bit against the oracle's serial walk."""
import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ALL = 2 ** 63 - 1


def _vertices(nv):
    """distinct, exactly representable rows: a vertex that lands in the wrong place shows"""
    i = np.arange(nv, dtype=np.float32)
    return np.stack([i, -i, i * np.float32(0.5)], 1)


def _check(gpu, v, t, keep_n, min_size, want=None):
    from asr_hip import ops
    t = np.ascontiguousarray(t, np.int32).reshape(-1, 3)
    if want is None:
        want = O.remove_connected_components(v, t, keep_n, min_size)
    got_v, got_t = ops.remove_components(torch.from_numpy(v).to(gpu), torch.from_numpy(t).to(gpu), keep_n, min_size)
    got_v, got_t = got_v.cpu().numpy(), got_t.cpu().numpy()
    assert got_v.shape == want[0].shape and got_t.shape == want[1].shape, (keep_n, min_size)
    assert np.array_equal(got_v.view(np.uint32), want[0].view(np.uint32)), (keep_n, min_size)
    assert np.array_equal(got_t, want[1]), (keep_n, min_size)
    return want


def _strip(n):
    i = np.arange(n, dtype=np.int32)
    return np.stack([i, i + 1, i + 2], 1)


@pytest.mark.parametrize("numbering", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("shuffle_triangles", [False, True])
def test_strip(gpu, numbering, shuffle_triangles):
    """20 000 triangles (i, i+1, i+2) and, behind them, a lone triangle and two isolated vertices: hanging the larger
    root below the smaller makes a chain as long as the strip unless the finds halve it"""
    rng = np.random.default_rng(3)
    n = 20000
    nv = n + 2 + 5
    t = np.concatenate([_strip(n), [[n + 2, n + 3, n + 4]]]).astype(np.int32)
    name = {"ascending": np.arange(nv), "descending": np.arange(nv)[::-1], "shuffled": rng.permutation(nv)}[numbering]
    t = name[t].astype(np.int32)
    if shuffle_triangles:
        t = t[rng.permutation(len(t))]
    v = _vertices(nv)
    kept = _check(gpu, v, t, 1, 3)
    assert kept[0].shape[0] == n + 2 and kept[1].shape[0] == n
    _check(gpu, v, t, ALL, 1)
    _check(gpu, v, t, 2, 3)


@pytest.mark.parametrize("hub", ["first", "last"])
def test_hub(gpu, hub):
    """one vertex in all 20 000 triangles: every union meets the same root"""
    n = 20000
    nv = 2 * n + 4  # the hub, 2 n rim vertices, and a triangle of its own
    h, rim = (0, 1) if hub == "first" else (nv - 1, 0)
    i = np.arange(n, dtype=np.int32)
    t = np.stack([np.full(n, h, np.int32), rim + 2 * i, rim + 2 * i + 1], 1)
    lone = rim + 2 * n
    t = np.concatenate([t, [[lone, lone + 1, lone + 2]]]).astype(np.int32)
    v = _vertices(nv)
    want = _check(gpu, v, t, 1, 3)
    assert want[0].shape[0] == 2 * n + 1 and want[1].shape[0] == n
    _check(gpu, v, t, ALL, 4)
    _check(gpu, v, t[np.random.default_rng(1).permutation(len(t))], 1, 3)


def test_ties_between_equal_components(gpu):
    """3 000 components of one triangle each: std::greater on (size, label) keeps the later ones first"""
    nc = 3000
    t = np.arange(nc * 3, dtype=np.int32).reshape(nc, 3)
    v = _vertices(nc * 3)
    for keep_n in (1, 7, 1500, 3000, ALL):
        for min_size in (1, 3, 4):
            want = _check(gpu, v, t, keep_n, min_size)
            assert want[1].shape[0] == (0 if min_size == 4 else min(keep_n, nc))
    want = O.remove_connected_components(v, t, 7, 3)
    assert np.array_equal(want[0], v[(nc - 7) * 3:])  # the last seven


def test_ties_in_a_mix_of_sizes(gpu):
    """components of 3, 3, 4, 4 and 5 vertices, 200 times over, keep_n cutting inside each run of equals"""
    tri, nv = [], 0
    for _ in range(200):
        for size in (3, 3, 4, 4, 5):
            tri += [[nv + k, nv + k + 1, nv + k + 2] for k in range(size - 2)]
            nv += size
    t = np.array(tri, np.int32)
    v = _vertices(nv)
    sizes = []
    for keep_n in (1, 100, 199, 200, 201, 400, 599, 600, 601, 800, 999, 1000, 1001):
        want = _check(gpu, v, t, keep_n, 3)
        sizes.append(want[0].shape[0])
        _check(gpu, v, t, keep_n, 4)
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes) - 1  # every cut but the last changes the result
    _check(gpu, v, t[np.random.default_rng(5).permutation(len(t))], 300, 3)


@pytest.mark.parametrize("where", ["front", "middle", "end"])
def test_isolated_vertices(gpu, where):
    n, iso = 300, 70
    t = _strip(n)
    t[100] = t[99]  # a repeated triangle: the strip stays whole
    nv = n + 2 + iso
    if where == "front":
        t = t + iso
    elif where == "middle":
        t = np.where(t >= 150, t + iso, t)
    v = _vertices(nv)
    for keep_n, min_size in ((1, 1), (2, 1), (40, 1), (ALL, 1), (ALL, 2), (1, 3), (0, 1)):
        _check(gpu, v, t.astype(np.int32), keep_n, min_size)


@pytest.mark.parametrize("nv", [1, 63, 64, 65, 257])
def test_no_triangles(gpu, nv):
    v = _vertices(nv)
    t = np.zeros((0, 3), np.int32)
    for min_size in (1, 2):
        for keep_n in (1, 10):
            want = _check(gpu, v, t, keep_n, min_size)
            assert want[0].shape[0] == (min(keep_n, nv) if min_size == 1 else 0)


def test_repeated_and_degenerate_triangles(gpu):
    """(i, i, j) joins two vertices, (i, i, i) none; a triangle given three times counts once for the component"""
    t = np.array([[0, 0, 1], [2, 2, 2], [3, 4, 5], [3, 4, 5], [5, 4, 3], [6, 7, 7], [7, 8, 8], [9, 9, 9], [10, 11, 10]],
                 np.int32)
    v = _vertices(13)
    for keep_n, min_size in ((1, 1), (1, 3), (2, 2), (3, 2), (ALL, 1), (ALL, 2), (ALL, 3), (5, 1)):
        _check(gpu, v, t, keep_n, min_size)


def test_waves_of_64_distinct_labels(gpu):
    """200 isolated vertices, then a mesh: three waves of k_comp_sizes carry 64 different labels each, the fourth is
    shared with the mesh, and the last wave of the launch is partial"""
    iso, n = 200, 333
    t = (_strip(n) + iso).astype(np.int32)
    t = np.concatenate([t, [[iso + n + 2, iso + n + 3, iso + n + 4]]]).astype(np.int32)
    nv = iso + n + 2 + 3 + 9  # nine more isolated vertices at the end
    assert nv % 64 != 0
    v = _vertices(nv)
    for keep_n, min_size in ((1, 1), (2, 1), (3, 1), (50, 1), (150, 1), (211, 1), (ALL, 1), (ALL, 2), (ALL, 3), (1, 3)):
        _check(gpu, v, t, keep_n, min_size)
