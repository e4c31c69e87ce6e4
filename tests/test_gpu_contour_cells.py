"""The contouring kernels (k_contour_active / _vertices / _edges of csrc/asr_mesh.hip, the unordered_set replay of
csrc/asr_uset.h on the device) on the hand-made cells of tests/contour_cells.py: 1..29 cells round one edge, open fans,
two arcs, cells with repeated corners, zeros / NaN / infinities / denormals in the field, odd thresholds, indices out of
range.  Every comparison with the oracle is on bits -- vertices as uint32, triangles as they are -- or on the error both
sides report; tests/test_contour_cells.py shows that the inputs reach what they are meant to reach."""
import numpy as np
import pytest
import torch

import contour_cells as C
from asr_hip import AsrHipError
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SORT = "cannot sort duals"


def _contour(gpu, values, duals, positions, thr=1.0):
    from asr_hip import ops
    v, t = ops.contour(torch.from_numpy(np.ascontiguousarray(values)).to(gpu),
                       torch.from_numpy(np.ascontiguousarray(duals)).to(gpu),
                       torch.from_numpy(np.ascontiguousarray(positions)).to(gpu), thr)
    return v.cpu().numpy(), t.cpu().numpy()


def _same_bits(got, want):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1], want[1])


def _both(gpu, values, duals, positions, thr=1.0):
    """both sides give a mesh with the same bits, or both report "cannot sort duals" -> True for a mesh"""
    try:
        want = O.create_triangle_mesh(values, duals, positions, thr)
    except RuntimeError as e:
        assert SORT in str(e)
        with pytest.raises(AsrHipError, match=SORT):
            _contour(gpu, values, duals, positions, thr)
        return False
    _same_bits(_contour(gpu, values, duals, positions, thr), want)
    return True


@pytest.mark.parametrize("pad", C.RING_PADS)
@pytest.mark.parametrize("n", C.RING_N)
def test_closed_rings(gpu, n, pad):
    """n cells round one edge, the vertex ids shifted by `pad`: past 8 entries the replay's list is longer than any real
    tree makes it, from 14 on it has rehashed to 29 buckets"""
    assert _both(gpu, *C.ring(n, pad=pad))


@pytest.mark.parametrize("n,gap", C.OPEN_RINGS)
def test_open_rings(gpu, n, gap):
    for pad in (0, 2):
        assert _both(gpu, *C.ring(n, missing=(gap,), pad=pad))


@pytest.mark.parametrize("n,owner", C.ONCE_RINGS)
def test_ring_edge_emitted_once(gpu, n, owner):
    v, d, p = C.ring(n, owner=owner, pad=2)
    assert _both(gpu, v, d, p)
    assert _contour(gpu, v, d, p)[1].shape[0] == n


def test_thirty_cells_round_an_edge_are_refused(gpu):
    """A documented limit, not parity: the oracle, like the reference, goes on and emits the fans of
    30.  The count call refuses, the fill call that would follow is refused too, and the context then contours a ring of
    29."""
    from asr_hip import ops
    v, d, p = C.ring(30, pad=5)
    assert O.create_triangle_mesh(v, d, p)[1].shape[0] == 30 * 30
    with pytest.raises(AsrHipError, match="more than 29 dual cells around one edge"):
        _contour(gpu, v, d, p)
    ctx = ops.context(gpu)
    out_v = torch.empty((8, 3), dtype=torch.float32, device=gpu)
    out_t = torch.empty((8, 3), dtype=torch.int32, device=gpu)
    with pytest.raises(AsrHipError, match="must follow"):
        ctx.call("asr_hip_contour_fill", ops.ptr(out_v), ops.ptr(out_t))
    assert _both(gpu, *C.ring(29, pad=5))


def test_two_arcs_cannot_be_sorted(gpu):
    n, gaps = C.TWO_GAPS
    assert not _both(gpu, *C.ring(n, missing=gaps))
    assert not _both(gpu, *C.ring(n, missing=gaps, pad=1000))
    assert _both(gpu, *C.ring(n, missing=gaps[:1]))  # the context is usable afterwards


def test_two_cells_without_a_common_face(gpu):
    """no triangle comes of two cells, but the reference orders them first and ends there (contouring.cpp:360-369)"""
    assert not _both(gpu, *C.ring(4, missing=(1, 3)))
    assert _both(gpu, *C.ring(4, missing=(2, 3)))


@pytest.mark.parametrize("m,frac,seed", C.LATTICES)
def test_merged_lattices(gpu, m, frac, seed):
    _both(gpu, *C.merged_lattice(m, frac, seed))


_SPECIAL = C.special_cases()


@pytest.mark.parametrize("case", _SPECIAL, ids=[c[0] for c in _SPECIAL])
def test_special_values(gpu, case):
    """zeros of both signs, NaN, infinities, denormals, FLT_MAX and FLT_MIN in the signed field; the threshold itself,
    its successor, NaN and infinity in the unsigned one; thresholds 1, 0, -1, inf and NaN.  The f32 test of
    crossing() and the f64 one of k_contour_vertices must agree on every edge or a vertex is 0 / 0."""
    _, v, d, p, thr = case
    assert _both(gpu, v, d, p, thr)


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_plane_through_mixed_density_tree(gpu, noise):
    """a real octree whose surface runs through the coarse rims: n = 1..7 in numbers (the sphere has few of 1, 3, 5)"""
    assert _both(gpu, *C.plane_field(5000, 0, noise))


def test_calling_conventions(gpu):
    from asr_hip import ops
    v, d, p = C.merged_lattice(7, 0.05, 0)
    want = O.create_triangle_mesh(v, d, p)
    # values one float into their storage: the float2 loads are 4-byte aligned only
    store = torch.full((v.size + 1,), 7.0, dtype=torch.float32, device=gpu)
    view = store[1:].view(-1, 2)
    view.copy_(torch.from_numpy(v))
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    td, tp = torch.from_numpy(d).to(gpu), torch.from_numpy(p).to(gpu)
    first = ops.contour(view, td, tp, 1.0)
    _same_bits((first[0].cpu().numpy(), first[1].cpu().numpy()), want)
    again = ops.contour(view, td, tp, 1.0)  # two identical calls, identical bits
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(first[1], again[1])
    # fill without count
    ctx = ops.context(gpu)
    with pytest.raises(AsrHipError, match="must follow"):
        ctx.call("asr_hip_contour_fill", ops.ptr(first[0]), ops.ptr(first[1]))
    # nothing to do
    for vv, dd, pp in ((v, d[:0], p), (v[:0], d[:0], p[:0])):
        got = _contour(gpu, vv, dd, pp)
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    _same_bits(_contour(gpu, v, d, p), want)


@pytest.mark.parametrize("bad", ["V", "-1", "2^31", "-2^63"])
def test_index_out_of_range_is_refused(gpu, bad):
    """k_contour_active checks every corner against [0, V) before it loads anything through it; the cell counts as
    inactive and the count call reports it before a later kernel runs"""
    v, d, p = C.merged_lattice(7, 0.05, 0)
    good, d = d, d.copy()
    d[len(d) // 2, 5] = {"V": len(v), "-1": -1, "2^31": 2 ** 31, "-2^63": -2 ** 63}[bad]
    with pytest.raises(AsrHipError, match="contour: dual vertex index out of range"):
        _contour(gpu, v, d, p)
    assert _both(gpu, v, good, p)  # the context is usable afterwards
