"""The arrays asr_hip_implicit_build exposes by name (asr_hip_implicit_get): every name with the byte size that
asr_implicit_sizes implies, written out here as a table of its own, and the names one past the last grid refused."""
import ctypes

import pytest

from asr_hip import synth

pytestmark = pytest.mark.gpu

ASR_HIP_OK, ASR_HIP_EINVAL = 0, 1


def _expected(sizes):
    """name -> bytes.  V[n], P[n]: voxels and 55-slot pairs of grid n.  An up list has one pair per voxel of its own grid n
    (rows there), the inverted (down) list the same pairs with its rows on grid n + 1."""
    V, P = list(sizes.num_voxels), list(sizes.num_pairs)
    agg = int(sizes.num_agg_pairs)
    want = {
        "nodes": 8 * int(sizes.num_nodes),
        "aggregation_neighbors_index": 4 * agg,
        "aggregation_neighbors_dist": 4 * agg,
        "aggregation_scale_compat": 4 * agg,
        "aggregation_row_splits": 8 * (V[0] + 1),
    }
    for n in range(5):
        want.update({
            "voxel_keys%d" % n: 8 * V[n],
            "voxel_centers%d" % n: 12 * V[n],
            "voxel_sizes%d" % n: 4 * V[n],
            "neighbors_index%d" % n: 4 * P[n],
            "neighbors_kernel_index%d" % n: P[n],
            "neighbors_row_splits%d" % n: 8 * (V[n] + 1),
            "tiling%d" % n: 4 * V[n],
        })
    for n in range(4):
        want.update({
            "up_neighbors_index%d" % n: 4 * V[n],
            "up_neighbors_kernel_index%d" % n: V[n],
            "up_neighbors_row_splits%d" % n: 8 * (V[n] + 1),
            "tiling_up%d" % n: 4 * V[n],
            "down_neighbors_index%d" % n: 4 * V[n],
            "down_neighbors_kernel_index%d" % n: V[n],
            "down_neighbors_row_splits%d" % n: 8 * (V[n + 1] + 1),
            "tiling_down%d" % n: 4 * V[n + 1],
        })
    return want


def test_every_array_of_a_build_is_exposed_under_its_name_and_size(gpu):
    from asr_hip.pipeline import ImplicitPipeline
    p, _ = synth.scan_cloud(6000, seed=31, device=gpu)
    rad = synth.knn_radii_gpu(p, 24)
    bb = synth.bounding_box(p, 0.1)
    pipe = ImplicitPipeline(synth.make_weights(4, seed=31), device=gpu)
    sizes = pipe.build(p, rad, bb[0], bb[1])
    assert all(v > 0 for v in sizes.num_voxels) and all(v > 0 for v in sizes.num_pairs), (
        list(sizes.num_voxels), list(sizes.num_pairs))
    want = _expected(sizes)
    assert len(want) == 5 + 5 * 7 + 4 * 8

    def size_of(name):
        nbytes = ctypes.c_size_t(0)
        rc = pipe.ctx.lib.asr_hip_implicit_get(pipe.ctx._h, name.encode(), ctypes.c_void_p(0), ctypes.byref(nbytes))
        return rc, nbytes.value

    got = {name: size_of(name) for name in want}
    assert got == {name: (ASR_HIP_OK, nbytes) for name, nbytes in want.items()}
    # the copies arrive too: the row splits of the three lists of grid 0 end at their pair counts
    V, P = list(sizes.num_voxels), list(sizes.num_pairs)
    assert int(pipe.get("neighbors_row_splits0")[-1]) == P[0]
    assert int(pipe.get("up_neighbors_row_splits0")[-1]) == V[0]
    assert int(pipe.get("down_neighbors_row_splits0")[-1]) == V[0]
    for name in ("up_neighbors_index4", "tiling_down4"):
        assert size_of(name)[0] == ASR_HIP_EINVAL, name
