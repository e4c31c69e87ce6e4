"""The synthetic neighbour lists of tests/sconv_lists.py keep what their names promise, so that
tests/test_gpu_sconv_lists.py cannot silently test less than it claims; the test data is conditioned well enough for
the plain 1e-5 tolerance; and the duplicate-slot predicate of asr_hip.ops agrees with numpy.  No GPU."""
import numpy as np
import pytest
import torch

import parity
import sconv_lists as L
from oracle import oracle as O


def _all_lists():
    lists = [lst for lst, _ in L.main_lists()]
    return lists + [L.all_empty(), L.duplicates(), L.duplicates55(), L.transposed_duplicates(), L.out_of_range_slots()]


def _transposed(lst):
    idx, rs, slots = O.invert_neighbors_list(lst.num_inp, lst.idx, lst.rs, lst.slots)
    return slots, rs


def test_every_list_is_small_well_formed_and_deterministic():
    for lst in _all_lists():
        v = len(lst.rs) - 1
        assert v <= 300 and lst.num_inp <= 200, lst.name
        assert lst.idx.dtype == np.int32 and lst.slots.dtype == np.uint8 and lst.rs.dtype == np.int64
        assert lst.rs[0] == 0 and lst.rs[-1] == len(lst.idx) == len(lst.slots) and np.all(np.diff(lst.rs) >= 0)
        assert 1 <= lst.kernel_size <= 56
        if len(lst.idx):
            assert lst.idx.min() >= 0 and lst.idx.max() < lst.num_inp
    again = _all_lists()
    for a, b in zip(_all_lists(), again):
        assert a.name == b.name and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4]))
    assert len({lst.name for lst in again}) == len(again)


@pytest.mark.parametrize("v", L.TILE_EDGE_ROWS)
def test_tile_edges(v):
    lst = L.tile_edges(v)
    n = L.row_lengths(lst)
    assert len(n) == v and lst.kernel_size == 55 and lst.slots.max() < 55
    assert L.rows_with_duplicates(lst.slots, lst.rs) == 0
    if v > 1:
        assert (n == 0).any() and (n == 55).sum() >= 2 and n.max() == 55
        assert np.all((n <= 14) | (n == 55))
        # entry order shuffled: some row is not sorted by slot
        assert any(np.any(np.diff(lst.slots[lst.rs[q]:lst.rs[q + 1]].astype(int)) < 0) for q in range(v))
        assert {0, 54} <= set(L.distinct_slots(lst))
    else:
        assert n[0] > 0


@pytest.mark.parametrize("s", L.STEP_COUNTS)
def test_step_counts(s):
    lst = L.step_counts(s)
    assert len(lst.rs) - 1 == 40  # one tile of either height
    used = L.distinct_slots(lst)
    assert len(used) == s and set(used) <= {0, 31, 32, 54} and tuple(used) == L.STEP_SLOTS[s]
    assert L.rows_with_duplicates(lst.slots, lst.rs) == 0
    assert (L.row_lengths(lst) == 0).any()
    # together the step lists put every one of the four slots in play
    assert set().union(*(L.distinct_slots(L.step_counts(t)) for t in L.STEP_COUNTS)) == {0, 31, 32, 54}


def test_step_counts_and_widths_give_short_pipelines_of_both_parities():
    """(distinct slots of the tile) x (cin panels of the instance) = pipeline steps: 1, 2, 3 and both parities occur
    for the default instances and for every forced one"""
    steps = {s * -(-cin // L.instance_kc(2, cin)) for s in L.STEP_COUNTS for cin, _ in L.FORCED_WIDTHS}
    assert {1, 2, 3, 4, 6, 9} <= steps
    for nt, _ in L.FORCED_INSTANCES:
        panels = {-(-cin // L.instance_kc(nt, cin)) for cin, _ in L.FORCED_WIDTHS}
        assert {1, 2, 3} <= panels, (nt, panels)
    for trio in L.WIDTH_TRIOS:
        assert [-(-cin // L.instance_kc(2, cin)) for cin, _ in trio] == [1, 2, 3]
    assert {c for t in L.WIDTH_TRIOS for c, _ in t} == {4, 16, 20, 32, 36, 64, 68, 132}
    assert {c for t in L.WIDTH_TRIOS for _, c in t} == {4, 12, 16, 20, 36, 64, 68, 132}


def test_striped():
    lst = L.striped()
    assert len(lst.rs) - 1 == 128
    sets = [set(L.distinct_slots(lst, 16 * w, 16 * w + 16)) for w in range(8)]
    assert sets == [set(s) for s in L.STRIPES]
    assert sum(len(s) for s in sets) == len(set().union(*sets))  # pairwise disjoint
    assert sum(not s for s in sets) == 1 and any(54 in s for s in sets) and any(31 in s for s in sets)
    assert any(32 in s for s in sets)
    assert L.rows_with_duplicates(lst.slots, lst.rs) == 0


def test_empty_tiles_and_all_empty():
    lst = L.empty_tiles()
    n = L.row_lengths(lst)
    assert len(n) == 200 and np.all(n[:128] == 0) and np.all(n[128:] > 0)
    e = L.all_empty()
    assert len(e.rs) - 1 == 70 and len(e.idx) == 0 and len(e.slots) == 0 and np.all(e.rs == 0)


@pytest.mark.parametrize("K", L.KERNEL_SIZES)
def test_kernel_sizes(K):
    lst = L.kernel_sizes(K)
    assert lst.kernel_size == K and lst.slots.max() == K - 1
    assert sorted(lst.slots[lst.rs[0]:lst.rs[1]].tolist()) == list(range(K))
    assert lst.slots[lst.rs[1]:lst.rs[2]].tolist() == [K - 1]
    assert L.rows_with_duplicates(lst.slots, lst.rs) == 0


def test_duplicates():
    d = L.duplicates()
    assert len(d.rs) - 1 == 64 and d.kernel_size == 3
    assert d.slots[d.rs[5]:d.rs[6]].tolist() == [0, 0] and d.idx[d.rs[5]] != d.idx[d.rs[5] + 1]
    assert L.rows_with_duplicates(d.slots, d.rs) == 1
    # apart from row 5 it is the list of test_gpu_conv16.py::test_duplicate_slot_in_a_row_is_refused
    kidx = np.zeros(128, np.uint8)
    kidx[1::2] = 1
    kidx[11] = 0
    assert np.array_equal(d.slots, kidx) and np.array_equal(d.rs, np.arange(0, 129, 2))
    assert np.array_equal(np.delete(d.idx, 11), np.delete(np.repeat(np.arange(64, dtype=np.int32), 2), 11))
    d55 = L.duplicates55()
    rows = L.rows_with_duplicates(d55.slots, d55.rs)
    assert len(d55.rs) - 1 == 100 and rows == 10
    row = L.row_of_pairs(d55.rs)
    for q in range(4, 100, 10):  # the repeated slot comes with two different inputs
        ks, ii = d55.slots[row == q], d55.idx[row == q]
        k = [k for k in set(ks.tolist()) if (ks == k).sum() == 2]
        assert len(k) == 1 and len(set(ii[ks == k[0]].tolist())) == 2


def test_transposed_duplicates():
    lst = L.transposed_duplicates()
    assert len(lst.rs) - 1 == 48 and lst.num_inp == 20 and lst.kernel_size == 9
    assert L.rows_with_duplicates(lst.slots, lst.rs) == 0
    t_slots, t_rs = _transposed(lst)
    assert L.rows_with_duplicates(t_slots, t_rs) > 10  # most of the 20 rows of the transposed list
    # the lists the existing backward test uses are free of them in both directions, like every other list here
    for other in [lst for lst, _ in L.main_lists()]:
        assert L.rows_with_duplicates(other.slots, other.rs) == 0


def test_out_of_range_slots():
    lst = L.out_of_range_slots()
    K = lst.kernel_size
    bad = lst.slots >= K
    assert K == 9 and 0.02 < bad.mean() < 0.1 and lst.slots.max() == K + 7 and lst.slots[bad].min() >= K
    valid, keep = L.without_out_of_range(lst)
    assert np.array_equal(keep, ~bad) and valid.slots.max() < K and len(valid.idx) == keep.sum()
    assert len(valid.rs) == len(lst.rs) and L.rows_with_duplicates(valid.slots, valid.rs) == 0
    row = L.row_of_pairs(lst.rs)
    assert np.array_equal(np.diff(valid.rs), np.bincount(row[keep], minlength=len(lst.rs) - 1))
    assert valid.rs[3] - valid.rs[2] == 0 and lst.rs[3] - lst.rs[2] == 1  # a row that loses everything


def test_zero_sum_importance_sums_are_exactly_zero_in_any_order():
    for lst in (L.tile_edges(65), L.empty_tiles(), L.striped()):
        w = L.zero_sum_importance(lst)
        rng = np.random.default_rng(3)
        seen = set()
        for q in range(len(lst.rs) - 1):
            seg = w[lst.rs[q]:lst.rs[q + 1]]
            if q % 3 == 2 or not len(seg):
                continue
            seen.add(q % 3)
            assert set(seg.tolist()) <= ({0.0} if q % 3 == 0 else {0.5, -0.5, 0.0})
            for _ in range(4):
                s = np.float32(0)
                for x in rng.permutation(seg):
                    s = np.float32(s + x)
                assert s == 0.0
        assert seen == {0, 1}
        assert (w == -0.5).any() and (w[L.row_of_pairs(lst.rs) % 3 == 2] > 0).all()


def _share_of_tolerance(lst, W, f, nimp, normalize):
    """largest |f32 oracle - precise oracle| / (1e-5 + 1e-5 |precise|)"""
    ref = L.reference(O, lst, W, f, nimp, normalize).astype(np.float64)
    got = O.sparse_conv(W, f, lst.idx, lst.slots, nimp, lst.rs, normalize).astype(np.float64)
    return float((np.abs(got - ref) / (1e-5 + 1e-5 * np.abs(ref))).max()) if ref.size else 0.0


def test_conditioning_f32_summation_stays_within_half_the_tolerance():
    """weights of standard deviation 0.25 / sqrt(longest row * cin): the oracle's plain f32 evaluation (sequential f32
    sums, one of the orders a kernel may use) differs from the double-accumulating one by at most HALF of
    parity.assert_close's tolerance 1e-5 + 1e-5 |ref|, for every list, width and data set of the GPU tests: plain,
    importance-weighted + normalised, per-pair importance, the bank-b filters of the two-bank test, the zero-sum
    importances and the per-pair importance of the out-of-range test.  The other half is the kernels' own."""
    worst = 0.0

    def check(what, lst, W, f, nimp, normalize):
        nonlocal worst
        frac = _share_of_tolerance(lst, W, f, nimp, normalize)
        worst = max(worst, frac)
        assert frac <= 0.5, (what, lst.name, W.shape, normalize, frac)

    for lst, cin, cout in L.all_cases():
        d = L.make_data(lst, cin, cout)
        for nimp, normalize in ((None, False), (d["nimp"], True), (d["pimp"], False), (d["pimp"], True)):
            check("case", lst, d["W"], d["f"], nimp, normalize)
    for lst in L.two_bank_lists():
        for cin, ca in L.TWO_BANK_WIDTHS:
            da, db = L.two_bank_data(lst, cin, ca)
            check("bank a", lst, da["W"], da["f"], None, False)
            check("bank b", lst, db["W"], da["f"], da["nimp"], True)
    for lst in L.zero_sum_lists():
        d = L.make_data(lst, 36, 20)
        w = L.zero_sum_importance(lst)
        check("zero sums", lst, d["W"], d["f"], w, True)
        check("zero sums, undivided", lst, d["W"], d["f"], w, False)
    bad = L.out_of_range_slots()
    valid, keep = L.without_out_of_range(bad)
    for cin, cout in L.WIDTH_TRIOS[0]:
        d = L.make_data(valid, cin, cout)
        check("out of range", valid, d["W"], d["f"], L.out_of_range_pair_importance(bad, cin)[keep], False)
    print("largest share of the tolerance used by the f32 oracle: %.3f" % worst)


def test_reference_sums_repeated_slots():
    lst = L.duplicates()
    d = L.make_data(lst, 8, 4)
    ref = L.reference(O, lst, d["W"], d["f"])
    want = d["f"][5].astype(np.float64) @ d["W"][0] + d["f"][6].astype(np.float64) @ d["W"][0]
    parity.assert_close(ref[5], want)


# ---- asr_hip.ops.slots_unique_per_row ---------------------------------------------------------------------------------
def _unique(slots, rs):
    from asr_hip import ops
    return ops.slots_unique_per_row(torch.from_numpy(np.ascontiguousarray(slots)), torch.from_numpy(rs))


def test_slots_unique_per_row_agrees_with_numpy_on_every_list():
    for lst in _all_lists():
        assert _unique(lst.slots, lst.rs) == (L.rows_with_duplicates(lst.slots, lst.rs) == 0), lst.name
        t_slots, t_rs = _transposed(lst) if len(lst.idx) else (lst.slots, np.zeros(lst.num_inp + 1, np.int64))
        assert _unique(t_slots, t_rs) == (L.rows_with_duplicates(t_slots, t_rs) == 0), lst.name
    assert not _unique(L.duplicates().slots, L.duplicates().rs)
    assert not _unique(L.duplicates55().slots, L.duplicates55().rs)
    assert _unique(L.transposed_duplicates().slots, L.transposed_duplicates().rs)
    assert not _unique(*_transposed(L.transposed_duplicates()))


def test_slots_unique_per_row_edges():
    i64 = np.int64
    assert _unique(np.zeros(0, np.uint8), np.zeros(5, i64))                        # no pairs
    assert _unique(np.array([3], np.uint8), np.array([0, 0, 1], i64))              # one pair
    assert not _unique(np.array([3, 3], np.uint8), np.array([0, 2], i64))          # one row, twice
    assert _unique(np.array([3, 3], np.uint8), np.array([0, 1, 2], i64))           # same slot in neighbouring rows
    assert _unique(np.array([3, 3], np.uint8), np.array([0, 1, 1, 1, 2], i64))     # ... with empty rows between
    assert not _unique(np.array([255, 0, 255], np.uint8), np.array([0, 0, 3], i64))  # not adjacent, highest slot value
    assert _unique(np.array([255, 0], np.uint8), np.array([0, 1, 2], i64))         # (row 0, 255) is not (row 1, 0) - 1
    assert _unique(np.arange(56, dtype=np.uint8), np.array([0, 56], i64))
    # int32 slots, as a host may pass them
    from asr_hip import ops
    assert not ops.slots_unique_per_row(torch.tensor([1, 2, 1], dtype=torch.int32), torch.tensor([0, 3]))
