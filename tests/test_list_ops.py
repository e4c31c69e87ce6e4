"""The restatements and list builders of tests/list_ops_ref.py: they agree with the oracle where the oracle has the
operator, keep their own invariants, and the lists can tell a right regrouping order from a wrong one -- so that
tests/test_gpu_list_ops.py cannot silently test less than it claims.  No GPU."""
import numpy as np
import pytest

import list_ops_ref as R
import parity
import sconv_lists as L
from oracle import oracle as O

SEGS = (16, 100, 128, 256, 1024, R.DEFAULT_SEGMENT)


# ---- A. row regrouping -----------------------------------------------------------------------------------------------
def _random_list(rng):
    v = int(rng.choice([1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1000, 3001]))
    K = int(rng.choice([9, 27, 55]))
    lens = rng.integers(0, min(K, 12) + 1, size=v)
    if rng.random() < 0.3:
        lens[rng.random(v) < 0.5] = 0
    rs = np.zeros(v + 1, np.int64)
    rs[1:] = np.cumsum(lens)
    pool = rng.integers(0, K, size=(int(rng.integers(1, 41)), 12))
    slots = np.concatenate([pool[int(rng.integers(len(pool)))][:n] for n in lens] + [np.zeros(0, np.int64)])
    return slots.astype(np.uint8), rs


def test_restated_order_is_a_permutation_that_keeps_segments():
    """300 random lists: always a permutation of the rows; for seg % 128 == 0 row r stays in segment r // seg"""
    rng = np.random.default_rng(5)
    for _ in range(300):
        slots, rs = _random_list(rng)
        seg = int(rng.choice(SEGS))
        for lpt in (True, False):
            for drop in (False, True):
                perm = R.row_groups_ref(slots, rs, seg, lpt, drop)
                assert perm.dtype == np.int32 and R.is_permutation(perm, len(rs) - 1)
                if seg % 128 == 0:
                    assert R.keeps_segments(perm, seg)


def test_restated_order_on_a_list_small_enough_to_read():
    """6 rows, seg 16: ascending mask, ties in row order; the mask without slot 0 ties rows 1 and 3 with rows 0 and 2"""
    lst = R._rg_build("by hand", [[1], [0, 1], [], [0], [2, 0], [1]], 9)
    assert R.row_masks(lst.slots, lst.rs).tolist() == [2, 3, 0, 1, 5, 2]
    assert R.row_groups_ref(lst.slots, lst.rs, 16).tolist() == [2, 3, 0, 5, 1, 4]
    assert R.row_groups_ref(lst.slots, lst.rs, 16, drop_slot0=True).tolist() == [2, 3, 0, 1, 5, 4]
    assert R.row_groups_ref(lst.slots, lst.rs, 16, lpt=False).tolist() == [2, 3, 0, 5, 1, 4]  # v <= 128: lpt does nothing


def test_chunk_order_puts_the_heaviest_chunk_of_a_segment_first_and_the_partial_one_last():
    # 300 rows, one segment: rows 0..127 name slot 0, rows 128..255 slots 1..4, the last 44 rows all of 0..8
    rows = [[0]] * 128 + [[1, 2, 3, 4]] * 128 + [list(range(9))] * 44
    lst = R._rg_build("chunks", [list(r) for r in rows], 9)
    perm = R.row_groups_ref(lst.slots, lst.rs, 1024)
    assert perm[:128].tolist() == list(range(128, 256)) and perm[128:256].tolist() == list(range(128))
    assert perm[256:].tolist() == list(range(256, 300))
    # two segments of 128 rows: every chunk stays where it is
    assert R.row_groups_ref(lst.slots, lst.rs, 128).tolist() == list(range(300))


def _wrong_orders(lst, seg):
    """deliberately wrong copies of the restatement: (name, order)"""
    m = R.row_masks(lst.slots, lst.rs)
    v = len(m)
    q = np.arange(v)
    out = [("no chunk order (the 127 - cost term dropped)", R.row_groups_ref(lst.slots, lst.rs, seg, lpt=False, masks=m)),
           ("slot 0 dropped from the key", R.row_groups_ref(lst.slots, lst.rs, seg, drop_slot0=True, masks=m))]
    # ties broken by descending row: what a sort that is not stable may return
    P = np.lexsort((-q, m, q // seg))
    out.append(("equal masks in reverse row order", _chunked(P, m, seg, lambda c, cost: (128 * c // seg) * 128 + 127 - cost)))
    P = R.mask_order(m, seg, False)
    out.append(("lightest chunk first", _chunked(P, m, seg, lambda c, cost: (128 * c // seg) * 128 + cost)))
    out.append(("chunks ordered across segments", _chunked(P, m, seg, lambda c, cost: 127 - cost)))
    out.append(("no segments", R.row_groups_ref(lst.slots, lst.rs, R.DEFAULT_SEGMENT, masks=m)))
    return out


def _chunked(P, m, seg, key):
    v = len(P)
    if v <= 128:
        return P.astype(np.int32)
    nc = (v + 127) // 128
    cost = R.chunk_costs(P, m)
    ckey = np.array([key(c, int(cost[c])) if 128 * c + 128 <= v else 1 << 40 for c in range(nc)])  # the partial chunk last
    order = np.argsort(ckey, kind="stable")
    r = np.arange(v)
    return P[order[r >> 7] * 128 + (r & 127)].astype(np.int32)


def test_the_test_lists_tell_a_wrong_order_from_the_right_one():
    """every deliberately wrong copy of the restatement differs from the right one on some list and segment length of
    the GPU test -- the comparison there is not vacuous"""
    caught = {}
    for v in R.ROW_GROUP_ROWS:
        for lst in R.row_group_lists(v) + (R.fixed_row_group_lists() if v == 200 else ()):
            for seg in SEGS:
                right = R.row_groups_ref(lst.slots, lst.rs, seg)
                for name, wrong in _wrong_orders(lst, seg):
                    assert R.is_permutation(wrong, len(lst.rs) - 1)
                    if not np.array_equal(right, wrong):
                        caught.setdefault(name, []).append((lst.name, seg))
    assert len(caught) == 6, sorted(caught)
    # slot 0 in the key matters exactly where rows differ in slot 0 only
    assert {n.split("(")[0] for n, _ in caught["slot 0 dropped from the key"]} >= {"slot0_and_empty"}
    # the chunk order needs more than 128 rows
    assert all(int(n.split("(")[1].split(",")[0].rstrip(")") or 200) > 128
               for n, _ in caught["no chunk order (the 127 - cost term dropped)"])


def test_row_group_lists_keep_what_their_names_promise():
    for v in R.ROW_GROUP_ROWS:
        pools = R.row_group_lists(v)[:3]
        for lst, K in zip(pools, R.POOL_KERNEL_SIZES):
            pool = int(lst.name.split(",")[2].rstrip(") "))
            m = R.row_masks(lst.slots, lst.rs)
            assert len(m) == v and lst.slots.max() < K and 1 <= len(np.unique(m)) <= pool and (m != 0).all()
        up, full, rep, s0 = R.row_group_lists(v)[3:]
        assert np.all(np.diff(up.rs) == 1) and up.slots.max() <= 8
        n = np.diff(full.rs)
        assert np.all((n == 55) | (n <= 14)) and (n == 55).sum() >= (v * 4) // 5
        assert R.row_masks(full.slots, full.rs).max() == (1 << 55) - 1
        assert L.rows_with_duplicates(rep.slots, rep.rs) == v
        m = R.row_masks(s0.slots, s0.rs)
        if v > 3:
            assert {0, 1, 3} <= set(m.tolist())
        for lst in R.row_group_lists(v):
            assert len(lst.rs) - 1 == v and lst.rs[-1] == len(lst.slots) and lst.slots.dtype == np.uint8
            assert lst.slots.max() < 55
    assert {int(l.name.split(",")[2].rstrip(") ")) for v in R.ROW_GROUP_ROWS for l in R.row_group_lists(v)[:3]} == {1, 5, 40}
    a, b = R.fixed_row_group_lists()
    assert np.all(np.diff(a.rs)[:128] == 0) and len(b.slots) == 0 and len(b.rs) == 71


# ---- B. invert_neighbors_list ----------------------------------------------------------------------------------------
def test_inversion_restatement_equals_the_oracle():
    for lst, num_points in R.invert_lists():
        if num_points < lst.num_inp and len(lst.idx):
            continue
        gi, gr, ga = R.invert_ref(num_points, lst.idx, lst.rs, lst.slots)
        ri, rr, ra = O.invert_neighbors_list(num_points, lst.idx, lst.rs, lst.slots)
        assert np.array_equal(gi, ri) and np.array_equal(gr, rr), lst.name
        assert np.array_equal(ga, ra) and ga.dtype == np.uint8, lst.name
        assert gi.dtype == np.int32 and gr.dtype == np.int64 and len(gr) == num_points + 1


def test_inversion_lists_keep_what_their_names_promise():
    lists = dict((lst.name + "/%d" % n, lst) for lst, n in R.invert_lists())
    assert len(lists) == len(R.invert_lists())
    n = np.diff(R.every_second_row_empty().rs)
    assert np.all(n[0::2] == 0) and np.all(n[1::2] > 0)
    n = np.diff(R.runs_of_empty_rows().rs)
    assert np.all(n[:5] == 0) and np.all(n[-9:] == 0) and n[5] > 0 and n[-10] > 0 and (n == 0).sum() == 5 + 1 + 2 + 70 + 9
    assert len(R.no_rows(7).rs) == 1 and len(R.no_rows(0).rs) == 1
    u = R.unnamed_inputs()
    assert set(u.idx.tolist()) == set(range(0, 50, 7)) and u.num_inp == 60 and (np.diff(u.rs) == 0).any()
    o = R.one_input()
    assert len(o.idx) == 5000 and set(o.idx.tolist()) == {4} and (np.diff(o.rs) == 0).any()
    assert R.one_input(1, 0).num_inp == 1
    assert sorted(np.diff(R.long_rows().rs).tolist()) == [0, 1, 3000, 3001, 4500]
    s = R.stored_twice()
    for q in range(len(s.rs) - 1):
        r = s.idx[s.rs[q]:s.rs[q + 1]]
        assert r[0] == r[-1] and len(set(r.tolist())) == len(r) - 1
    # the attributes cover the whole range of a byte
    assert set(R.long_rows().slots.tolist()) == set(range(256))


def test_inverting_twice_sorts_every_row_by_input():
    for lst, num_points in R.invert_lists():
        if num_points < lst.num_inp and len(lst.idx):
            continue
        i1, r1, a1 = R.invert_ref(num_points, lst.idx, lst.rs, lst.slots)
        i2, r2, a2 = R.invert_ref(len(lst.rs) - 1, i1, r1, a1)
        idx, rs, attr = R.rows_sorted_by_input(lst)
        assert np.array_equal(i2, idx) and np.array_equal(r2, rs) and np.array_equal(a2, attr), lst.name


# ---- C. reduce_subarrays_sum -----------------------------------------------------------------------------------------
def test_reduce_restatement_against_the_oracle_and_the_sequential_bound():
    rs = R.reduce_row_splits()
    assert sorted(set(np.diff(rs).tolist())) == [0, 1, 55, 1000, 5000, 20000]
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 1, size=int(rs[-1])).astype(np.float32)
    ref, mags = R.reduce_ref(x, rs)
    assert np.array_equal(ref, mags)
    got = O.reduce_subarrays_sum(x, rs)  # sequential f32 sum, the kernel's order
    parity.assert_close(got, ref)
    assert R.err_over_limit(got, ref) < 0.1  # (1.9e-3 of 0.1 at 20000 entries)
    assert np.all(got[np.diff(rs) == 0] == 0)
    x = rng.standard_normal(int(rs[-1])).astype(np.float32)
    ref, mags = R.reduce_ref(x, rs)
    assert np.all(np.abs(O.reduce_subarrays_sum(x, rs) - ref) <= R.sequential_sum_bound(rs, mags))
    g = rng.integers(0, 100, size=int(rs[-1]))
    ref_g, _ = R.reduce_ref(x[:100], rs, g)
    assert np.allclose(ref_g, R.reduce_ref(x[:100][g], rs)[0], rtol=0, atol=0)


# ---- D. decode_mlp ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", R.DECODE_WIDTHS)
def test_decoder_restatement_leaves_room_for_any_summation_order(widths):
    """the oracle's f32 decoder stays within a fraction of the 1e-5 limit of the float64 restatement"""
    c, h1, h2 = widths
    d = R.decode_data(1000, c, h1, h2)
    args = [d[k] for k in ("code", "w1", "b1", "w2", "b2", "w3")]
    worst = 0.0
    for sizes in (None, d["sizes"]):
        ref = R.decode_ref(*args, sizes)
        got = O.decode(*args, sizes)
        parity.assert_close(got, ref)
        worst = max(worst, R.err_over_limit(got, ref))
        with O.precise():
            assert R.err_over_limit(O.decode(*args, sizes), ref) < 0.02  # double accumulation, rounded once
    assert worst < 0.25, worst
    # about half of the hidden units are cut, and the row of zeros is the bias path alone
    f1 = d["code"].astype(np.float64) @ d["w1"].astype(np.float64)[:, 3:].T + d["b1"]
    if h1 >= 16:
        assert 0.25 < (f1 > 0).mean() < 0.75
    z = R.decode_ref(np.zeros((1, c), np.float32), *args[1:])
    f2 = np.maximum(d["w2"].astype(np.float64) @ np.maximum(d["b1"].astype(np.float64), 0) + d["b2"], 0)
    assert np.allclose(z[0], d["w3"].astype(np.float64) @ f2, rtol=1e-12, atol=0)
    assert np.allclose(R.decode_ref(*args)[500], z[0], rtol=1e-12, atol=0) and not d["code"][500].any()


# ---- E. f16 conversion -----------------------------------------------------------------------------------------------
def test_f16_probe_holds_every_value_every_midpoint_and_the_edges():
    x = R.f16_probe()
    assert x.dtype == np.float32 and 100003 < len(x) < 140000
    bits = R.f16_bits_ref(x)
    assert set(bits[:65536].tolist()) - set(np.arange(65536)[np.isnan(x[:65536])].tolist()) == \
        set(np.arange(65536)[~np.isnan(x[:65536])].tolist())
    nmid = 0x7c00 - 1
    mid, mbits = x[65536:65536 + 2 * nmid], bits[65536:65536 + 2 * nmid]
    lo = np.arange(nmid, dtype=np.uint16)  # the midpoint of the f16 values with bits b and b + 1 goes to the even one
    even = np.where(lo % 2 == 0, lo, lo + 1)
    assert np.array_equal(mbits[:nmid], even) and np.array_equal(mbits[nmid:], even | 0x8000) and np.all(mid[:nmid] > 0)
    for v, want in ((65504, 0x7bff), (65519.99, 0x7bff), (65520, 0x7c00), (1e6, 0x7c00), (2.0 ** -24, 1), (2.0 ** -25, 0),
                    (-2.0 ** -25, 0x8000), (-0.0, 0x8000), (-np.inf, 0xfc00)):
        assert np.float32(v) in x and R.f16_bits_ref(np.float32(v)) == want, v
    assert np.isnan(x).sum() >= 2 and np.isnan(bits[np.isnan(x)].view(np.float16)).all()
