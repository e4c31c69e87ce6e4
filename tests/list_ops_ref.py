"""Synthetic lists and plain NumPy restatements for the small operators between the convolutions: row regrouping
(asr_geom_row_groups_batch), invert_neighbors_list, reduce_subarrays_sum, decode_mlp, and the f16
conversion behind asr_hip_convert_f16.

The lists of an octree build all look alike: rows of 4 to 25 entries, never an empty row, slot 0 in every neighbour row,
one entry per row of an up list.  Each builder here makes a list the build never produces.  Plain numpy, deterministic;
tests/test_list_ops.py pins the restatements against the oracle and their own invariants, tests/test_gpu_list_ops.py
compares the kernels with them.  No GPU in this module.
"""
import functools

import numpy as np

import sconv_lists as L
from sconv_lists import row_of_pairs

DEFAULT_SEGMENT = 524288  # option "row_segment"; what segment_rows = 0 means
# 3001 rows in 16-row segments: 188 segments, an 8-bit segment field + the 56-bit mask = one 64-bit key; 4200 rows: 263
# segments, 9 + 56 bits, which takes two sorts (by mask, then by segment)
ROW_GROUP_ROWS = L.TILE_EDGE_ROWS + (255, 256, 257, 1000, 3001, 4200)
SEGMENT_ROWS = (0, 16, 100, 128, 256, 1024)
POOL_SIZES = (1, 5, 40)
POOL_KERNEL_SIZES = (9, 27, 55)


# ---- A. row regrouping -----------------------------------------------------------------------------------------------
def row_masks(kidx, rs):
    """m[q] = OR of 1 << (kidx[p] & 63) over row q (uint64); an empty row has mask 0"""
    m = np.zeros(len(rs) - 1, np.uint64)
    if len(kidx):
        np.bitwise_or.at(m, row_of_pairs(rs), np.uint64(1) << (np.asarray(kidx, np.uint64) & np.uint64(63)))
    return m


def popcount(x):
    return bin(int(x)).count("1")


def mask_order(m, seg, drop_slot0):
    """P: the rows in stable order by (segment = q // seg, key, q); key = m, or m >> 1 where slot 0 is dropped"""
    q = np.arange(len(m))
    key = m >> np.uint64(1) if drop_slot0 else m
    return np.lexsort((q, key, q // seg))


def chunk_costs(P, m):
    """cost of every 128-row chunk of P: slots in the union of the masks of its first 64 rows plus the same for its
    second 64 rows; a chunk with fewer than 128 rows costs 0"""
    nc = (len(P) + 127) // 128
    cost = np.zeros(nc, np.int64)
    for c in range(len(P) // 128):
        rows = P[128 * c:128 * c + 128]
        cost[c] = popcount(np.bitwise_or.reduce(m[rows[:64]])) + popcount(np.bitwise_or.reduce(m[rows[64:]]))
    return cost


def row_groups_ref(kidx, rs, seg, lpt=True, drop_slot0=False, masks=None):
    """The tiling order of a list's rows as the code documents it (int32 [v]).
    1. rows in stable order by (q // seg, slot mask, q) -- the mask without bit 0 in the batched build (drop_slot0);
    2. with lpt and more than 128 rows: the 128-row chunks of that order, stably ordered by
       (128 c // seg) * 128 + 127 - cost(c): inside a segment the chunks with the most slots first, the partial one last.
    seg: the segment length in rows, > 0 (segment_rows = 0 means DEFAULT_SEGMENT)."""
    assert seg > 0
    m = row_masks(kidx, rs) if masks is None else masks
    v = len(m)
    P = mask_order(m, seg, drop_slot0)
    if lpt and v > 128:
        nc = (v + 127) // 128
        ckey = (128 * np.arange(nc) // seg) * 128 + 127 - chunk_costs(P, m)
        order = np.argsort(ckey, kind="stable")
        r = np.arange(v)
        P = P[order[r >> 7] * 128 + (r & 127)]
    return P.astype(np.int32)


def is_permutation(perm, v):
    return len(perm) == v and np.array_equal(np.sort(np.asarray(perm, np.int64)), np.arange(v))


def keeps_segments(perm, seg):
    """perm[r] // seg == r // seg for every r: what the sharded row lists need (holds for seg % 128 == 0)"""
    return np.array_equal(np.asarray(perm, np.int64) // seg, np.arange(len(perm)) // seg)


RgList = L.SconvList  # (name, idx, slots, rs, num_inp, kernel_size); regrouping reads slots and rs only


def _rg_build(name, rows, kernel_size):
    slots = np.array([k for r in rows for k in r], np.uint8)
    rs = np.zeros(len(rows) + 1, np.int64)
    rs[1:] = np.cumsum([len(r) for r in rows])
    assert slots.size == 0 or slots.max() < 55
    return RgList(name, np.zeros(len(slots), np.int32), slots, rs, 1, kernel_size)


def pooled(v, K, pool):
    """v rows, each one of `pool` slot sets over K slots (1..min(K, 14) slots, stored in random order): equal masks recur"""
    rng = np.random.default_rng([11000, v, K, pool])
    sets = [rng.choice(K, size=int(rng.integers(1, min(K, 14) + 1)), replace=False) for _ in range(pool)]
    rows = [rng.permutation(sets[int(rng.integers(pool))]).tolist() for _ in range(v)]
    return _rg_build("pooled(%d, %d, %d)" % (v, K, pool), rows, K)


def up_like(v):
    """v rows of one entry each, a slot of 0..8: the shape of an up list"""
    rng = np.random.default_rng(12000 + v)
    return _rg_build("up_like(%d)" % v, [[int(k)] for k in rng.integers(0, 9, size=v)], 9)


def full_rows(v):
    """v rows that name all 55 slots (shuffled), every fifth row a random 1..14 of them instead"""
    rng = np.random.default_rng(13000 + v)
    rows = [rng.permutation(55).tolist() if q % 5 != 4 else
            rng.choice(55, size=int(rng.integers(1, 15)), replace=False).tolist() for q in range(v)]
    return _rg_build("full_rows(%d)" % v, rows, 55)


def repeated_slots(v):
    """v rows of 2..6 entries over 27 slots; every row names one of its slots twice (the mask is that of the set)"""
    rng = np.random.default_rng(14000 + v)
    rows = []
    for _ in range(v):
        r = rng.choice(27, size=int(rng.integers(1, 6)), replace=False).tolist()
        r.insert(int(rng.integers(len(r) + 1)), r[int(rng.integers(len(r)))])
        rows.append(r)
    return _rg_build("repeated_slots(%d)" % v, rows, 27)


SLOT0_ROWS = ((), (0,), (1,), (1, 0), (2,), (0, 2))


def slot0_and_empty(v):
    """v rows drawn from SLOT0_ROWS: empty rows next to rows that hold slot 0 alone, and rows that differ in slot 0 only.
    By the mask m the order is () < (0) < (1) < (0 1) < (2) < (0 2); by m >> 1 the pairs tie and stay in row order."""
    rng = np.random.default_rng(15000 + v)
    rows = [list(SLOT0_ROWS[int(k)]) for k in rng.integers(0, len(SLOT0_ROWS), size=v)]
    if v > 3:
        rows[0], rows[1], rows[2] = [0], [], [1, 0]
    return _rg_build("slot0_and_empty(%d)" % v, rows, 9)


@functools.lru_cache(maxsize=None)
def row_group_lists(v):
    """the lists of v rows of the per-list regrouping test; the pool sizes rotate over the kernel sizes with v"""
    i = ROW_GROUP_ROWS.index(v)
    lists = [pooled(v, K, POOL_SIZES[(i + j) % 3]) for j, K in enumerate(POOL_KERNEL_SIZES)]
    return tuple(lists + [up_like(v), full_rows(v), repeated_slots(v), slot0_and_empty(v)])


def fixed_row_group_lists():
    """lists of sconv_lists with a fixed row count: a whole 128-row chunk of empty rows; no pair at all"""
    return (L.empty_tiles(), L.all_empty())


# ---- B. invert_neighbors_list ----------------------------------------------------------------------------------------
def invert_ref(num_points, idx, rs, attr=None):
    """open3d::invert_neighbors_list: the pairs in stable order by the input they name
    -> (row of each pair int32, row splits over the inputs int64 [num_points + 1], attributes in that order or None)"""
    idx = np.asarray(idx, np.int64)
    order = np.argsort(idx, kind="stable")
    out_rs = np.zeros(num_points + 1, np.int64)
    out_rs[1:] = np.cumsum(np.bincount(idx, minlength=num_points))
    out_idx = row_of_pairs(rs)[order].astype(np.int32)
    return out_idx, out_rs, (np.asarray(attr)[order] if attr is not None else None)


InvList = L.SconvList  # slots double as uint8 attributes


def _inv_build(name, rows, num_inp):
    """rows: per row the inputs it names, in storage order; attributes: (7 p + 3) mod 256 of the pair's position p"""
    idx = np.array([i for r in rows for i in r], np.int32)
    rs = np.zeros(len(rows) + 1, np.int64)
    rs[1:] = np.cumsum([len(r) for r in rows])
    attr = ((7 * np.arange(len(idx)) + 3) % 256).astype(np.uint8)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < num_inp)
    return InvList(name, idx, attr, rs, num_inp, 256)


def every_second_row_empty():
    rng = np.random.default_rng(21000)
    rows = [rng.integers(0, 40, size=int(rng.integers(1, 9))).tolist() if q % 2 else [] for q in range(101)]
    return _inv_build("every_second_row_empty()", rows, 40)


def runs_of_empty_rows():
    """empty rows at the start (5), in the middle (runs of 1, 2 and 70) and at the end (9)"""
    rng = np.random.default_rng(21500)
    row = lambda: rng.integers(0, 33, size=int(rng.integers(1, 6))).tolist()  # noqa: E731
    rows = [[]] * 5 + [row()] + [[]] + [row(), row()] + [[]] * 2 + [row()] + [[]] * 70 + [row(), row()] + [[]] * 9
    return _inv_build("runs_of_empty_rows()", [list(r) for r in rows], 33)


def no_rows(num_inp):
    return _inv_build("no_rows(%d)" % num_inp, [], num_inp)


def unnamed_inputs():
    """60 inputs of which only the multiples of 7 below 50 are named: empty output rows, the last eleven in a row"""
    rng = np.random.default_rng(22000)
    rows = [(7 * rng.integers(0, 8, size=int(rng.integers(0, 7)))).tolist() for _ in range(80)]
    return _inv_build("unnamed_inputs()", rows, 60)


def one_input(num_inp=9, which=4):
    """5000 pairs in 700 rows that all name input `which`: one long output row, a contended histogram"""
    rng = np.random.default_rng(23000 + num_inp)
    cuts = np.sort(rng.integers(0, 5001, size=699))
    lens = np.diff(np.concatenate([[0], cuts, [5000]]))
    return _inv_build("one_input(%d, %d)" % (num_inp, which), [[which] * int(n) for n in lens], num_inp)


def long_rows():
    """rows of 3000, 0, 4500, 1 and 3001 entries over 500 inputs"""
    rng = np.random.default_rng(24000)
    rows = [rng.integers(0, 500, size=n).tolist() for n in (3000, 0, 4500, 1, 3001)]
    return _inv_build("long_rows()", rows, 500)


def stored_twice():
    """every row names one of its inputs twice (not side by side): the two pairs stay in storage order"""
    rng = np.random.default_rng(25000)
    rows = []
    for _ in range(150):
        r = rng.choice(20, size=int(rng.integers(2, 7)), replace=False).tolist()
        r.append(r[0])
        rows.append(r)
    return _inv_build("stored_twice()", rows, 20)


def from_sconv(lst):
    """a list of sconv_lists with the inversion's attributes"""
    return _inv_build(lst.name, [lst.idx[lst.rs[q]:lst.rs[q + 1]].tolist() for q in range(len(lst.rs) - 1)], lst.num_inp)


def invert_lists():
    """every list of the inversion tests, (list, num_points)"""
    empty = from_sconv(L.all_empty())
    cases = [(lst, lst.num_inp) for lst in (from_sconv(L.empty_tiles()), every_second_row_empty(), runs_of_empty_rows(),
                                            empty, no_rows(7), no_rows(0), unnamed_inputs(), one_input(), one_input(1, 0),
                                            long_rows(), stored_twice(), from_sconv(L.tile_edges(129)))]
    return cases + [(empty, 0)]


def rows_sorted_by_input(lst):
    """the list with the entries of every row in stable order by input: what inverting twice returns"""
    key = row_of_pairs(lst.rs).astype(np.int64) * (lst.num_inp + 1) + lst.idx
    order = np.argsort(key, kind="stable")
    return lst.idx[order], lst.rs, lst.slots[order]


# ---- C. reduce_subarrays_sum -----------------------------------------------------------------------------------------
REDUCE_ROW_LENGTHS = (0, 1, 55, 1000, 5000, 20000, 0, 0, 55, 1, 0)


def reduce_row_splits(lengths=REDUCE_ROW_LENGTHS):
    rs = np.zeros(len(lengths) + 1, np.int64)
    rs[1:] = np.cumsum(lengths)
    return rs


def reduce_ref(values, rs, gather_index=None):
    """float64 sum of every row (of values[gather_index] when given) -> (sums f64, sums of |x| f64)"""
    x = np.asarray(values, np.float64)
    if gather_index is not None:
        x = x[np.asarray(gather_index, np.int64)]
    # (every row summed on its own: a difference of prefix sums would cancel)
    sums = np.array([x[rs[q]:rs[q + 1]].sum() for q in range(len(rs) - 1)], np.float64)
    mags = np.array([np.abs(x[rs[q]:rs[q + 1]]).sum() for q in range(len(rs) - 1)], np.float64)
    return sums, mags


def sequential_sum_bound(rs, mags):
    """n 2^-24 sum|x|: the error bound of a sequential f32 sum of n terms (and of any other order)"""
    return np.diff(rs) * 2.0 ** -24 * mags


# ---- D. decode_mlp ---------------------------------------------------------------------------------------------------
DECODE_WIDTHS = ((32, 32, 32), (8, 8, 8), (64, 64, 64), (1, 1, 1), (33, 5, 7), (32, 16, 32), (16, 64, 8))
DECODE_ROWS = (1, 15, 16, 17, 63, 64, 65, 1000)
DECODE_ROWS_WIDTHS = ((32, 32, 32), (33, 5, 7))
DECODE_SECOND_PASS_ROWS = 131072 + 16 + 5  # 2048 blocks x 4 waves x 16 rows is one pass of k_decode_mfma


def decode_data(v, c, h1, h2, seed=0):
    """He-scaled weights, biases 0.1 normal (the ReLU cuts about half of the units), standard normal code, sizes in
    (0.01, 0.5); row v // 2 of the code is all zeros when v > 2"""
    rng = np.random.default_rng([31000, seed, c, h1, h2])
    d = dict(w1=(rng.standard_normal((h1, 3 + c)) * np.sqrt(2.0 / (3 + c))).astype(np.float32),
             b1=(0.1 * rng.standard_normal(h1)).astype(np.float32),
             w2=(rng.standard_normal((h2, h1)) * np.sqrt(2.0 / max(h1, 1))).astype(np.float32),
             b2=(0.1 * rng.standard_normal(h2)).astype(np.float32),
             w3=(rng.standard_normal((2, h2)) * np.sqrt(2.0 / max(h2, 1))).astype(np.float32))
    rng = np.random.default_rng([32000, seed, v, c])
    d["code"] = rng.standard_normal((v, c)).astype(np.float32)
    if v > 2:
        d["code"][v // 2] = 0
    d["sizes"] = rng.uniform(0.01, 0.5, size=v).astype(np.float32)
    return d


def decode_ref(code, w1, b1, w2, b2, w3, voxel_sizes=None):
    """the decoder with zero shifts in float64: relu(code W1[:, 3:]^T + b1) -> relu(. W2^T + b2) -> . W3^T"""
    code, w1, b1, w2, b2, w3 = (np.asarray(a, np.float64) for a in (code, w1, b1, w2, b2, w3))
    f1 = np.maximum(code @ w1[:, 3:].T + b1, 0)
    f2 = np.maximum(f1 @ w2.T + b2, 0)
    o = f2 @ w3.T
    if voxel_sizes is not None:
        o[:, 0] *= np.asarray(voxel_sizes, np.float64)
    return o


def err_over_limit(got, ref, atol=1e-5, rtol=1e-5):
    """largest |got - ref| / (atol + rtol |ref|): at most 1 where parity.assert_close passes"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max()) if ref.size else 0.0


# ---- E. f16 conversion -----------------------------------------------------------------------------------------------
def f16_probe():
    """float32 values at which an f32 -> f16 rounding can go wrong: every f16 value, the midpoints between neighbouring
    finite f16 values of both signs, the overflow threshold, the smallest denormal and half of it, zeros, infinities, NaN"""
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
    pos = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)  # 0 .. 65504, ascending
    mid = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (pos[:-1] + pos[1:]) / 2)  # exact in f32
    tiny = np.float32(2.0 ** -24)
    extra = np.array([65504, 65519.99, 65520, 1e6, tiny, tiny / 2, np.nextafter(tiny / 2, np.float32(1)),
                      np.nextafter(tiny / 2, np.float32(0)), 0.0, np.inf, np.nan], np.float32)
    return np.concatenate([every, mid, -mid, extra, -extra])


def f16_bits_ref(x):
    """np.float32 -> np.float16 (round to nearest even, overflow to inf) as uint16 bits"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)
