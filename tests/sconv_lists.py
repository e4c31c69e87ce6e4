"""Synthetic neighbour lists for the f32 sparse convolution (k_sconv_mfma / k_sconv_scalar, csrc/asr_conv.hip).

The lists of the grid builder all look alike: no empty row, ~8 of 55 slots per row, many slots in play in every tile.
Each builder here makes the list of ONE edge the kernels have and the grid never produces, so that a failing test
names the edge.  Plain numpy, deterministic, at most 300 rows and 200 inputs per list; tests/test_sconv_lists.py pins
what every builder promises.

Also the two references the GPU tests share: the precise oracle with the epilogue (`reference`) and the dense fp64
autograd restatement of open3d::sparse_conv (`dense_autograd_reference`).
"""
import collections

import numpy as np

SconvList = collections.namedtuple("SconvList", "name idx slots rs num_inp kernel_size")

TILE_EDGE_ROWS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)
STEP_COUNTS = (1, 2, 3, 4)
STEP_SLOTS = {1: (32,), 2: (31, 54), 3: (0, 31, 32), 4: (0, 31, 32, 54)}
KERNEL_SIZES = (1, 9, 27, 55, 56)
# striped(): slot set of rows 16w .. 16w+15; pairwise disjoint, one empty, one with slot 54
STRIPES = ((0, 1, 2), (31,), (32, 33), (), (7, 54), tuple(range(10, 21)), (30,), (40, 41, 53))


def _build(name, rows, num_inp, kernel_size):
    """rows: per output row a list of (input, slot) pairs in the order they are stored"""
    idx = np.array([i for r in rows for i, _ in r], np.int32)
    slots = np.array([k for r in rows for _, k in r], np.uint8)
    rs = np.zeros(len(rows) + 1, np.int64)
    rs[1:] = np.cumsum([len(r) for r in rows])
    assert len(rows) <= 300 and num_inp <= 200
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < num_inp)
    return SconvList(name, idx, slots, rs, num_inp, kernel_size)


def _row(rng, slot_pool, n, num_inp):
    """n distinct slots of the pool with random inputs, in random order"""
    ks = rng.choice(np.asarray(slot_pool), size=n, replace=False)
    return [(int(rng.integers(num_inp)), int(k)) for k in ks]


def tile_edges(v):
    """v rows around the 16 / 64 / 128-row tile sizes: random rows of 0..14 of 55 slots, a few full rows, shuffled"""
    assert v in TILE_EDGE_ROWS
    rng = np.random.default_rng(1000 + v)
    num_inp = min(200, max(8, v + 3))
    rows = [_row(rng, range(55), int(rng.integers(0, 15)), num_inp) for _ in range(v)]
    if v == 1:
        rows[0] = _row(rng, range(55), 7, num_inp)
    else:
        for q in {v - 1, v // 2, v // 3}:
            rows[q] = _row(rng, range(55), 55, num_inp)
        rows[1 if v > 3 else 0] = []  # an empty row in every list
    return _build("tile_edges(%d)" % v, rows, num_inp, 55)


def step_counts(s):
    """one tile (40 rows) whose rows together use exactly s slots of {0, 31, 32, 54}: s * (cin panels) pipeline steps"""
    pool = STEP_SLOTS[s]
    rng = np.random.default_rng(2000 + s)
    rows = [_row(rng, pool, int(rng.integers(0, s + 1)), 50) for _ in range(40)]
    rows[3] = _row(rng, pool, s, 50)
    rows[17] = []
    return _build("step_counts(%d)" % s, rows, 50, 55)


def striped():
    """128 rows; rows 16w .. 16w+15 (the rows of one wave) use only the slot set STRIPES[w]"""
    rng = np.random.default_rng(3000)
    rows = []
    for w, pool in enumerate(STRIPES):
        for r in range(16):
            n = len(pool) if r == 0 else (int(rng.integers(1, len(pool) + 1)) if pool else 0)
            rows.append(_row(rng, pool, n, 150) if n else [])
    return _build("striped()", rows, 150, 55)


def empty_tiles():
    """200 rows, rows 0..127 empty (two 64-row tiles / one 128-row tile with no slot at all), the rest random"""
    rng = np.random.default_rng(4000)
    rows = [[] for _ in range(128)] + [_row(rng, range(55), int(rng.integers(1, 15)), 90) for _ in range(72)]
    return _build("empty_tiles()", rows, 90, 55)


def all_empty():
    """70 rows, no pair at all"""
    return _build("all_empty()", [[] for _ in range(70)], 12, 55)


def kernel_sizes(K):
    """kernel_size K: row 0 names every slot of K once, row 1 the highest slot alone, the rest random"""
    assert K in KERNEL_SIZES
    rng = np.random.default_rng(5000 + K)
    rows = [_row(rng, range(K), int(rng.integers(0, min(K, 14) + 1)), 30) for _ in range(20)]
    rows[0] = _row(rng, range(K), K, 30)
    rows[1] = [(int(rng.integers(30)), K - 1)]
    return _build("kernel_sizes(%d)" % K, rows, 30, K)


def duplicates():
    """the list of test_gpu_conv16.py::test_duplicate_slot_in_a_row_is_refused (64 rows, K = 3, slots 0 and 1 of every
    row), with row 5 naming slot 0 twice through two different inputs"""
    v = 64
    rows = [[(q, 0), (q, 1)] for q in range(v)]
    rows[5] = [(5, 0), (6, 0)]
    return _build("duplicates()", rows, v, 3)


def duplicates55():
    """100 rows of 55 slots; about one row in ten names one of its slots twice (two different inputs)"""
    rng = np.random.default_rng(6000)
    rows = []
    for q in range(100):
        r = _row(rng, range(55), int(rng.integers(2, 15)), 120)
        if q % 10 == 4:
            i, k = r[int(rng.integers(len(r)))]
            r.insert(int(rng.integers(len(r) + 1)), ((i + 1 + int(rng.integers(118))) % 120, k))
        rows.append(r)
    return _build("duplicates55()", rows, 120, 55)


def transposed_duplicates():
    """48 outputs over 20 inputs, K = 9: every row duplicate-free, but many outputs read the same input through the
    same slot, so most rows of the transposed list (the one the backward pass convolves over) name a slot twice"""
    rng = np.random.default_rng(7000)
    rows = [_row(rng, range(9), int(rng.integers(2, 7)), 20) for _ in range(48)]
    return _build("transposed_duplicates()", rows, 20, 9)


def out_of_range_slots():
    """K = 9, 100 rows; about 5 % of the entries carry a slot in K .. K+7 (malformed: both kernels skip them)"""
    rng = np.random.default_rng(8000)
    K = 9
    rows = []
    for _ in range(100):
        r = _row(rng, range(K), int(rng.integers(0, K + 1)), 80)
        rows.append([(i, K + int(rng.integers(8))) if rng.random() < 0.05 else (i, k) for i, k in r])
    rows[2] = [(7, K + 7)]  # a row with nothing valid
    return _build("out_of_range_slots()", rows, 80, K)


def without_out_of_range(lst):
    """(list with the entries whose slot is >= kernel_size deleted, boolean mask of the entries kept)"""
    keep = lst.slots < lst.kernel_size
    row = row_of_pairs(lst.rs)
    rs = np.zeros_like(lst.rs)
    rs[1:] = np.cumsum(np.bincount(row[keep], minlength=len(lst.rs) - 1))
    return SconvList(lst.name + " valid part", lst.idx[keep], lst.slots[keep], rs, lst.num_inp, lst.kernel_size), keep


# ---- properties ------------------------------------------------------------------------------------------------------
def row_of_pairs(rs):
    return np.repeat(np.arange(len(rs) - 1), np.diff(rs))


def row_lengths(lst):
    return np.diff(lst.rs)


def rows_with_duplicates(slots, rs):
    """number of rows that name some slot more than once"""
    row = row_of_pairs(rs)
    key = np.sort(row.astype(np.int64) * 256 + slots.astype(np.int64))
    dup_rows = key[1:][key[1:] == key[:-1]] // 256
    return len(np.unique(dup_rows))


def distinct_slots(lst, row_lo=0, row_hi=None):
    """sorted distinct slots named by the rows [row_lo, row_hi)"""
    row_hi = len(lst.rs) - 1 if row_hi is None else row_hi
    return sorted(set(lst.slots[lst.rs[row_lo]:lst.rs[row_hi]].tolist()))


def weight_scale(lst, cin):
    """standard deviation of the test filters: 0.25 / sqrt(longest row * cin).  Outputs are then O(0.25) and the
    f32 summation error of any order stays well inside 1e-5 + 1e-5 |ref| (asserted in tests/test_sconv_lists.py)"""
    n_max = max(1, int(np.diff(lst.rs).max())) if len(lst.rs) > 1 else 1
    return 0.25 / np.sqrt(n_max * cin)


def reference(O, lst, W, f, nimp=None, normalize=False, bias=None, relu=False, residual=None):
    """the oracle's operator under O.precise() (double accumulation, rounded once; sums repeated slots) and the
    epilogue of SpecialSparseConv.forward"""
    assert lst.slots.size == 0 or lst.slots.max() < W.shape[0], "the oracle reads the filter of every slot it is given"
    with O.precise():
        out = O.sparse_conv(W, f, lst.idx, lst.slots, nimp, lst.rs, normalize)
    if bias is not None:
        out = out + bias
    if relu:
        out = np.maximum(out, 0)
    if residual is not None:
        out = out + residual
    return out.astype(np.float32)


def dense_autograd_reference(f0, W0, idx, kidx, rs, imp, normalize, gout):
    """open3d::sparse_conv restated densely in fp64 on the CPU with torch autograd:
    out[q] = (1 / n_q) sum_p imp_p W[k_p]^T f[idx_p]; imp None = all ones; n_q the importance sum (the neighbour count
    without importance), rows whose sum is 0 stay undivided.  Returns (out, d out / d f, d out / d W) contracted with
    gout, as fp64 numpy arrays."""
    import torch
    v = len(rs) - 1
    cout = W0.shape[2]
    fr = torch.from_numpy(f0).double().requires_grad_(True)
    Wr = torch.from_numpy(W0).double().requires_grad_(True)
    row = torch.repeat_interleave(torch.arange(v), torch.from_numpy(np.diff(rs)))
    w = torch.from_numpy(imp).double() if imp is not None else torch.ones(len(idx), dtype=torch.float64)
    contrib = torch.einsum("pc,pco->po", fr[torch.from_numpy(idx).long()] * w[:, None],
                           Wr[torch.from_numpy(kidx.astype(np.int64))])
    ref = torch.zeros((v, cout), dtype=torch.float64).index_add(0, row, contrib)
    if normalize:
        norm = torch.zeros(v, dtype=torch.float64).index_add(0, row, w)
        ref = ref / torch.where(norm != 0, norm, torch.ones_like(norm))[:, None]
    ref.backward(torch.from_numpy(gout).double())
    return ref.detach().numpy(), fr.grad.numpy(), Wr.grad.numpy()


# ---- the cases of tests/test_gpu_sconv_lists.py (shared with the conditioning check on the CPU) -----------------------
# Without force_nt a list of a few hundred rows runs the 16- or 32-column tile, whose panels are 32 deep for cin <= 32 and
# 64 deep above: cin 4..64 is one panel, 68 two, 132 three.  Every trio therefore has one width of each panel count, and
# together the trios use every cin of {4, 16, 20, 32, 36, 64, 68, 132} and every cout of {4, 12, 16, 20, 36, 64, 68, 132}.
WIDTH_TRIOS = (
    ((4, 12), (68, 20), (132, 68)),
    ((16, 16), (68, 132), (132, 4)),
    ((20, 36), (68, 64), (132, 12)),
    ((32, 64), (68, 4), (132, 36)),
    ((36, 68), (68, 16), (132, 20)),
    ((64, 132), (68, 36), (132, 64)),
)
# forced instances: panels are 16 deep (nt 8, 16), 32 deep (nt 4) or 32 / 64 deep (nt 1, 2; cin <= 32 / above).
# cin 4, 20, 36 are 1, 2, 3 panels of 16; 20, 36, 68 are 1, 2, 3 panels of 32; 36, 68, 132 are 1, 2, 3 panels of 64.
FORCED_INSTANCES = ((1, 4), (2, 4), (2, 8), (4, 4), (4, 8), (8, 8), (16, 4), (16, 8))
FORCED_WIDTHS = ((4, 20), (20, 132), (36, 12), (68, 36), (132, 68))
TWO_BANK_WIDTHS = ((20, 8), (36, 24), (68, 56))  # (cin, cout of bank a); bank b is 8 wide
FALLBACK_WIDTHS = ((6, 5), (8, 6), (8, 8))       # the last one runs on a feature view that is not 16-byte aligned


def instance_kc(nt, cin):
    """panel depth KC of the k_sconv_mfma instance with column tile nt * 16 (asr_conv_sparse)"""
    return 16 if nt >= 8 else 32 if nt == 4 or cin <= 32 else 64


def main_lists():
    """the lists of the per-list test, each with its width trio"""
    lists = [tile_edges(v) for v in TILE_EDGE_ROWS] + [step_counts(s) for s in STEP_COUNTS]
    lists += [striped(), empty_tiles()] + [kernel_sizes(K) for K in KERNEL_SIZES]
    return [(lst, WIDTH_TRIOS[i % len(WIDTH_TRIOS)]) for i, lst in enumerate(lists)]


def forced_lists():
    return [step_counts(s) for s in STEP_COUNTS] + [striped(), empty_tiles(), tile_edges(65), tile_edges(129),
                                                    kernel_sizes(56)]


def two_bank_lists():
    return [tile_edges(17), tile_edges(65), tile_edges(129), empty_tiles(), striped()]


def all_cases():
    """every (list, cin, cout) the GPU tests convolve and compare with the reference"""
    cases = [(lst, cin, cout) for lst, trio in main_lists() for cin, cout in trio]
    cases += [(lst, cin, cout) for lst in forced_lists() for cin, cout in FORCED_WIDTHS]
    cases += [(lst, cin, c) for lst in two_bank_lists() for cin, ca in TWO_BANK_WIDTHS for c in (ca, 8)]
    cases += [(tile_edges(v), 36, 132) for v in (65, 129)]
    cases += [(tile_edges(65), cin, cout) for cin, cout in FALLBACK_WIDTHS]
    cases += [(lst, 36, 20) for lst in (tile_edges(65), empty_tiles(), striped())]  # zero sums, row lists
    cases += [(without_out_of_range(out_of_range_slots())[0], cin, cout) for cin, cout in WIDTH_TRIOS[0]]
    cases += [(lst, 32, 32) for lst in (duplicates(), duplicates55(), transposed_duplicates())]
    cases += [(all_empty(), 20, 36)]
    return cases


def make_data(lst, cin, cout, seed=0):
    """features, filters (weight_scale), bias, residual, per-point and per-pair importance of a case"""
    rng = np.random.default_rng([seed, cin, cout, len(lst.idx), len(lst.rs)])
    v = len(lst.rs) - 1
    d = dict(f=rng.standard_normal((lst.num_inp, cin)).astype(np.float32),
             W=(rng.standard_normal((lst.kernel_size, cin, cout)) * weight_scale(lst, cin)).astype(np.float32),
             bias=(rng.standard_normal(cout) * 0.1).astype(np.float32),
             res=rng.standard_normal((v, cout)).astype(np.float32),
             imp=rng.uniform(0.05, 1.0, size=lst.num_inp).astype(np.float32),
             pimp=rng.uniform(0.05, 1.0, size=len(lst.idx)).astype(np.float32))
    d["nimp"] = d["imp"][lst.idx.astype(np.int64)]
    return d


def two_bank_data(lst, cin, ca):
    """data of bank a (cin x ca) and of bank b (cin x 8, its own filters and bias; features and importance are bank a's)"""
    return make_data(lst, cin, ca), make_data(lst, cin, 8, seed=1)


def out_of_range_pair_importance(lst, cin):
    """per-pair importance over ALL entries of out_of_range_slots(), the malformed ones included"""
    return np.random.default_rng(cin).uniform(0.05, 1.0, size=len(lst.idx)).astype(np.float32)


def zero_sum_lists():
    return [tile_edges(65), empty_tiles(), striped()]


def zero_sum_importance(lst):
    """per-pair importance with rows q % 3 == 0 all 0.0 and rows q % 3 == 1 alternating +0.5 / -0.5 (an odd row ends
    with 0.0): both sums are exactly 0 in every summation order; the other rows are random"""
    rng = np.random.default_rng(9000 + len(lst.idx))
    w = rng.uniform(0.05, 1.0, size=len(lst.idx)).astype(np.float32)
    for q in range(len(lst.rs) - 1):
        lo, hi = int(lst.rs[q]), int(lst.rs[q + 1])
        if q % 3 == 0:
            w[lo:hi] = 0.0
        elif q % 3 == 1:
            n = (hi - lo) // 2 * 2
            w[lo:lo + n:2], w[lo + 1:lo + n:2], w[lo + n:hi] = 0.5, -0.5, 0.0
    return w
