"""The f32 sparse convolution (k_sconv_mfma, k_sconv_scalar: csrc/asr_conv.hip) on the synthetic neighbour lists of
tests/sconv_lists.py: tile and grid edges, 1..4-slot tiles (the shortest paths through the prefetch pipeline), slots
31 / 32 / 54 / 55, per-wave slot stripes, empty rows and tiles, zero importance sums, row lists, malformed slots,
repeated slots.  Every value is compared with the oracle's operator under O.precise() within the plain
parity.assert_close tolerance; tests/test_sconv_lists.py shows that the data leaves the kernels half of it.

Features are a column slice of a wider buffer (inp_ld = cin + 4) whose pad columns hold 1e3;
the residual is a column slice too (residual_ld = cout + 3); `out` and `out_importance`
are slices of buffers pre-filled with -3 that have pad columns and a guard row / element on either side, and every
call asserts that the guards are untouched."""
import numpy as np
import pytest
import torch

import parity
import sconv_lists as L
from oracle import oracle as O

pytestmark = pytest.mark.gpu

_close = parity.assert_close
SENTINEL = -3.0


def _t(a, gpu):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _opt(a, gpu):
    return None if a is None else _t(a, gpu)


def _conv(gpu, lst, W, f, importance=False, feature_offset=0, filters_b=None, bias=None, bias_b=None, residual=None,
          inp_importance=None, neighbors_importance=None, row_perm=None, **kw):
    """ops.sparse_conv on padded, guarded buffers -> (out [v, cout (+ cout_b)], out_importance [v] or None)"""
    from asr_hip import ops
    v, cin = len(lst.rs) - 1, f.shape[1]
    ctot = W.shape[2] + (filters_b.shape[2] if filters_b is not None else 0)
    ld = cin if feature_offset else cin + 4  # off the 16-byte grid: contiguous rows (a padded view would be copied)
    flat = torch.full((lst.num_inp * ld + feature_offset,), 1e3, dtype=torch.float32, device=gpu)
    feats = flat[feature_offset:].view(lst.num_inp, ld)[:, :cin]
    feats.copy_(_t(f, gpu))
    assert (feats.data_ptr() % 16 != 0) == bool(feature_offset % 4)
    res = None
    if residual is not None:  # a column slice of a wider buffer as well (residual_ld = cout + 3, off the 16-byte grid)
        rbuf = torch.full((v, ctot + 3), 1e3, dtype=torch.float32, device=gpu)
        res = rbuf[:, 2:2 + ctot]
        res.copy_(_t(residual, gpu))
        assert v < 2 or (res.stride(0) == ctot + 3 and not res.is_contiguous())
    obuf = torch.full((v + 2, ctot + 4), SENTINEL, dtype=torch.float32, device=gpu)
    ibuf = torch.full((v + 2,), SENTINEL, dtype=torch.float32, device=gpu)
    ops.sparse_conv(_t(W, gpu), feats, _t(lst.idx, gpu), _t(lst.slots, gpu), _t(lst.rs, gpu), out=obuf[1:v + 1, :ctot],
                    out_importance=ibuf[1:v + 1] if importance else None, filters_b=_opt(filters_b, gpu),
                    bias=_opt(bias, gpu), bias_b=_opt(bias_b, gpu), residual=res,
                    inp_importance=_opt(inp_importance, gpu), neighbors_importance=_opt(neighbors_importance, gpu),
                    row_perm=_opt(row_perm, gpu), **kw)
    o, i = obuf.cpu().numpy(), ibuf.cpu().numpy()
    assert np.all(o[:, ctot:] == SENTINEL) and np.all(o[0] == SENTINEL) and np.all(o[-1] == SENTINEL), "out guards"
    assert i[0] == SENTINEL and i[-1] == SENTINEL and (importance or np.all(i == SENTINEL)), "out_importance guards"
    assert bool(torch.all(flat[feature_offset:].view(lst.num_inp, ld)[:, cin:] == 1e3)), "feature pad columns"
    return o[1:v + 1, :ctot].copy(), (i[1:v + 1].copy() if importance else None)


def _sum(lst, w):
    """importance sum of every row, in double"""
    return np.bincount(L.row_of_pairs(lst.rs), weights=w.astype(np.float64), minlength=len(lst.rs) - 1)


def _counts(gpu, reset=False):
    from asr_hip import ops
    return ops.context(gpu).sconv_variant_counts(reset=reset)


def _three_ways(gpu, lst, d, ref_lst=None, keep=None, W=None, **kw):
    """the three uses of the operator, each against the reference on ref_lst (default: the list itself):
    plain with bias, relu and residual; per-point importance with normalize and the importance sum; per-pair importance
    given together with a per-point one (the per-pair one wins).  Returns the three outputs."""
    ref_lst = lst if ref_lst is None else ref_lst
    keep = slice(None) if keep is None else keep
    Wg = d["W"] if W is None else W
    outs = []
    out, _ = _conv(gpu, lst, Wg, d["f"], bias=d["bias"], relu=True, residual=d["res"], **kw)
    _close(out, L.reference(O, ref_lst, d["W"], d["f"], bias=d["bias"], relu=True, residual=d["res"]))
    outs.append(out)
    nimp = d["imp"][lst.idx.astype(np.int64)]
    out, oimp = _conv(gpu, lst, Wg, d["f"], importance=True, inp_importance=d["imp"], normalize=True, bias=d["bias"],
                      relu=True, **kw)
    _close(out, L.reference(O, ref_lst, d["W"], d["f"], nimp[keep], True, bias=d["bias"], relu=True))
    _close(oimp, _sum(ref_lst, nimp[keep]))
    outs += [out, oimp]
    out, oimp = _conv(gpu, lst, Wg, d["f"], importance=True, inp_importance=d["imp"], neighbors_importance=d["pimp"],
                      **kw)
    _close(out, L.reference(O, ref_lst, d["W"], d["f"], d["pimp"][keep], False))
    _close(oimp, _sum(ref_lst, d["pimp"][keep]))
    outs += [out, oimp]
    return outs


MAIN = L.main_lists()


@pytest.mark.parametrize("case", MAIN, ids=[lst.name for lst, _ in MAIN])
def test_both_algorithms_on_a_list(gpu, case):
    """scalar (algo = 1) and MFMA (algo = 2) kernel on one list, at one, two and three cin panels of the instance the
    launcher picks, three uses each"""
    lst, trio = case
    for cin, cout in trio:
        d = L.make_data(lst, cin, cout)
        _counts(gpu, reset=True)
        _three_ways(gpu, lst, d, algo=1)
        assert _counts(gpu) == {}
        _three_ways(gpu, lst, d, algo=2)
        counts = _counts(gpu)
        assert sum(counts.values()) == 3 and {k[2] for k in counts} == {0, 1}, counts
        assert all(k[1] == L.instance_kc(k[0], cin) and k[4] == 0 for k in counts), counts


FORCED = L.forced_lists()


@pytest.mark.parametrize("lst", FORCED, ids=[lst.name for lst in FORCED])
def test_forced_instances(gpu, lst):
    """every tile shape on one list, at 1, 2 and 3 (and more) panels of its depth; the variant counter proves the
    instance.  Plain convolutions: the bits of the first instance (a row's slots are accumulated in the same order
    whatever the tile); with importance: the reference."""
    for cin, cout in L.FORCED_WIDTHS:
        d = L.make_data(lst, cin, cout)
        ref = L.reference(O, lst, d["W"], d["f"], bias=d["bias"], relu=True, residual=d["res"])
        ref_imp = L.reference(O, lst, d["W"], d["f"], d["pimp"], True)
        first = None
        for nt, waves in L.FORCED_INSTANCES:
            _counts(gpu, reset=True)
            out, _ = _conv(gpu, lst, d["W"], d["f"], bias=d["bias"], relu=True, residual=d["res"], algo=2, force_nt=nt,
                           force_waves=waves)
            assert _counts(gpu) == {(nt, L.instance_kc(nt, cin), 0, waves, 0): 1}
            if first is None:
                first = out
                _close(out, ref)
            assert np.array_equal(out.view(np.uint32), first.view(np.uint32)), (cin, cout, nt, waves)
            _counts(gpu, reset=True)
            out, oimp = _conv(gpu, lst, d["W"], d["f"], importance=True, neighbors_importance=d["pimp"], normalize=True,
                              algo=2, force_nt=nt, force_waves=waves)
            assert _counts(gpu) == {(nt, L.instance_kc(nt, cin), 1, waves, 0): 1}
            _close(out, ref_imp)
            _close(oimp, _sum(lst, d["pimp"]))


@pytest.mark.parametrize("v", [65, 129])
def test_column_chunks_over_a_ragged_width(gpu, v):
    """cout = 132 in 16-column chunks (9 of them) and 32-column chunks (5): the last chunk is mostly padding, and with
    more than one chunk the grid is padded to a multiple of 8 row tiles whose blocks must leave at once"""
    lst = L.tile_edges(v)
    d = L.make_data(lst, 36, 132)
    first = None
    for nt, waves in ((1, 4), (2, 4), (2, 8)):
        _counts(gpu, reset=True)
        outs = _three_ways(gpu, lst, d, algo=2, force_nt=nt, force_waves=waves)
        assert sum(_counts(gpu).values()) == 3 and {(k[0], k[3]) for k in _counts(gpu)} == {(nt, waves)}
        first = outs if first is None else first
        assert np.array_equal(outs[0].view(np.uint32), first[0].view(np.uint32))


TWO_BANK = L.two_bank_lists()


@pytest.mark.parametrize("lst", TWO_BANK, ids=[lst.name for lst in TWO_BANK])
def test_two_banks(gpu, lst):
    """conv1a + conv1b in one launch: the bits of the two separate launches, both banks against the reference, empty
    rows give relu(bias) in either bank and an importance sum of 0"""
    empty = L.row_lengths(lst) == 0
    assert empty.any()
    for cin, ca in L.TWO_BANK_WIDTHS:
        da, db = L.two_bank_data(lst, cin, ca)
        nimp = da["imp"][lst.idx.astype(np.int64)]
        _counts(gpu, reset=True)
        out, oimp = _conv(gpu, lst, da["W"], da["f"], importance=True, inp_importance=da["imp"], normalize=True,
                          bias=da["bias"], relu=True, filters_b=db["W"], bias_b=db["bias"], algo=2)
        counts = _counts(gpu)
        assert sum(counts.values()) == 1 and all(k[2] == 1 and k[4] == 1 for k in counts), counts
        oa, _ = _conv(gpu, lst, da["W"], da["f"], bias=da["bias"], relu=True, algo=2)
        ob, oimp_b = _conv(gpu, lst, db["W"], da["f"], importance=True, inp_importance=da["imp"], normalize=True,
                           bias=db["bias"], relu=True, algo=2)
        assert np.array_equal(out[:, :ca].view(np.uint32), oa.view(np.uint32))
        assert np.array_equal(out[:, ca:].view(np.uint32), ob.view(np.uint32))
        assert np.array_equal(oimp.view(np.uint32), oimp_b.view(np.uint32))
        _close(out[:, :ca], L.reference(O, lst, da["W"], da["f"], bias=da["bias"], relu=True))
        _close(out[:, ca:], L.reference(O, lst, db["W"], da["f"], nimp, True, bias=db["bias"], relu=True))
        _close(oimp, _sum(lst, nimp))
        assert np.array_equal(out[empty, :ca], np.broadcast_to(np.maximum(da["bias"], 0), (empty.sum(), ca)))
        assert np.array_equal(out[empty, ca:], np.broadcast_to(np.maximum(db["bias"], 0), (empty.sum(), 8)))
        assert np.all(oimp[empty] == 0)


ZERO_SUM = L.zero_sum_lists()


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("lst", ZERO_SUM, ids=[lst.name for lst in ZERO_SUM])
def test_zero_importance_sums(gpu, lst, algo):
    """normalize with an importance sum of exactly 0 -- all importances 0.0, +0.5 / -0.5 pairs, an empty row: the
    contract of both kernels is the undivided sum (and 0 as the importance sum)"""
    cin, cout = 36, 20
    d = L.make_data(lst, cin, cout)
    w = L.zero_sum_importance(lst)
    out, oimp = _conv(gpu, lst, d["W"], d["f"], importance=True, neighbors_importance=w, normalize=True,
                      bias=d["bias"], algo=algo)
    sums = _sum(lst, w)
    zero = (np.arange(len(sums)) % 3 != 2) | (L.row_lengths(lst) == 0)
    assert np.all(sums[zero] == 0) and np.all(sums[~zero] > 0) and zero.any() and (~zero).any()
    assert np.all(oimp[zero] == 0)
    _close(oimp, sums)
    _close(out, L.reference(O, lst, d["W"], d["f"], w, True, bias=d["bias"]))
    # the undivided sum, stated without the oracle's own rule for a zero sum
    undivided = L.reference(O, lst, d["W"], d["f"], w, False, bias=d["bias"])
    _close(out[zero], undivided[zero])
    empty = L.row_lengths(lst) == 0
    assert np.array_equal(out[empty], np.broadcast_to(d["bias"], (empty.sum(), cout)))


ROW_LISTS = [L.tile_edges(65), L.striped()]


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("lst", ROW_LISTS, ids=[lst.name for lst in ROW_LISTS])
def test_row_lists(gpu, lst, algo):
    """row_perm only changes which block computes a row: a random permutation gives identical bits; with
    num_rows = v // 2 the rows that are not listed keep what `out` and `out_importance` held"""
    v = len(lst.rs) - 1
    d = L.make_data(lst, 36, 20)
    kw = dict(importance=True, inp_importance=d["imp"], normalize=True, bias=d["bias"], relu=True, algo=algo)
    out, oimp = _conv(gpu, lst, d["W"], d["f"], **kw)
    perm = np.random.default_rng(v).permutation(v).astype(np.int32)
    out_p, oimp_p = _conv(gpu, lst, d["W"], d["f"], row_perm=perm, **kw)
    assert np.array_equal(out_p.view(np.uint32), out.view(np.uint32))
    assert np.array_equal(oimp_p.view(np.uint32), oimp.view(np.uint32))
    out_h, oimp_h = _conv(gpu, lst, d["W"], d["f"], row_perm=perm, num_rows=v // 2, **kw)
    listed = np.zeros(v, bool)
    listed[perm[:v // 2]] = True
    assert np.array_equal(out_h[listed].view(np.uint32), out[listed].view(np.uint32))
    assert np.array_equal(oimp_h[listed].view(np.uint32), oimp[listed].view(np.uint32))
    assert np.all(out_h[~listed] == SENTINEL) and np.all(oimp_h[~listed] == SENTINEL)


@pytest.mark.parametrize("cin,cout,offset", [(6, 5, 0), (8, 6, 0), (8, 8, 1)], ids=["6x5", "8x6", "unaligned"])
def test_fallback_to_the_scalar_kernel(gpu, cin, cout, offset):
    """algo = 0 on widths and addresses the MFMA kernel does not take: odd widths, cout % 4 != 0, a feature matrix
    that starts one float after a 16-byte boundary.  No MFMA instance is counted and the values are the reference's."""
    assert (cin, cout) in L.FALLBACK_WIDTHS
    lst = L.tile_edges(65)
    d = L.make_data(lst, cin, cout)
    _counts(gpu, reset=True)
    _three_ways(gpu, lst, d, algo=0, feature_offset=offset)
    assert _counts(gpu) == {}
    if offset:  # the same call on an aligned matrix does take the MFMA kernel
        _three_ways(gpu, lst, d, algo=0)
        assert sum(_counts(gpu).values()) == 3


@pytest.mark.parametrize("algo", [0, 1, 2])
def test_all_rows_empty_and_no_rows(gpu, algo):
    """a list without a single pair is not an error: every row is relu(bias) with an importance sum of 0; a list
    without rows gives an empty tensor"""
    from asr_hip import ops
    lst = L.all_empty()
    cin, cout = 20, 36
    d = L.make_data(lst, cin, cout)
    out, oimp = _conv(gpu, lst, d["W"], d["f"], importance=True, inp_importance=d["imp"], normalize=True,
                      bias=d["bias"], relu=True, algo=algo)
    assert np.array_equal(out, np.broadcast_to(np.maximum(d["bias"], 0), out.shape)) and np.all(oimp == 0)
    out, _ = _conv(gpu, lst, d["W"], d["f"], residual=d["res"], algo=algo)
    assert np.array_equal(out, d["res"])
    none = L.SconvList("no rows", lst.idx, lst.slots, np.zeros(1, np.int64), lst.num_inp, 55)
    out, oimp = _conv(gpu, none, d["W"], d["f"], importance=True, inp_importance=d["imp"], bias=d["bias"], algo=algo)
    assert out.shape == (0, cout) and oimp.shape == (0,)
    got = ops.sparse_conv(_t(d["W"], gpu), _t(d["f"], gpu), _t(none.idx, gpu), _t(none.slots, gpu), _t(none.rs, gpu),
                          algo=algo)
    assert got.shape == (0, cout)


@pytest.mark.parametrize("algo", [1, 2])
def test_out_of_range_slots_are_skipped(gpu, algo):
    """an entry whose slot is >= kernel_size is skipped by both kernels, its importance included: the result is the
    one of the list without those entries.  The filter tensor is allocated with K + 8 slots (the extra ones hold 100)
    and the call passes filters[:K], so that no kernel reads outside an allocation."""
    lst = L.out_of_range_slots()
    valid, keep = L.without_out_of_range(lst)
    K = lst.kernel_size
    for cin, cout in L.WIDTH_TRIOS[0]:
        d = L.make_data(valid, cin, cout)
        d["pimp"] = L.out_of_range_pair_importance(lst, cin)
        wide = torch.full((K + 8, cin, cout), 100.0, dtype=torch.float32, device=gpu)
        wide[:K] = _t(d["W"], gpu)
        _three_ways(gpu, lst, d, ref_lst=valid, keep=keep, W=wide[:K], algo=algo)


DUPLICATES = [L.duplicates(), L.duplicates55()]


@pytest.mark.parametrize("lst", DUPLICATES, ids=[lst.name for lst in DUPLICATES])
def test_scalar_kernel_sums_repeated_slots(gpu, lst):
    """asr_hip.ops.sparse_conv leaves the duplicate-slot precondition of algo 0 / 2 to its caller (nothing is asserted
    about those on such a list); algo = 1 takes any list"""
    assert L.rows_with_duplicates(lst.slots, lst.rs) > 0
    _three_ways(gpu, lst, L.make_data(lst, 32, 32), algo=1)


def _facade(gpu, lst, d, imp, normalize, grad=None):
    import open3d.ml.torch as ml3d
    empty = torch.empty((0,), dtype=torch.float32, device=gpu)
    f = _t(d["f"], gpu).requires_grad_(grad is not None)
    W = _t(d["W"], gpu).requires_grad_(grad is not None)
    out = ml3d.ops.sparse_conv(filters=W, inp_features=f, inp_importance=empty, neighbors_index=_t(lst.idx, gpu),
                               neighbors_kernel_index=_t(lst.slots, gpu),
                               neighbors_importance=_t(imp, gpu) if imp is not None else empty,
                               neighbors_row_splits=_t(lst.rs, gpu), normalize=normalize)
    if grad is not None:
        out.backward(_t(grad, gpu))
        return out.detach().cpu().numpy(), f.grad.cpu().numpy(), W.grad.cpu().numpy()
    return out.cpu().numpy()


@pytest.mark.parametrize("lst", DUPLICATES, ids=[lst.name for lst in DUPLICATES])
def test_facade_forward_sums_repeated_slots(gpu, lst):
    """open3d::sparse_conv sums the neighbours of a row that share a slot; the facade finds such a list and sends it
    to the kernel that does"""
    d = L.make_data(lst, 32, 32)
    _counts(gpu, reset=True)
    for imp, normalize in ((None, False), (d["pimp"], True), (None, True), (d["pimp"], False)):
        ones = np.ones(len(lst.idx), np.float32) if normalize and imp is None else imp  # count normalisation
        _close(_facade(gpu, lst, d, imp, normalize), L.reference(O, lst, d["W"], d["f"], ones, normalize))
    assert _counts(gpu) == {}  # the scalar kernel


@pytest.mark.parametrize("with_imp,normalize", [(False, False), (True, True), (False, True), (True, False)])
def test_facade_backward_on_a_list_whose_transpose_repeats_slots(gpu, with_imp, normalize):
    """the feature gradient is the forward operator on the transposed list; two outputs that read one input through
    the same slot make that list name a slot twice although the forward list never does.  Against torch autograd over
    the dense fp64 restatement, gradient tolerance as in test_sparse_conv_backward_against_torch_autograd."""
    lst = L.transposed_duplicates()
    cin, cout = 32, 32
    d = L.make_data(lst, cin, cout)
    gout = np.random.default_rng(11).standard_normal((len(lst.rs) - 1, cout)).astype(np.float32)
    imp = d["pimp"] if with_imp else None
    _counts(gpu, reset=True)
    out, f_grad, W_grad = _facade(gpu, lst, d, imp, normalize, grad=gout)
    assert sum(_counts(gpu).values()) == 1  # forward: MFMA kernel; transposed list: scalar kernel
    ref, f_ref, W_ref = L.dense_autograd_reference(d["f"], d["W"], lst.idx, lst.slots, lst.rs, imp, normalize, gout)
    _close(out, ref)
    _close(f_grad, f_ref, 2e-5, 2e-5)
    _close(W_grad, W_ref, 2e-5, 2e-5)


@pytest.mark.parametrize("waves", [4, 8])
def test_a_wave_skips_the_slots_none_of_its_rows_name(gpu, waves):
    """striped(): the 16 rows of every wave use a slot set of their own.  A wave issues MFMAs only for the slots of its
    own rows (wmask), so a non-finite filter at a slot of ANOTHER wave's stripe cannot reach it -- the probe for the
    skip, which no finite value can see (a skipped step would only add zeros).  Rows of the stripe that owns the
    poisoned slot are not looked at at all: inside one wave the zero-line operand lets a NaN through, which is known, and
    what non-finite filters do to the rows that use them is no contract of this test."""
    lst = L.striped()
    cin, cout = 36, 20
    d = L.make_data(lst, cin, cout)
    ref = L.reference(O, lst, d["W"], d["f"], bias=d["bias"])
    for stripe, slots in enumerate(L.STRIPES):
        if not slots:
            continue
        W = d["W"].copy()
        W[list(slots)] = np.nan
        out, _ = _conv(gpu, lst, W, d["f"], bias=d["bias"], algo=2, force_nt=2, force_waves=waves)
        other = np.ones(len(ref), bool)
        other[16 * stripe:16 * stripe + 16] = False
        assert np.all(np.isfinite(out[other])), "stripe %d reached another wave" % stripe
        _close(out[other], ref[other])
