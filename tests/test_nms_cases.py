"""CPU proof of tests/nms_cases.py: every closed-form keep mask equals the numpy float32 greedy NMS of that file AND the torch restatement
oracle.detops_ref.nms_sorted, the ladder IoUs are the stated fractions, and the knife-edge set holds what the GPU test relies on (pairs at
exactly the three float32 quotients around 0.5, enough of which change side when the products are fused into the sums)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import nms_cases as N
from oracle import detops_ref as R

# every code path of the builders (n below / at / above a period, a tile, L) at sizes the two CPU references walk in well under a second;
# the closed forms are functions of the row number alone, so the GPU sizes (N.COL_SIZES, N.ROW_SIZES) follow the same formula
CPU_SIZES = (1, 2, 3, 33, 64, 65, 129, 700)


def _both_references(case):
    greedy = N.greedy_nms_f32(case.boxes, case.idxs, case.thr)
    idxs = None if case.idxs is None else torch.from_numpy(case.idxs)
    oracle = R.nms_sorted(torch.from_numpy(case.boxes), idxs, case.thr).numpy()
    return greedy, oracle


@pytest.mark.parametrize('name', list(N.CASES))
def test_closed_form_equals_both_references(name):
    sizes = CPU_SIZES + ((2100,) if name.startswith('interleaved') else ())           # two full rounds of the 1000 interleaved ladders
    for n in sizes:
        case = N.CASES[name](n)
        assert case.boxes.shape == (n, 4) and case.boxes.dtype == np.float32 and case.keep.shape == (n,) and case.keep.dtype == bool
        assert case.idxs is None or (case.idxs.shape == (n,) and case.idxs.dtype == np.int32)
        greedy, oracle = _both_references(case)
        assert np.array_equal(case.keep, greedy), (name, n, np.nonzero(case.keep != greedy)[0][:8])
        assert np.array_equal(greedy, oracle), (name, n, np.nonzero(greedy != oracle)[0][:8])
        again = N.CASES[name](n)                                                        # deterministic
        assert np.array_equal(again.boxes, case.boxes, equal_nan=True) and np.array_equal(again.keep, case.keep)


def test_closed_form_at_the_largest_gpu_size():
    """The longest chain the GPU tests run (6209 rows), against the numpy reference (the torch one takes seconds at this size)."""
    for name in ('ladder2', 'ladder5', 'interleaved1000', 'degenerate_in_ladder'):
        case = N.CASES[name](N.ROW_SIZES[-1])
        assert np.array_equal(case.keep, N.greedy_nms_f32(case.boxes, case.idxs, case.thr)), name


@pytest.mark.parametrize('period', sorted(N.LADDERS))
def test_ladder_ious_are_the_stated_fractions(period):
    boxes = N.ladder(period + 3, period).boxes

    def iou(a, b):
        a, b = [Fraction(float(v)) for v in a], [Fraction(float(v)) for v in b]
        w, h = max(min(a[2], b[2]) - max(a[0], b[0]), 0), max(min(a[3], b[3]) - max(a[1], b[1]), 0)
        return w * h / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - w * h)

    stated = N.LADDER_IOUS[period]
    assert len(stated) == period
    for start in (0, 2):
        assert tuple(iou(boxes[start], boxes[start + d]) for d in range(1, period + 1)) == stated
    assert all(v > Fraction(1, 2) for v in stated[:-1]) and stated[-1] < Fraction(1, 2)   # k suppresses k+1 .. k+period-1, not k+period
    # far from the threshold: no rounding of the float32 sequence can move a decision
    assert min(abs(v - Fraction(1, 2)) for v in stated) > Fraction(1, 50)


def test_ladders_are_not_aligned_to_the_tile():
    assert 64 % 3 and 64 % 5
    for L in (64, 256, 1000):
        keep = N.interleaved_ladders(2 * L + 1, L).keep
        assert keep[:L].all() and not keep[L:2 * L].any() and keep[2 * L]


@pytest.mark.parametrize('name', N.CASES_WITH_NAN)
def test_no_decision_depends_on_how_max_and_min_treat_nan(name):
    """numpy / torch maximum propagate NaN, the kernel's fmaxf / fminf drop it: the masks are the same (module docstring)."""
    for n in (65, 700):
        case = N.CASES[name](n)
        assert np.isnan(case.boxes).any()
        assert np.array_equal(N.greedy_nms_f32(case.boxes, case.idxs, case.thr, nan_like_fmaxf=True), case.keep)


def test_degenerate_rows_cover_every_kind_and_stay_out_of_the_ladder():
    case = N.degenerate_in_ladder(700)
    b = case.boxes
    special = np.arange(700) % 7 == 3
    assert special.sum() >= 2 * N.N_DEGENERATE_KINDS
    with np.errstate(invalid='ignore'):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    assert (area[~special] == 100).all() and case.keep[special].all()
    assert (area[special] == 0).sum() >= 2 and (area[special] < 0).any() and np.isnan(area[special]).any() and np.isinf(area[special]).any()
    assert all(np.isnan(b[special][:, c]).any() for c in range(4))                       # a NaN in each coordinate
    # against every ladder row and every other special row the quotient is 0 (either sign) or NaN, in both directions
    for r in np.nonzero(special)[0]:
        others = np.delete(np.arange(700), r)
        for q in (N._quotient(b[r], b[others]), np.array([N._quotient(b[o], b[r:r + 1])[0] for o in others[::13]])):
            assert (np.isnan(q) | (q == 0)).all(), r


def test_extreme_group_ids_survive_the_int32_round_trip():
    g = N.extreme_groups(12).idxs
    assert g.dtype == np.int32 and g.min() == N.INT32_MIN and g.max() == N.INT32_MAX and (g < 0).any()
    assert len(set(g.tolist())) == len(N.EXTREME_GROUPS)


@pytest.mark.parametrize('per_class', [N.KNIFE_PAIRS_BELOW, N.KNIFE_PAIRS_ABOVE])
def test_knife_edge_pairs(per_class):
    case, flips = N.knife_edge(per_class)
    npairs = 3 * per_class
    assert case.boxes.shape == (2 * npairs, 4) and per_class >= N.KNIFE_MIN_PER_CLASS
    assert (2 * npairs <= 6144) == (per_class == N.KNIFE_PAIRS_BELOW)                    # one set for each single-problem sweep
    a, b = case.boxes[0::2], case.boxes[1::2]
    # the quotient of every pair is exactly the float32 value of its class (recomputed pair by pair with the reference's helper)
    q = np.array([N._quotient(a[p], b[p:p + 1])[0] for p in range(npairs)])
    for c, target in enumerate(N.KNIFE_QUOTIENTS):
        assert (q[c::3] == target).all() and len(q[c::3]) >= N.KNIFE_MIN_PER_CLASS
    assert N.KNIFE_QUOTIENTS[0] < 0.5 == N.KNIFE_QUOTIENTS[1] < N.KNIFE_QUOTIENTS[2]
    assert float(N.KNIFE_QUOTIENTS[2]) - float(N.KNIFE_QUOTIENTS[0]) == 2.0 ** -24 + 2.0 ** -25      # one ulp to each side
    # fractional coordinates whose products are not exact in float32
    assert (case.boxes != np.round(case.boxes)).mean() > 0.99 and case.boxes.min() >= 0 and case.boxes.max() < 2000 + 400 + 134
    # expectation: B goes only in class 2; both references agree
    assert case.keep[0::2].all() and np.array_equal(case.keep[1::2], np.arange(npairs) % 3 != 2)
    greedy, oracle = _both_references(case)
    assert np.array_equal(case.keep, greedy) and np.array_equal(greedy, oracle)
    # pairs that a contracted evaluation decides differently: the set can tell a contracted kernel from the reference
    print('knife-edge: %d pairs per class, %d of %d pairs change side under a fused form (per form: %s)' % (
        per_class, flips.sum(), npairs,
        ((N.fused_quotients(a, b) > N.HALF) != (np.arange(npairs) % 3 == 2)[None]).sum(axis=1).tolist()))
    assert flips.sum() >= N.KNIFE_MIN_FLIPS
    # fusing only ever moves a quotient by an ulp or so: the fused forms stay within the three values' neighbourhood
    assert np.abs(N.fused_quotients(a, b).astype(np.float64) - 0.5).max() < 4 * 2.0 ** -24
    # the smaller set is a prefix of the larger one's sampling order
    if per_class == N.KNIFE_PAIRS_BELOW:
        big = N.knife_edge(N.KNIFE_PAIRS_ABOVE)[0].boxes
        assert np.array_equal(big[:2 * npairs], case.boxes)
