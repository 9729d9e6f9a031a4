"""CPU proof of tests/softnms_cases.py: every case's expected rows and counts equal the numpy float64 restatement of that file AND the C
oracle (oracle/softnms_oracle.c) bit for bit, the closed forms among them included; the builders are deterministic; the stated IoUs of the
dyadic chains are exact; and the cases hold what the GPU test relies on (which boxes the reference drops, which sizes change path)."""
from fractions import Fraction

import numpy as np
import pytest

import softnms_cases as S


def _assert_case_equal(name, what, exp_rows, exp_counts, rows, counts, offsets):
    assert np.array_equal(exp_counts, counts), (name, what, exp_counts.tolist(), counts.tolist())
    for g in range(len(counts)):
        a, b = int(offsets[g]), int(offsets[g]) + int(counts[g])
        assert np.array_equal(exp_rows[a:b], rows[a:b], equal_nan=True), (name, what, g)
        assert S.same_bits(exp_rows[a:b], rows[a:b]), (name, what, g, 'sign of zero')


@pytest.mark.parametrize('name', list(S.CASES))
def test_expected_equals_restatement_and_oracle(name, oracle):
    case = S.get(name)
    n, G = len(case.rows), len(case.offsets) - 1
    assert case.rows.dtype == np.float64 and case.rows.shape == (n, 5) and case.exp_rows.shape == (n, 5)
    assert case.offsets.dtype == np.int64 and case.offsets[0] == 0 and case.offsets[-1] == n and np.all(np.diff(case.offsets) >= 0)
    assert case.exp_counts.shape == (G,) and np.all(case.exp_counts <= np.diff(case.offsets))
    ref_rows, ref_counts = S.reference(case)
    _assert_case_equal(name, 'restatement', case.exp_rows, case.exp_counts, ref_rows, ref_counts, case.offsets)
    orc_rows, orc_counts = S.oracle_expected(oracle, case, 2)
    _assert_case_equal(name, 'oracle', case.exp_rows, case.exp_counts, orc_rows, orc_counts, case.offsets)
    again = S.CASES[name]()                                                              # deterministic
    assert S.same_bits(again.rows, case.rows) and np.array_equal(again.offsets, case.offsets)
    assert S.same_bits(again.exp_rows, case.exp_rows) and np.array_equal(again.exp_counts, case.exp_counts)


def test_closed_forms_are_where_the_geometry_allows():
    closed = [n for n in S.CASES if S.get(n).closed]
    assert 'issue_table' in closed and 'ties' in closed and 'touching_killer' in closed and 'far_killer' in closed
    assert all(('chain_%d' % k) in closed for k in S.CHAIN_LENGTHS) and all(('pairs_%d' % n) in closed for n in S.GROUP_SIZES)
    assert S.get('issue_table').exp_counts.tolist() == list(S.ISSUE_TABLE_COUNTS)


def test_dyadic_ious_are_exact():
    k, v = S.KILLER, S.VICTIM
    assert S.iou_exact(k, v) == Fraction(3, 4) and S.iou_exact(k, k) == 1                # weight 1/2, and IoU >= cut = 1: weight 0
    assert S.iou_exact((0, 0, 1, 4), (0, 0, 1, 3)) == Fraction(3, 4)                     # touching_killer: Q over V
    assert S.iou_exact((-4, 0, 4, 4), (0, 0, 1, 4)) == 0                                 # T touches Q
    assert S.iou_exact((0, 0, 256, 4), (64, 0, 192, 4)) == Fraction(3, 4)                # far_killer, and every window of sliding_rows
    for i in (0, 1, 64):
        assert S.iou_exact((0, 0, 256, 4), (i, 0, 192, 4)) == Fraction(3, 4)
    # the weight itself, in float64: (1 - 3/4) / (1 - 1/2) = 1/2 and (1 - 1) / (1 - 1/2) = 0 without rounding
    assert (1.0 - 12.0 / ((12.0 - 12.0) + 16.0)) / (1.0 - 0.5) == 0.5 and (1.0 - 16.0 / ((16.0 - 16.0) + 16.0)) / (1.0 - 0.5) == 0.0


def test_chain_scores():
    for k in S.CHAIN_LENGTHS:
        case = S.get('chain_%d' % k)
        assert case.exp_counts.tolist() == [k + 1]
        assert case.exp_rows[0, 0] == 1.0 and np.all(case.exp_rows[1:k, 0] == 0.0) and not np.signbit(case.exp_rows[1:k, 0]).any()
        assert Fraction(case.exp_rows[k, 0]) == Fraction(1, 2) ** (k + 1)                # 0.5 * 2^-k, exact
    z, nz = S.get('chain_zero_score').exp_rows[3, 0], S.get('chain_negative_zero_score').exp_rows[3, 0]
    assert z == 0.0 and not np.signbit(z) and nz == 0.0 and np.signbit(nz)
    assert S.get('chain_subnormal_score').exp_rows[4, 0] == 2.0 ** -1074
    assert S.get('chain_subnormal_to_zero').exp_rows[5, 0] == 0.0


def test_which_special_boxes_the_reference_drops():
    """Kept rows per (top, middle, bottom) group, by the rules above S.SPECIAL_SETS: 7 ordinary boxes + the surviving special ones; a NaN-area
    box drops everything ranked after it and is itself dropped unless it ranks first."""
    want = ('zero2_far', 'zero3_far', 'zero2_same', 'zero3_same', 'zero_w_vs_zero_h', 'zero1', 'underflow1', 'underflow2', 'overflow1',
            'overflow2', 'neg_w', 'neg_h', 'neg_both', 'neg_cancel', 'neg_cancel_reversed')           # exactly one special box survives
    for name in S.SPECIAL_SETS:
        for centre in (False, True):
            got = S.bad_geometry(name, centre).exp_counts.tolist()
            if name in want or (centre and name in ('pinf_w', 'pinf_h', 'ninf_w', 'ninf_h')):     # centre form: area +-inf, no NaN
                assert got == [8] * 3, (name, centre, got)
            else:
                assert got == [1, 7, 7], (name, centre, got)         # non-finite coordinate: first -> alone; else dropped by the box above it


def test_sizes_reach_both_kernels_and_every_chunk_shape():
    assert S.FAST_MAX_ROWS in S.GROUP_SIZES and S.FAST_MAX_ROWS + 1 in S.GROUP_SIZES and S.FAST_MAX_ROWS - 1 in S.GROUP_SIZES
    assert {1, 63, 64, 65, 255, 256, 257} <= set(S.GROUP_SIZES)
    for n in S.GROUP_SIZES:
        assert len(S.get('pairs_%d' % n).rows) == n and S.get('pairs_%d' % n).exp_counts.tolist() == [n]
    x1 = S.get('chain_65').rows[:, 1]
    assert len(x1) == 66 and np.all(x1 == x1[0])                                           # more than 64 equal x1
    t = S.get('touching_killer').rows
    assert len(t) == 66 and (t[:, 1] < 0).sum() == 64 and (t[:, 1] + t[:, 3])[t[:, 1] < 0].max() == 0.0 and t[t[:, 1] >= 0, 1].min() == 0.0
    f = S.get('far_killer').rows
    order = np.argsort(f[:, 1], kind='stable')
    assert f[order[0], 3] == 256.0 and f[order[-1], 3] == 192.0 and len(f) > 65          # killer in the first chunk, its victim in the second
    d = S.get('pairs_257_disjoint_chunks').rows
    xs = np.sort(d[:, 1])
    assert all(xs[c * 64 - 1] + 4 <= xs[c * 64] for c in range(1, 5))                    # consecutive chunks do not overlap in x
    m = S.get('mixed_launch')
    assert (np.diff(m.offsets) == 0).sum() >= 3 and np.isnan(m.rows[:, 0]).any() and (m.rows[:, 0] < 0).any()


def test_dispatch_edges():
    assert S.get('dispatch_cut_equals_thr').exp_counts.tolist()[2] == 1                  # IoU == cut: 0 / 0, dropped
    assert S.get('dispatch_cut_infinite').exp_counts.tolist() == [1, 1, 1]
    assert S.get('dispatch_thr_zero').exp_counts.tolist() == [7, 21, 2]
