"""tests/view_fusion_ref.py (the host composition wt_fuse_slots_dev is compared with) pinned on answers worked by hand: the cases
of tests/wbf_cases.py placed into wire slots, and the wsum case."""
import numpy as np
import pytest

from view_fusion_ref import WSUM_MIN_SCORE, WSUM_WEIGHTS, case_as_slots, host_fuse_slots, wsum_case
from wbf_cases import CASES


@pytest.mark.parametrize('name', sorted(CASES))
def test_hand_worked_cases_in_slots(name):
    rows, wsum, method, thr, exp_out, _, _ = CASES[name]
    xywhs, cat, weights = case_as_slots(rows, wsum)
    K, S = cat.shape
    filler = sum(1 for k in range(K) if (cat[k] == 2).any())
    assert K == wsum and filler == max(0, K - len(rows))
    ox, oc, on = host_fuse_slots(xywhs, cat, 1, S, weights, 2, method, thr, -np.inf)
    n = len(exp_out)
    assert on.tolist() == [n + filler]
    assert oc[:n].tolist() == [1] * n and oc[n:n + filler].tolist() == [2] * filler and not oc[n + filler:].any()
    exp = np.asarray(exp_out, np.float64)
    assert np.array_equal(ox[0:4, :n], exp[:, 1:5].T)
    assert np.array_equal(ox[4, :n], np.round(exp[:, 0], 5))
    assert not ox[:, n + filler:].any()


@pytest.mark.parametrize('method', ['weighted_fusion_b', 'nmw'])
def test_wsum_counts_views_with_a_kept_row_of_any_category(method):
    xywhs, cat, F, S, C, expected = wsum_case()
    got = host_fuse_slots(xywhs, cat, F, S, WSUM_WEIGHTS, C, method, 0.5, WSUM_MIN_SCORE)
    exp = expected[method]
    assert np.array_equal(got[2], exp[2])
    assert np.array_equal(got[1], exp[1])
    assert np.array_equal(got[0], exp[0])


def test_output_filter_is_strict_and_input_filter_is_not():
    """score * weight == min_score is kept on the way in (>=); conf == min_score is dropped on the way out (>)."""
    xywhs, cat = np.zeros((1, 5, 2)), np.zeros((1, 2), np.int32)
    xywhs[0, :, 0] = [0, 0, 10, 10, 0.25]
    xywhs[0, :, 1] = [50, 0, 10, 10, 0.5]
    cat[0] = 1
    ox, oc, on = host_fuse_slots(xywhs, cat, 1, 2, [1.0], 1, 'nmw', 0.5, 0.25)
    assert on.tolist() == [1] and ox[:, 0].tolist() == [50, 0, 10, 10, 0.5] and oc.tolist() == [1, 0]
