"""tests/wbf_ref.py - the restatement of weighted boxes fusion / NMW that the HIP kernel is compared with - pinned by hand-worked
cases in exact (dyadic) arithmetic.  The cases (tests/wbf_cases.py) also run through the kernel in tests/test_gpu_wbf.py."""
import pytest

import wbf_ref as R
from wbf_cases import CASES

@pytest.mark.parametrize('name', sorted(CASES))
def test_hand_worked_case(name):
    rows, wsum, method, thr, out, members, row_cluster = CASES[name]
    got = R.fuse_xyxy(rows, wsum, method, thr)
    assert got[0] == [[float(v) for v in r] for r in out]
    assert got[1] == members and got[2] == row_cluster


def test_the_ious_the_cases_rest_on():
    assert R.iou([0, 0, 10, 10], [2, 0, 12, 10]) == 80 / 120
    assert R.iou([0, 0, 10, 10], [5, 0, 15, 10]) == 50 / 150 and R.iou([2, 0, 12, 10], [5, 0, 15, 10]) == 70 / 130
    assert R.iou([0, 0, 3, 1], [1, 0, 4, 1]) == 0.5
    assert R.iou([0, 0, 4, 4], [2, 0, 10, 4]) == R.iou([8, 0, 12, 4], [2, 0, 10, 4]) == 0.2
    assert R.iou([0, 0, 10, 10], [10, 0, 20, 10]) == 0.0 and R.iou([0, 0, 10, 10], [30, 30, 40, 40]) == 0.0
    assert R.iou([3, 4, 8, 9], [3, 4, 8, 9]) == 1.0


def test_packed_form_equals_the_group_form():
    rows = [[0.75, 0, 0, 10, 10], [0.25, 2, 0, 10, 10], [0.5, 40, 40, 10, 10], [0.5, 1, 1, 2, 2]]       # [score, x, y, w, h]
    out5, counts, members, row_cluster = R.fuse_groups(rows, [0, 3, 3, 4], [2, 1, 1], 'weighted_fusion', 0.5)
    assert counts.tolist() == [2, 0, 1]
    assert out5.tolist() == [[0.5, 0.5, 0, 10, 10], [0.25, 40, 40, 10, 10], [0, 0, 0, 0, 0], [0.5, 1, 1, 2, 2]]
    assert members.tolist() == [2, 1, 0, 1] and row_cluster.tolist() == [0, 0, 1, 0]


def _row(image, category, score, bbox):
    return {'image_id': image, 'category_id': category, 'bbox': bbox, 'score': score}


def test_wsum_counts_the_inputs_of_all_categories_of_the_image():
    """Input C contributes to image p only in category 2: it still counts in the wsum of p's category 1.  Input B's only row in
    image q has zero width: B does not count there."""
    a = [_row('p', 1, 0.75, [0, 0, 10, 10]), _row('p', 2, 0.5, [40, 40, 10, 10]), _row('q', 1, 0.5, [0, 0, 4, 4])]
    b = [_row('p', 1, 0.25, [2, 0, 10, 10]), _row('q', 1, 0.9, [0, 0, 0, 4])]
    c = [_row('p', 2, 0.25, [40, 40, 10, 10])]
    got = R.ensemble_rows([a, b, c], 'weighted_fusion', 0.5)
    assert got == [_row('p', 1, round(((1.0 / 2) * 2) / 3, 5), [0.5, 0.0, 10.0, 10.0]),       # wsum 3, 2 members
                   _row('p', 2, 0.25, [40.0, 40.0, 10.0, 10.0]),                                # ((0.75 / 2) * 2) / 3
                   _row('q', 1, 0.5, [0.0, 0.0, 4.0, 4.0])]                                     # wsum 1
    assert got[0]['score'] == 0.33333
    # without input C the same cluster scores ((1 / 2) * 2) / 2
    assert R.ensemble_rows([a, b], 'weighted_fusion', 0.5)[0]['score'] == 0.5


def test_explicit_weights_scale_scores_and_wsum():
    a = [_row('p', 1, 0.5, [0, 0, 8, 8])]
    b = [_row('p', 1, 0.5, [0, 0, 8, 8]), _row('p', 1, 0.25, [100, 0, 8, 8])]
    got = R.ensemble_rows([a, b], 'weighted_fusion', 0.5, weights=[2, 1])
    # scores 1.0 and 0.5, wsum 3: ((1.5 / 2) * 2) / 3 = 0.5; the lone box ((0.25 / 1) * 1) / 3
    assert [r['score'] for r in got] == [0.5, round(0.25 / 3, 5)]
    assert got[0]['bbox'] == [0.0, 0.0, 8.0, 8.0]


def test_rows_of_an_image_are_sorted_across_categories():
    a = [_row('r', 2, 0.5, [0, 0, 8, 8]), _row('r', 1, 0.5, [0, 0, 8, 8]), _row('r', 1, 0.75, [100, 0, 8, 8]), _row('r', 3, 0.625, [0, 0, 8, 8])]
    got = R.ensemble_rows([a, []], 'nmw', 0.5)
    assert [(r['category_id'], r['score']) for r in got] == [(1, 0.75), (3, 0.625), (1, 0.5), (2, 0.5)]


def test_non_finite_input_is_refused():
    with pytest.raises(ValueError):
        R.ensemble_rows([[_row('p', 1, float('nan'), [0, 0, 8, 8])], []])
    with pytest.raises(ValueError):
        R.ensemble_rows([[_row('p', 1, 0.5, [0, float('inf'), 8, 8])], []])


def test_random_groups_cluster_the_way_an_ensemble_does():
    dets5, offsets, wsum = R.random_groups(7)
    assert len(offsets) == 201 and (offsets[1:] == offsets[:-1]).any() and dets5[:, 3:].min() > 0
    _, counts, members, _ = R.fuse_groups(dets5, offsets, wsum, 'weighted_fusion', 0.5)
    m = [int(members[o + j]) for o, c in zip(offsets[:-1].tolist(), counts.tolist()) for j in range(c)]
    print('clusters %d, with more than one member %d, with more than 3 members %d' % (len(m), sum(v > 1 for v in m), sum(v > 3 for v in m)))
    assert sum(m) == len(dets5) and sum(v > 1 for v in m) >= 0.3 * len(m) and max(m) > 3
