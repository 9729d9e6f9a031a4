"""Pins tests/hota_ref.py (the plain-Python restatement of DESIGN.md section 19) with hand-worked cases.  No GPU, no product code."""
import math

import pytest

import hota_ref

CLOSE = dict(rel=1e-14, abs=0.0)


def _gt(f, box, oid, cat=1, level=1):
    return {'image_id': 'seg/%d/FRONT' % f, 'bbox': box, 'category_id': cat, 'object_id': oid, 'tracking_difficulty_level': level}


def _hyp(f, box, oid, cat=1):
    return {'image_id': 'seg/%d/FRONT' % f, 'bbox': box, 'score': 1.0, 'category_id': cat, 'object_id': oid}


def test_alphas_are_the_19_quotients():
    assert hota_ref.ALPHAS[0] == 0.05 and hota_ref.ALPHAS[9] == 0.5 and hota_ref.ALPHAS[18] == 0.95 and len(hota_ref.ALPHAS) == 19
    assert hota_ref.ALPHAS[4] == 0.25 and hota_ref.ALPHAS[14] == 0.75


def test_case_1_split_trajectory():
    anns = [_gt(f, [0, 0, 10, 10], 'o') for f in range(4)]
    rows = [_hyp(f, [0, 0, 10, 10], 'a' if f < 2 else 'b') for f in range(4)]
    res = hota_ref.evaluate(anns, rows)
    for lv in (1, 2):
        row = res['table'][1][lv]
        assert row['tp'] == [4] * 19 and row['gt'] == 4 and row['hyp'] == 4
        assert row['sums']['ass'] == [2.0] * 19                 # two cells with c = 2: 2 * (2 / (4 + 2 - 2)) each
        assert row['DetA'] == 1.0 and row['AssA'] == pytest.approx(0.5, **CLOSE) and row['HOTA'] == pytest.approx(math.sqrt(0.5), **CLOSE)
        assert row['LocA'] == 1.0 and row['HOTA(0)'] == pytest.approx(math.sqrt(0.5), **CLOSE)
    assert res['table']['ALL'][2]['tp'] == [4] * 19


def test_case_2_iou_exactly_at_a_threshold():
    res = hota_ref.evaluate([_gt(0, [0, 0, 2, 1], 'o')], [_hyp(0, [0, 0, 1, 1], 'a')])
    assert hota_ref.iou(hota_ref.xyxy([0, 0, 2, 1]), hota_ref.xyxy([0, 0, 1, 1])) == 0.5
    row = res['table'][1][2]
    assert row['tp'] == [1] * 10 + [0] * 9
    for name in ('HOTA', 'DetA', 'AssA'):
        assert row[name] == pytest.approx(10 / 19, **CLOSE), name
    assert row['LocA'] == 0.5 and row['LocA(0)'] == 0.5
    assert math.isnan(row['per_alpha']['LocA'][10]) and row['per_alpha']['AssA'][10] == 0.0


def _self_result(anns):
    return [_hyp(int(a['image_id'].split('/')[1]), a['bbox'], a['object_id'], a['category_id']) for a in anns]


def test_case_3_ground_truth_against_itself():
    anns = [_gt(f, [30 * i + f, 5 * i, 20 + i, 25], 'o%d' % i, cat=1 + i % 2, level=1 + (i == 3)) for f in range(3) for i in range(5)]
    res = hota_ref.evaluate(anns, _self_result(anns))
    for c in (1, 2, 'ALL'):
        row = res['table'][c][2]
        assert row['HOTA'] == 1.0 and row['DetA'] == 1.0 and row['AssA'] == 1.0 and row['LocA'] == 1.0, c
        assert row['tp'] == [row['gt']] * 19 and row['gt'] == row['hyp'] > 0


def test_case_4_identity_swap():
    anns = [_gt(f, [100 * i, 0, 10, 10], 'o%d' % i) for f in range(4) for i in range(2)]
    rows = [_hyp(f, [100 * i, 0, 10, 10], 'h%d' % (i if f < 2 else 1 - i)) for f in range(4) for i in range(2)]
    row = hota_ref.evaluate(anns, rows)['table'][1][2]
    assert row['tp'] == [8] * 19 and row['DetA'] == 1.0
    for a in range(19):
        assert row['sums']['ass'][a] == pytest.approx(8 / 3, **CLOSE)
    assert row['AssA'] == pytest.approx(1 / 3, **CLOSE) and row['HOTA'] == pytest.approx(math.sqrt(1 / 3), **CLOSE)


def case_5():
    anns = [_gt(f, [0, 0, 10, 10], 'o') for f in range(3)]
    rows = [_hyp(f, [0, 0, 10, 8], 'a') for f in range(3)] + [_hyp(1, [0, 0, 10, 9], 'b')]
    return anns, rows


def test_case_5_alignment_beats_iou():
    anns, rows = case_5()
    res = hota_ref.evaluate(anns, rows)
    row = res['table'][1][2]
    assert res['matches'][2] == {0: 0, 1: 1, 2: 2}              # frame 1 goes to `a` (result row 1), not to `b` (row 3) with the higher IoU
    assert row['gt'] == 3 and row['hyp'] == 4 and row['tp'] == [3] * 16 + [0] * 3
    assert row['HOTA'] == pytest.approx(16 / 19 * math.sqrt(0.75), **CLOSE)
    assert row['DetA'] == pytest.approx(16 / 19 * 0.75, **CLOSE) and row['AssA'] == pytest.approx(16 / 19, **CLOSE)
    assert row['LocA'] == pytest.approx(0.8, **CLOSE)


def test_case_6_level_1_is_level_2_of_the_filtered_input():
    anns, rows = [], []
    for f in range(3):
        anns += [_gt(f, [0, 0, 20, 20], 'counted'), _gt(f, [100, 0, 20, 20], 'dontcare', level=2)]
        rows += [_hyp(f, [1, 0, 20, 20], 'h0'), _hyp(f, [101, 1, 20, 20], 'h1'), _hyp(f, [300, 0, 20, 20], 'clutter')]
    res = hota_ref.evaluate(anns, rows)
    assert res['removed'][1] == {1, 4, 7} and res['removed'][2] == set()
    without = hota_ref.evaluate([a for a in anns if a['object_id'] != 'dontcare'], [r for r in rows if r['object_id'] != 'h1'])
    drop = lambda row: dict((k, v) for k, v in row.items() if k != 'per_alpha')
    assert repr(drop(res['table'][1][1])) == repr(drop(without['table'][1][2]))
    assert res['table'][1][1]['gt'] == 3 and res['table'][1][2]['gt'] == 6 and res['table'][1][1]['hyp'] == 6
    # a hypothesis that reaches a counted box as well stays at LEVEL_1
    anns2 = anns + [_gt(0, [102, 0, 20, 20], 'counted_too')]
    assert hota_ref.evaluate(anns2, rows)['removed'][1] == {4, 7}


def test_nan_where_a_denominator_is_zero():
    none = hota_ref.evaluate([_gt(0, [0, 0, 10, 10], 'o')], [])['table']
    assert none[1][2]['DetA'] == 0.0 and none[1][2]['DetRe'] == 0.0 and math.isnan(none[1][2]['DetPr']) and math.isnan(none[1][2]['LocA'])
    assert none[1][2]['HOTA'] == 0.0 and none[1][2]['AssA'] == 0.0
    assert all(math.isnan(none[2][2][n]) for n in ('HOTA', 'DetA', 'DetRe', 'DetPr', 'LocA'))        # a class without rows
    only_hyp = hota_ref.evaluate({'annotations': [], 'images': [{'id': 'seg/0/FRONT'}]}, [_hyp(0, [0, 0, 10, 10], 'a')])['table'][1][2]
    assert only_hyp['DetPr'] == 0.0 and math.isnan(only_hyp['DetRe']) and only_hyp['DetA'] == 0.0
