"""Known answers, computed by hand, that pin tests/refine_ref.py (the restatement the GPU tests compare with)."""
import refine_ref
from refine_cases import job, result


def test_three_slot_gap_in_thirds():
    rows = [(0, 1, [0.0, 3.0, 30.0, 9.0], 0.25, 4), (3, 1, [3.0, 0.0, 60.0, 9.0], 1.0, 4)]
    r = refine_ref.refine([0, 4], result(rows), job(max_gap=2))
    assert r['frame'] == [0, 1, 2, 3] and r['source'] == [0, -2, -2, 1] and r['object_id'] == [4] * 4 and r['category'] == [1] * 4
    third, two_thirds = 1.0 / 3.0, 2.0 / 3.0
    assert r['bbox'][1] == [0.0 + 3.0 * third, 3.0 + (-3.0) * third, 30.0 + 30.0 * third, 9.0]
    assert r['bbox'][2] == [0.0 + 3.0 * two_thirds, 3.0 + (-3.0) * two_thirds, 30.0 + 30.0 * two_thirds, 9.0]
    assert r['bbox'][1] == [1.0, 2.0, 40.0, 9.0] and r['bbox'][2] == [2.0, 1.0, 50.0, 9.0]
    assert r['score'] == [0.25, 0.25 + 0.75 * third, 0.25 + 0.75 * two_thirds, 1.0] == [0.25, 0.5, 0.75, 1.0]
    assert r['frame_row_offsets'] == [0, 1, 2, 3, 4]


def test_mean_adds_in_slot_order():
    # (0.1 + 0.2) + 0.3 = 0.6000000000000001, 0.1 + (0.2 + 0.3) = 0.6: the rows come in with the slots out of order
    rows = [(2, 1, [0, 0, 5, 5], 0.3, 1), (0, 1, [0, 0, 5, 5], 0.1, 1), (1, 1, [0, 0, 5, 5], 0.2, 1)]
    r = refine_ref.refine([0, 3], result(rows), job(score_mode='mean'))
    assert (0.1 + 0.2) + 0.3 == 0.6000000000000001 and 0.1 + (0.2 + 0.3) == 0.6
    assert r['score'] == [0.6000000000000001 / 3.0] * 3 and r['source'] == [1, 2, 0]
    assert 0.6000000000000001 / 3.0 != 0.6 / 3.0
    keep = refine_ref.refine([0, 3], result(rows), job())
    assert keep['score'] == [0.1, 0.2, 0.3]


def test_length_below_and_at_min_len():
    rows = [(0, 1, [0, 0, 5, 5], 0.5, 1), (0, 1, [9, 9, 5, 5], 0.5, 2), (1, 1, [0, 0, 5, 5], 0.5, 1), (1, 1, [9, 9, 5, 5], 0.5, 2),
            (2, 1, [9, 9, 5, 5], 0.5, 2)]
    r = refine_ref.refine([0, 3], result(rows), job(min_len=3))
    assert r['object_id'] == [2, 2, 2] and r['source'] == [1, 3, 4] and r['frame_row_offsets'] == [0, 1, 2, 3]
    assert refine_ref.refine([0, 3], result(rows), job(min_len=2))['source'] == [0, 1, 2, 3, 4]
    assert refine_ref.refine([0, 3], result(rows), job(min_len=4))['source'] == []


def test_gap_of_max_gap_and_one_more():
    rows = [(0, 2, [0, 0, 4, 4], 0.5, 1), (0, 2, [8, 8, 4, 4], 0.5, 2), (3, 2, [4, 4, 4, 4], 0.5, 2), (4, 2, [8, 8, 12, 4], 0.5, 1)]
    r = refine_ref.refine([0, 5], result(rows), job(max_gap=2))
    assert r['frame'] == [0, 0, 1, 2, 3, 4] and r['source'] == [0, 1, -3, -3, 2, 3]              # 2 holes filled, 3 holes not
    r = refine_ref.refine([0, 5], result(rows), job(max_gap=3))
    assert r['frame'] == [0, 0, 1, 1, 2, 2, 3, 3, 4] and r['source'] == [0, 1, -4, -3, -4, -3, 2, -4, 3]
    assert r['bbox'][2] == [2.0, 2.0, 6.0, 4.0] and r['bbox'][4] == [4.0, 4.0, 8.0, 4.0] and r['bbox'][7] == [6.0, 6.0, 10.0, 4.0]
    assert refine_ref.refine([0, 5], result(rows), job(max_gap=1))['source'] == [0, 1, 2, 3]


def test_identity_setting_reproduces_the_input():
    rows = [(0, 1, [0.1, 0.2, 4.5, 4.25], 0.5, 1), (0, 3, [8, 8, 4, 4], 0.25, 2), (2, 1, [4, 4, 4, 4], 0.125, 2)]
    r = refine_ref.refine([0, 1, 3], result(rows), job())
    for name, v in result(rows).items():
        assert r[name] == v
    assert r['source'] == [0, 1, 2] and r['frame_row_offsets'] == [0, 2, 2, 3]
