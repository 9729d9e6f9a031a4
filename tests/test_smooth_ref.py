"""tests/smooth_ref.py pinned with answers worked out by hand (no GPU): the reference the kernel is compared with bit for bit."""
import smooth_cases
import smooth_ref

DYADIC = [1.0, 0.5, 0.25, 0.125]


def rows_of_line(slots, oid=7, category=1):
    """an object moving 3 right and 2 down per slot while it grows by 1 and 4: integers"""
    return [(f, category, [10.0 + 3 * f, 50.0 - 2 * f, 20.0 + f, 30.0 + 4 * f], 0.9, oid) for f in slots]


def test_linear_integer_motion_with_holes_is_reproduced_exactly_under_dyadic_weights():
    slots = [0, 1, 2, 4, 5, 6, 7, 9, 10, 13, 14, 15, 16, 17]
    res = smooth_cases.result(rows_of_line(slots))
    out = smooth_ref.smooth([0, 18], res, smooth_cases.job(window=3, weights=DYADIC))
    assert out['bbox'] == res['bbox']                                  # every sum and product is an exact integer multiple of 1/8
    present = set(slots)
    expected = [sum(1 for d in (1, 2, 3) if f - d in present and f + d in present) for f in slots]
    assert out['pairs'] == expected and out['pairs'][:4] == [0, 1, 1, 2] and max(out['pairs']) == 2


def test_one_value_by_hand():
    # slots 0..4, values 1, 2, 4, 8, 16; W = 2, k = 1, 1/2, 1/4; at slot 2: (4 + (2 + 8) / 2 + (1 + 16) / 4) / (1 + 1 + 1/2) = 13.25 / 2.5
    values = dict(enumerate([1.0, 2.0, 4.0, 8.0, 16.0]))
    assert smooth_ref.smooth_value(values, 2, 2, DYADIC) == (13.25 / 2.5, 2)
    assert smooth_ref.smooth_value(values, 1, 2, DYADIC) == ((2.0 + 0.5 * 5.0) / 2.0, 1)
    assert smooth_ref.smooth_value(values, 0, 2, DYADIC) == (1.0, 0) and smooth_ref.smooth_value(values, 4, 2, DYADIC) == (16.0, 0)
    # a hole on one side at distance 1 leaves distance 2
    del values[1]
    assert smooth_ref.smooth_value(values, 2, 2, DYADIC) == ((4.0 + 0.25 * 17.0) / 1.5, 1)


def test_alternating_noise_shrinks_to_a_third_under_the_box_of_width_one():
    n = 9
    rows = [(f, 2, [100.0 + 6 * f + (2 if f % 2 == 0 else -2), 40.0, 30.0, 30.0], 0.9, 1) for f in range(n)]
    res = smooth_cases.result(rows)
    out = smooth_ref.smooth([0, n], res, smooth_cases.job(window=1, kernel='box'))
    errors = [out['bbox'][f][0] - (100.0 + 6 * f) for f in range(n)]
    assert errors[0] == 2.0 and errors[-1] == 2.0                      # the end rows are the input
    for f in range(1, n - 1):                                          # (e - e - e) / 3: the sign turns, the size is a third
        assert abs(errors[f] - (-2.0 / 3.0 if f % 2 == 0 else 2.0 / 3.0)) < 1e-12
    assert out['pairs'] == [0] + [1] * (n - 2) + [0]
    assert all(row[1:] == [40.0, 30.0, 30.0] for row in out['bbox'])


def test_class_parameters_streams_and_order():
    rows = rows_of_line(range(5), oid=1, category=1) + rows_of_line(range(5), oid=2, category=3)
    res = smooth_cases.result(rows)
    noisy = [list(b) for b in res['bbox']]
    noisy[2][0] += 9.0
    noisy[7][0] += 9.0
    res['bbox'] = noisy
    j = smooth_cases.job(window=[1, 1, 0, 1], kernel='box')
    out = smooth_ref.smooth([0, 5], res, j)
    assert out['bbox'][2][0] == res['bbox'][2][0] - 6.0 and out['bbox'][7] == res['bbox'][7]      # class 3 has window 0
    assert out['pairs'] == [0, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    # the caller's order does not matter
    perm = [3, 9, 0, 5, 2, 8, 1, 7, 4, 6]
    shuffled = dict((k, [v[i] for i in perm]) for k, v in res.items())
    again = smooth_ref.smooth([0, 5], shuffled, j)
    assert again['bbox'] == [out['bbox'][i] for i in perm] and again['pairs'] == [out['pairs'][i] for i in perm]
    # a stream boundary inside the run of slots splits the trajectory
    split = smooth_ref.smooth([0, 2, 5], res, j)
    assert split['pairs'] == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0]


def test_the_same_trajectory_twice_in_a_slot_is_refused():
    import pytest
    res = smooth_cases.result(rows_of_line([0, 1, 1]))
    with pytest.raises(ValueError, match='occurs twice in slot 1'):
        smooth_ref.smooth([0, 3], res, smooth_cases.job(window=1))


def test_kernels():
    import math
    assert smooth_ref.box(3) == [1.0, 1.0, 1.0]
    g = smooth_ref.gaussian(1.5, 4)
    assert g[0] == 1.0 and g[2] == math.exp(-4 / (2.0 * 1.5 * 1.5)) and g[3] < g[2] < g[1] < 1.0
