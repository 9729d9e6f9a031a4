"""tests/xlink_ref.py, the plain-Python restatement of the cross-class track linking, pinned by hand-worked
answers: every number below was worked out from the definition, not read off the code."""
import math

import pytest

import stitch_ref
import xlink_ref
from track_cases import result

BOX = [100.0, 50.0, 40.0, 30.0]


def job(pairs, prio=0, motion='hold'):
    return {'pairs': pairs, 'prio': prio, 'motion': motion}


def on(g=1, t=0.3):
    return {'max_link': g, 'link_iou': t}


def test_cyclist_pedestrian_cyclist_becomes_one_cyclist():
    rows = [(f, 4, BOX, 0.9, 7) for f in (0, 1, 2)] + [(f, 2, BOX, 0.9, 8) for f in (3, 4)] + [(f, 4, BOX, 0.9, 9) for f in (5, 6, 7)]
    got = xlink_ref.xlink([0, 8], result(rows), job({(2, 4): on(1)}))
    assert got['object_id'] == [7] * 8 and got['category'] == [4] * 8                        # six rows of class 4 against two of class 2
    assert got['n_relabelled'] == [2] and got['n_links'] == [2]
    assert got['links'] == [(7, 8, 1, 1.0), (8, 9, 1, 1.0)]
    assert got['pred'] == [-1, 0, 1] and got['root'] == [0, 0, 0] and got['affinity'] == [-1.0, 1.0, 1.0] and got['cls'] == [4, 4, 4]
    assert got['row_root'] == [0] * 8 and got['traj_offsets'] == [0, 3]
    # with the pair off nothing happens at all
    off = xlink_ref.xlink([0, 8], result(rows), job({}))
    assert off['object_id'] == [7, 7, 7, 8, 8, 9, 9, 9] and off['category'] == [4, 4, 4, 2, 2, 4, 4, 4] and off['n_links'] == [0] and off['n_relabelled'] == [0]
    assert off['cls'] == [4, 2, 4] and off['root'] == [0, 1, 2]


def test_two_rows_against_two_rows_is_decided_by_prio_then_by_the_roots_class():
    rows = [(0, 2, BOX, 0.9, 1), (1, 2, BOX, 0.9, 1), (2, 4, BOX, 0.9, 2), (3, 4, BOX, 0.9, 2)]
    res = result(rows)
    assert xlink_ref.xlink([0, 4], res, job({(2, 4): on()}))['category'] == [2] * 4             # equal prio: the root's class
    assert xlink_ref.xlink([0, 4], res, job({(2, 4): on()}, prio=[0, 0, 0, 1]))['category'] == [4] * 4
    assert xlink_ref.xlink([0, 4], res, job({(2, 4): on()}, prio=[0, 1, 0, 0]))['category'] == [2] * 4
    assert xlink_ref.xlink([0, 4], res, job({(2, 4): on()}, prio=3))['category'] == [2] * 4        # one value: the same for every class
    swapped = result([(r[0], 6 - r[1], r[2], r[3], r[4]) for r in rows])                     # the root is the class-4 piece now
    assert xlink_ref.xlink([0, 4], swapped, job({(2, 4): on()}))['category'] == [4] * 4
    # neither tied class is the root's: the lower class
    rows3 = [(0, 1, BOX, 0.9, 1)] + [(f, 4, BOX, 0.9, 2) for f in (1, 2)] + [(f, 2, BOX, 0.9, 3) for f in (3, 4)]
    got = xlink_ref.xlink([0, 5], result(rows3), job({(1, 4): on(), (2, 4): on()}))
    assert got['category'] == [2] * 5 and got['object_id'] == [1] * 5 and got['n_relabelled'] == [3]


def test_a_pair_that_is_off_and_an_unlisted_diagonal_do_not_link():
    rows = [(0, 1, BOX, 0.9, 1), (1, 2, BOX, 0.9, 2), (2, 2, BOX, 0.9, 3), (3, 4, BOX, 0.9, 4)]
    got = xlink_ref.xlink([0, 4], result(rows), job({(2, 4): on()}))
    assert got['links'] == [(3, 4, 1, 1.0)]                                                  # not 1 -> 2 (off), not 2 -> 3 ((2, 2) not listed)
    assert got['object_id'] == [1, 2, 3, 3] and got['category'] == [1, 2, 2, 2]
    got = xlink_ref.xlink([0, 4], result(rows), job({(2, 4): on(), (2, 2): on()}))
    assert got['links'] == [(2, 3, 1, 1.0), (3, 4, 1, 1.0)] and got['category'] == [1, 2, 2, 2]
    assert xlink_ref.xlink([0, 4], result(rows), job({(2, 4): on(0)}))['links'] == []           # max_link 0: the pair is off


def test_equal_affinities_in_two_classes_follow_the_order():
    # tail 0 (class 2); heads 1 (class 4) and 2 (class 2) at the same slot with the same box: (-a, n, i, j) picks head 1
    rows = [(0, 2, BOX, 0.9, 10), (1, 4, BOX, 0.9, 11), (1, 2, BOX, 0.9, 12)]
    both = {(2, 4): on(2), (2, 2): on(2)}
    assert xlink_ref.xlink([0, 3], result(rows), job(both))['links'] == [(10, 11, 1, 1.0)]
    rows = [(0, 2, BOX, 0.9, 10), (1, 2, BOX, 0.9, 12), (1, 4, BOX, 0.9, 11)]                # the class-2 head appears first now
    assert xlink_ref.xlink([0, 3], result(rows), job(both))['links'] == [(10, 12, 1, 1.0)]
    # the smaller gap before the smaller index
    rows = [(0, 2, BOX, 0.9, 10), (1, 2, BOX, 0.9, 12), (2, 4, BOX, 0.9, 11)]
    got = xlink_ref.xlink([0, 3], result(rows), job({(2, 4): on(2)}))
    assert got['links'] == [(12, 11, 1, 1.0)]                                                # 12 -> 11 at n = 1 beats 10 -> 11 at n = 2
    # a higher affinity before a smaller gap
    rows = [(0, 2, BOX, 0.9, 10), (1, 2, [120.0, 50.0, 40.0, 30.0], 0.9, 12), (2, 4, BOX, 0.9, 11)]
    got = xlink_ref.xlink([0, 3], result(rows), job({(2, 4): on(2)}))
    assert got['links'] == [(10, 11, 2, 1.0)]


def test_threshold_equal_to_the_affinity_links_and_zero_affinity_never_does():
    a_box, b_box = [0.0, 0.0, 10.0, 10.0], [5.0, 0.0, 10.0, 10.0]                            # 50 of 150
    a = 50.0 / 150.0
    assert stitch_ref.iou_dd([0.0, 0.0, 10.0, 10.0], [5.0, 0.0, 15.0, 10.0]) == a
    rows = [(0, 2, a_box, 0.9, 1), (1, 4, b_box, 0.9, 2)]
    assert xlink_ref.xlink([0, 2], result(rows), job({(2, 4): on(1, a)}))['links'] == [(1, 2, 1, a)]
    assert xlink_ref.xlink([0, 2], result(rows), job({(2, 4): on(1, math.nextafter(a, 1.0))}))['links'] == []
    apart = [(0, 2, a_box, 0.9, 1), (1, 4, [10.0, 0.0, 10.0, 10.0], 0.9, 2)]                 # the boxes touch: a == 0
    for thr in (0.0, -1.0):
        assert xlink_ref.xlink([0, 2], result(apart), job({(2, 4): on(1, thr)}))['links'] == []


def test_linear_motion_is_stitchings():
    rows = [(0, 2, [0.0, 0.0, 10.0, 10.0], 0.9, 1), (1, 2, [4.0, 0.0, 10.0, 10.0], 0.9, 1), (3, 4, [12.0, 0.0, 10.0, 10.0], 0.9, 2)]
    assert xlink_ref.xlink([0, 4], result(rows), job({(2, 4): on(2, 0.5)}, motion='linear'))['links'] == [(1, 2, 2, 1.0)]
    assert xlink_ref.xlink([0, 4], result(rows), job({(2, 4): on(2, 0.5)}))['links'] == []      # held: 2 of 18


def test_refusals():
    res = result([(0, 2, BOX, 0.9, 1)])
    with pytest.raises(ValueError, match=r'pair \(4, 2\) is given twice'):
        xlink_ref.xlink([0, 1], res, job({(2, 4): on(), (4, 2): on()}))
    with pytest.raises(ValueError, match=r'pair \(2, 5\): classes are 1\.\.4'):
        xlink_ref.xlink([0, 1], res, job({(2, 5): on()}))
    with pytest.raises(ValueError, match='at most 16 classes'):
        xlink_ref.xlink([0, 1], res, job({(2, 4): on()}), n_classes=17)
    with pytest.raises(ValueError, match='max_link must be >= 0'):
        xlink_ref.xlink([0, 1], res, job({(2, 4): on(-1)}))
    with pytest.raises(ValueError, match='link_iou must not be NaN'):
        xlink_ref.xlink([0, 1], res, job({(2, 4): on(1, float('nan'))}))
    with pytest.raises(ValueError, match='one value, or one per class'):
        xlink_ref.xlink([0, 1], res, job({(2, 4): on()}, prio=[1, 2]))
    with pytest.raises(ValueError, match="motion must be 'hold' or 'linear'"):
        xlink_ref.xlink([0, 1], res, job({(2, 4): on()}, motion='kalman'))
    assert xlink_ref.xlink([0, 1], res, job({(16, 16): on()}), n_classes=16)['cls'] == [2]
