"""tests/stitch_ref.py pinned with answers computed by hand."""
import stitch_ref
from stitch_cases import job, result


def stitched(rows, offsets, **kw):
    return stitch_ref.stitch(offsets, result(rows), job(**kw))


# one object, [x, 0, 10, 10], moving 2 per slot: seen at slots 0, 1 as id 7, missed at 2, 3, seen at 4, 5 as id 9
TWO_PIECES = [(0, 1, [0.0, 0.0, 10.0, 10.0], 0.9, 7), (1, 1, [2.0, 0.0, 10.0, 10.0], 0.9, 7),
              (4, 1, [8.0, 0.0, 10.0, 10.0], 0.9, 9), (5, 1, [10.0, 0.0, 10.0, 10.0], 0.9, 9)]


def test_two_pieces_under_hold_and_linear():
    # hold: [2, 12] against [8, 18]: overlap 4 of union 16 -> 40 / 160
    s = stitched(TWO_PIECES, [0, 6], max_link=3, link_iou=0.25)
    assert s['object_id'] == [7, 7, 7, 7] and s['links'] == [(7, 9, 3, 0.25)]
    assert s['pred'] == [-1, 0] and s['root'] == [0, 0] and s['affinity'] == [-1.0, 0.25] and s['row_root'] == [0, 0, 0, 0] and s['n_links'] == [1]
    assert stitched(TWO_PIECES, [0, 6], max_link=3, link_iou=0.26)['object_id'] == [7, 7, 9, 9]
    # linear: 2 + ((2 - 0) / 1) * 3 = 8: the head's box exactly
    s = stitched(TWO_PIECES, [0, 6], max_link=3, link_iou=0.26, motion='linear')
    assert s['object_id'] == [7, 7, 7, 7] and s['links'] == [(7, 9, 3, 1.0)]
    # a single observation is held, whatever the motion
    s = stitched(TWO_PIECES[1:], [0, 6], max_link=3, link_iou=0.25, motion='linear')
    assert s['links'] == [(7, 9, 3, 0.25)]


def test_gap_equal_to_max_link_links_and_one_more_does_not():
    assert stitched(TWO_PIECES, [0, 6], max_link=3, link_iou=0.1)['n_links'] == [1]
    assert stitched(TWO_PIECES, [0, 6], max_link=2, link_iou=0.1)['n_links'] == [0]
    s = stitched(TWO_PIECES, [0, 6], max_link=0, link_iou=0.0)
    assert s['object_id'] == [7, 7, 9, 9] and s['pred'] == [-1, -1] and s['root'] == [0, 1] and s['row_root'] == [0, 0, 1, 1]
    # consecutive slots: n = 1
    rows = [(0, 1, [0.0, 0.0, 10.0, 10.0], 0.9, 1), (1, 1, [0.0, 0.0, 10.0, 10.0], 0.9, 2)]
    assert stitched(rows, [0, 2], max_link=1)['links'] == [(1, 2, 1, 1.0)]
    # the same slot is no gap: n = 0
    rows = [(0, 1, [0.0, 0.0, 10.0, 10.0], 0.9, 1), (0, 1, [0.0, 0.0, 10.0, 10.0], 0.9, 2)]
    assert stitched(rows, [0, 2], max_link=1)['n_links'] == [0]


def test_affinity_equal_to_link_iou_links():
    assert stitched(TWO_PIECES, [0, 6], max_link=3, link_iou=0.25)['n_links'] == [1]               # 40 / 160 is exactly 0.25
    # boxes that only touch: a = 0 is not a link even with link_iou 0, nor with a negative one
    rows = [(0, 1, [0.0, 0.0, 10.0, 10.0], 0.9, 1), (1, 1, [10.0, 0.0, 10.0, 10.0], 0.9, 2)]
    assert stitched(rows, [0, 2], max_link=1, link_iou=0.0)['n_links'] == [0]
    assert stitched(rows, [0, 2], max_link=1, link_iou=-1.0)['n_links'] == [0]


def test_zero_area_boxes_never_link():
    rows = [(0, 1, [5.0, 5.0, 0.0, 0.0], 0.9, 1), (1, 1, [5.0, 5.0, 0.0, 0.0], 0.9, 2)]
    a = stitch_ref.affinity([(0, rows[0][2])], [(1, rows[1][2])], 'hold')
    assert a != a                                                                                 # 0 / 0
    assert stitched(rows, [0, 2], max_link=1, link_iou=0.0)['n_links'] == [0]
    assert stitched(rows, [0, 2], max_link=1, link_iou=-1.0)['n_links'] == [0]


def test_per_class_parameters():
    rows = [(0, 1, [0.0, 0.0, 10.0, 10.0], 0.9, 1), (0, 2, [100.0, 0.0, 10.0, 10.0], 0.9, 2), (0, 4, [200.0, 0.0, 10.0, 10.0], 0.9, 3),
            (2, 1, [0.0, 0.0, 10.0, 10.0], 0.9, 4), (2, 2, [105.0, 0.0, 10.0, 10.0], 0.9, 5), (2, 4, [200.0, 0.0, 10.0, 10.0], 0.9, 6)]
    # class 1: the gap of 2 is too long; class 2: 1/3 reaches 0.3; class 4: linked
    s = stitched(rows, [0, 3], max_link=[1, 2, 2, 2], link_iou=[0.3, 0.3, 0.3, 0.3])
    assert s['links'] == [(2, 5, 2, 50.0 / 150.0), (3, 6, 2, 1.0)] and s['object_id'] == [1, 2, 3, 4, 2, 3]
    s = stitched(rows, [0, 3], max_link=[2, 2, 2, 0], link_iou=[0.3, 0.5, 0.3, 0.3])
    assert s['links'] == [(1, 4, 2, 1.0)]
    # the class of a trajectory is that of its first observation
    rows = [(0, 1, [0.0, 0.0, 10.0, 10.0], 0.9, 1), (1, 2, [0.0, 0.0, 10.0, 10.0], 0.9, 1), (2, 1, [0.0, 0.0, 10.0, 10.0], 0.9, 2)]
    assert stitched(rows, [0, 3], max_link=[1, 0, 0, 0])['links'] == [(1, 2, 1, 1.0)]


def test_chain_of_three_pieces_takes_the_roots_id():
    box = [0.0, 0.0, 10.0, 10.0]
    rows = [(0, 1, box, 0.9, 30), (2, 1, box, 0.9, 20), (4, 1, box, 0.9, 10)]
    s = stitched(rows, [0, 5], max_link=2)
    assert s['object_id'] == [30, 30, 30] and s['pred'] == [-1, 0, 1] and s['root'] == [0, 0, 0] and s['links'] == [(30, 20, 2, 1.0), (20, 10, 2, 1.0)]
    # with a reach of 4 the first piece could take the third, but the shorter gap comes first among equal affinities
    assert stitched(rows, [0, 5], max_link=4)['pred'] == [-1, 0, 1]
    # unsorted rows are sorted first; the per-row outputs stay in the caller's order
    s = stitched([rows[2], rows[0], rows[1]], [0, 5], max_link=2)
    assert s['object_id'] == [30, 30, 30] and s['row_root'] == [0, 0, 0] and s['pred'] == [-1, 0, 1]


def test_streams_do_not_link_and_a_duplicate_is_refused():
    box = [0.0, 0.0, 10.0, 10.0]
    rows = [(2, 1, box, 0.9, 1), (3, 1, box, 0.9, 2)]
    assert stitched(rows, [0, 3, 6], max_link=3)['n_links'] == [0, 0]
    assert stitched(rows, [0, 6], max_link=3)['n_links'] == [1]
    try:
        stitched([(0, 1, box, 0.9, 1), (0, 1, box, 0.9, 1)], [0, 2], max_link=1)
    except ValueError as e:
        assert 'occurs twice in slot 0' in str(e)
    else:
        raise AssertionError('a duplicate was accepted')
