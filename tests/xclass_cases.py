"""Adversarial inputs for the cross-class track suppression.  Every case is (stream_frame_offsets, result,
jobs, claim): `result` has the columns utils.track_packed returns, `jobs` are dicts as tracking/xclass.py takes them and
claim(refs) - given the list of xclass_ref.xclass() outputs, one per job - asserts that the case is in the class its name says,
with the reference alone.  tests/test_xclass_cases.py runs the claims; tests/test_gpu_track_xclass.py compares the kernel with the
reference.  Boxes are [x, y, w, h]; classes: 1 vehicle, 2 pedestrian, 4 cyclist."""
import math

import dedup_ref
import xclass_ref
from dedup_cases import track
from track_cases import N_CLASSES, by_slot, result

NAN, INF = float('nan'), float('inf')
VEHICLE, PEDESTRIAN, CYCLIST = 1, 2, 4


def job(pairs, prio=0, measure='iomin'):
    """pairs: {(a, b): (frames, overlap, frac)}"""
    return {'pairs': dict((k, {'frames': v[0], 'overlap': v[1], 'frac': v[2]}) for k, v in pairs.items()),
            'prio': list(prio) if isinstance(prio, (list, tuple)) else [prio] * N_CLASSES, 'measure': measure}


def stream_trajectories(offsets, res, stream=0):
    return dedup_ref.trajectories(offsets, res).get(stream, [])


def rider_in_cyclist():
    """the pedestrian box on the rider lies wholly inside the cyclist box: IoMin 1, IoU 0.4.  IoMin >= 0.9 drops the pedestrian
    track, IoU >= 0.5 never sees the pair"""
    rows = by_slot(track(1, range(10), 0.0, w=10.0, h=15.0, category=CYCLIST) + track(2, range(1, 9), 2.0, w=6.0, h=10.0, category=PEDESTRIAN))
    jobs = [job({(2, 4): (3, 0.9, 0.5)}), job({(2, 4): (3, 0.5, 0.5)}, measure='iou')]

    def claim(refs):
        a, b = [0.0, 0.0, 10.0, 15.0], [2.0, 0.0, 8.0, 10.0]
        assert xclass_ref.iomin_dd(a, b) == 1.0 and 0.39 < dedup_ref.iou_dd(a, b) < 0.41
        assert refs[0]['keep'] == [1, 0] and refs[0]['by'] == [-1, 0] and refs[0]['match'] == [0, 8] and refs[0]['dropped'] == [(2, 1, 8)]
        assert refs[0]['category'] == [CYCLIST] * 10
        assert refs[1]['keep'] == [1, 1] and refs[1]['dropped'] == []
    return [0, 10], result(rows), jobs, claim


def priority_beats_length():
    """a pedestrian track of 12 rows and a cyclist track of 10 on one box, m = 10: with equal priorities the shorter cyclist goes,
    with the cyclist's priority raised the longer pedestrian goes"""
    rows = by_slot(track(1, range(12), 0.0, category=PEDESTRIAN) + track(2, range(1, 11), 0.0, category=CYCLIST))
    jobs = [job({(2, 4): (3, 0.9, 0.5)}), job({(2, 4): (3, 0.9, 0.5)}, prio=[0, 0, 0, 1])]

    def claim(refs):
        assert refs[0]['dropped'] == [(2, 1, 10)] and refs[0]['category'] == [PEDESTRIAN] * 12
        assert refs[1]['dropped'] == [(1, 2, 10)] and refs[1]['category'] == [CYCLIST] * 10
    return [0, 12], result(rows), jobs, claim


def weaker_ones_rows():
    """a cyclist track of 3 rows with priority 1 over a pedestrian of 50 rows, frames 3, frac 0.5: 3 < 0.5 * 50 - the test is made
    against the weaker one's rows, not the shorter one's, and nobody goes.  With equal priorities the cyclist is the weaker: 3 >= 1.5"""
    rows = by_slot(track(1, range(50), 0.0, category=PEDESTRIAN) + track(2, range(20, 23), 0.0, category=CYCLIST))
    jobs = [job({(2, 4): (3, 0.9, 0.5)}, prio=[0, 0, 0, 1]), job({(2, 4): (3, 0.9, 0.5)})]

    def claim(refs):
        assert refs[0]['dropped'] == [] and refs[0]['keep'] == [1, 1] and refs[0]['row_keep'] == [1] * 53
        assert refs[1]['dropped'] == [(2, 1, 3)]
        # the rule of the shorter one's rows would let the 3-row track remove the 50-row one
        assert 3.0 >= 0.5 * 3.0 and not 3.0 >= 0.5 * 50.0
    return [0, 50], result(rows), jobs, claim


def pairs_on_and_off():
    """a pedestrian and a cyclist track on one box, and far away two vehicle tracks on one box.  Pair (1, 2) on: nothing is
    compared.  Pair (2, 4) on, the diagonal 0: the vehicle twins are untouched.  Pair (1, 1) on: the weaker twin goes, the
    other two stay.  An asymmetric table is refused."""
    rows = track(1, range(6), 0.0, category=PEDESTRIAN, score=0.4) + track(2, range(6), 0.0, category=CYCLIST, score=0.9)
    rows += track(3, range(6), 500.0, category=VEHICLE, score=0.9) + track(4, range(6), 500.0, category=VEHICLE, score=0.4)
    jobs = [job({(1, 2): (1, 0.5, 0.0)}), job({(2, 4): (3, 0.9, 0.5)}), job({(1, 1): (3, 0.9, 0.5)}), job({(2, 4): (0, 0.9, 0.5), (1, 1): (0, 0.0, 0.0)})]

    def claim(refs):
        assert refs[0]['dropped'] == [] and refs[3]['dropped'] == []
        assert refs[1]['dropped'] == [(1, 2, 6)] and refs[1]['keep'] == [0, 1, 1, 1]
        assert refs[2]['dropped'] == [(4, 3, 6)] and refs[2]['keep'] == [1, 1, 1, 0]
        frames, overlap, frac = [[0] * 4 for _ in range(4)], [[0.7] * 4 for _ in range(4)], [[0.5] * 4 for _ in range(4)]
        frames[1][3] = 3
        for bad in ({'frames': frames, 'overlap': overlap, 'frac': frac},):
            try:
                xclass_ref.tables(bad, 4)
            except ValueError as e:
                assert 'pair (2, 4) and pair (4, 2) differ' in str(e)
            else:
                raise AssertionError('an asymmetric table was taken')
    return [0, 6], result(by_slot(rows)), jobs, claim


def iomin_at_threshold():
    """[0, 0, 10, 10] against [5, 0, 20, 10]: 50 of the smaller area 100, IoMin 0.5 exactly - the same object at overlap 0.5 and
    one ulp below, not one ulp above"""
    rows = by_slot(track(1, range(4), 0.0, w=10.0, h=10.0, category=CYCLIST) + track(2, range(3), 5.0, w=20.0, h=10.0, category=PEDESTRIAN))
    jobs = [job({(2, 4): (1, t, 0.5)}) for t in (0.5, math.nextafter(0.5, 1.0), math.nextafter(0.5, 0.0))]

    def claim(refs):
        assert xclass_ref.iomin_dd([0.0, 0.0, 10.0, 10.0], [5.0, 0.0, 25.0, 10.0]) == 0.5
        assert [r['n_dropped'] for r in refs] == [[1], [0], [1]] and refs[0]['match'] == [0, 3] and refs[0]['dropped'] == [(2, 1, 3)]
    return [0, 4], result(rows), jobs, claim


def _naive_iomin(a, b):
    """wh over the smaller area WITHOUT the guard, in the ternaries of iou_dd"""
    xx1 = a[0] if a[0] > b[0] else b[0]
    yy1 = a[1] if a[1] > b[1] else b[1]
    xx2 = a[2] if a[2] < b[2] else b[2]
    yy2 = a[3] if a[3] < b[3] else b[3]
    w = xx2 - xx1
    if not w > 0.0:
        w = 0.0
    h = yy2 - yy1
    if not h > 0.0:
        h = 0.0
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[2] - b[0]) * (b[3] - b[1])
    lo = area_a if area_a < area_b else area_b
    return (w * h) / lo


def degenerate_boxes():
    """pairs of a pedestrian and a cyclist track on one place whose boxes are degenerate - zero size, a NaN coordinate, a NaN width
    against a sound box, an infinite width against a sound box, negative extents, a negative width: under both measures nothing
    matches and everything survives.  The unguarded quotient would match the NaN-wide and the infinitely wide box."""
    both = lambda i, x, **kw: track(2 * i + 1, range(4), x, category=PEDESTRIAN, **kw) + track(2 * i + 2, range(4), x, category=CYCLIST, **kw)
    rows = both(0, 5.0, w=0.0, h=0.0) + both(1, NAN) + both(5, 400.0, w=-10.0, h=-10.0) + both(6, 500.0, w=-10.0)
    rows += track(21, range(4), 100.0, w=NAN, category=PEDESTRIAN) + track(22, range(4), 100.0, category=CYCLIST)
    rows += track(23, range(4), 200.0, w=INF, category=PEDESTRIAN) + track(24, range(4), 200.0, category=CYCLIST)
    rows += track(25, range(4), 300.0, w=INF, h=INF, category=PEDESTRIAN) + track(26, range(4), 300.0, w=INF, h=INF, category=CYCLIST)
    res = result(by_slot(rows))
    jobs = [job({(2, 4): (1, 0.0, 0.0)}, measure='iomin'), job({(2, 4): (1, 0.0, 0.0)}, measure='iou')]

    def claim(refs):
        nan = lambda v: v != v
        sound = [100.0, 0.0, 110.0, 10.0]
        assert _naive_iomin([100.0, 0.0, NAN, 10.0], sound) > 0.0 and nan(xclass_ref.iomin_dd([100.0, 0.0, NAN, 10.0], sound))
        assert _naive_iomin([100.0, 0.0, INF, 10.0], sound) == 1.0 and nan(xclass_ref.iomin_dd([100.0, 0.0, INF, 10.0], sound))
        assert nan(xclass_ref.iomin_dd([5.0, 0.0, 5.0, 0.0], [5.0, 0.0, 5.0, 0.0])) and xclass_ref.iomin_dd([0.0, 0.0, -10.0, -10.0], [0.0, 0.0, -10.0, -10.0]) == 0.0
        for ref in refs:
            assert ref['keep'] == [1] * 14 and ref['row_keep'] == [1] * 56 and ref['n_dropped'] == [0]
    return [0, 4], res, jobs, claim


def cross_class_chain():
    """vehicle A > cyclist B > pedestrian C by length; A / B and B / C overlap by 8 / 12, A / C by 6 / 14: B goes, and C - whose
    only stronger match was suppressed - stays.  A rule that lets suppressed tracks suppress would drop C too."""
    rows = by_slot(track(1, range(8), 0.0, category=VEHICLE) + track(2, range(7), 2.0, category=CYCLIST) + track(3, range(6), 4.0, category=PEDESTRIAN))
    res = result(rows)
    jobs = [job({(1, 4): (3, 0.6, 0.5), (2, 4): (3, 0.6, 0.5), (1, 2): (3, 0.6, 0.5)}, measure='iou')]

    def claim(refs):
        assert refs[0]['keep'] == [1, 0, 1] and refs[0]['by'] == [-1, 0, -1] and refs[0]['match'] == [0, 7, 0]
        other = xclass_ref.xclass([0, 8], res, jobs[0], suppressed_suppress=True)
        assert other['keep'] == [1, 0, 0] and other['by'] == [-1, 0, 1]
    return [0, 8], res, jobs, claim


def strongest_kept_suppressor():
    """the pedestrian track (index 2) is the same object as two kept tracks of two classes that are not each other's: by is the
    stronger one - index 1, the cyclist, the longer - and match is that pair's count, 8, not the 7 of the other pair.  With the
    vehicle's priority raised it is the vehicle, and match 7."""
    rows = by_slot(track(20, range(9), 6.0, category=VEHICLE) + track(10, range(10), 0.0, category=CYCLIST) + track(30, range(2, 10), 3.0, category=PEDESTRIAN))
    res = result(rows)
    pairs = {(1, 2): (3, 0.5, 0.5), (2, 4): (3, 0.5, 0.5), (1, 4): (3, 0.5, 0.5)}
    jobs = [job(pairs, measure='iou'), job(pairs, prio=[1, 0, 0, 0], measure='iou')]

    def claim(refs):
        assert xclass_ref.same_objects(stream_trajectories([0, 10], res), jobs[0], 4) == {(0, 2): 7, (1, 2): 8}
        assert refs[0]['keep'] == [1, 1, 0] and refs[0]['by'] == [-1, -1, 1] and refs[0]['match'] == [0, 0, 8] and refs[0]['dropped'] == [(30, 10, 8)]
        assert refs[1]['by'] == [-1, -1, 0] and refs[1]['match'] == [0, 0, 7]
    return [0, 10], res, jobs, claim


def first_rows_class():
    """track 5's first row says cyclist and its later rows pedestrian: it is a cyclist, and the pedestrian track 6 on its box goes.
    Track 7's first row says pedestrian and its later rows cyclist: it is a pedestrian, and the pedestrian track 8 on its box is not
    compared with it (the diagonal is off)."""
    mixed = track(5, range(6), 0.0, category=PEDESTRIAN)
    mixed[0] = (0, CYCLIST) + mixed[0][2:]
    other = track(7, range(6), 300.0, category=CYCLIST)
    other[0] = (0, PEDESTRIAN) + other[0][2:]
    res = result(by_slot(mixed + track(6, range(5), 0.0, category=PEDESTRIAN) + other + track(8, range(5), 300.0, category=PEDESTRIAN)))

    def claim(refs):
        assert [t.category for t in stream_trajectories([0, 6], res)] == [CYCLIST, PEDESTRIAN, PEDESTRIAN, PEDESTRIAN]
        assert refs[0]['keep'] == [1, 0, 1, 1] and refs[0]['dropped'] == [(6, 5, 5)]
    return [0, 6], res, [job({(2, 4): (3, 0.9, 0.5)})], claim


def inert_categories():
    """categories 0 and C + 1 = 5 take part in no pair, whatever lies on them: tracks of category 0, 5, 2 and 4 on one box, every
    pair of classes on - only the pedestrian and the cyclist are compared.  The Python layer and the host form refuse such
    categories; the device form must not follow them into its tables."""
    rows = track(1, range(6), 0.0, category=0, score=0.9) + track(2, range(6), 0.0, category=5, score=0.9)
    rows += track(3, range(6), 0.0, category=CYCLIST, score=0.6) + track(4, range(6), 0.0, category=PEDESTRIAN)
    every = dict(((a, b), (1, 0.5, 0.0)) for a in range(1, 5) for b in range(a, 5))

    def claim(refs):
        assert refs[0]['keep'] == [1, 1, 1, 0] and refs[0]['dropped'] == [(4, 3, 6)]
    return [0, 6], result(by_slot(rows)), [job(every, prio=[0, 0, 0, 1])], claim


def slot_of(n):
    """n trajectories with a row in every one of three slots: more rows in a slot than a wavefront has lanes.  The last one, a
    pedestrian, sits on the first, a cyclist (their rows are in different 64-row blocks of the slot when n > 64); 2, a pedestrian,
    sits on 1, a cyclist."""
    rows = []
    for k in range(n):
        x, category = 40.0 * k, (PEDESTRIAN, CYCLIST, VEHICLE)[k % 3]
        if k in (0, 1):
            category = CYCLIST
        if k == n - 1:
            x, category = 0.0, PEDESTRIAN
        if k == 2:
            x, category = 40.0, PEDESTRIAN
        rows += track(k, range(3), x, score=0.5 - 0.001 * k, category=category)
    res = result(by_slot(rows))

    def claim(refs):
        assert refs[0]['dropped'] == [(2, 1, 3), (n - 1, 0, 3)] and len(refs[0]['keep']) == n and sum(refs[0]['keep']) == n - 2
        assert res['frame'].count(0) == n
    return [0, 3], res, [job({(2, 4): (3, 0.7, 0.5)}, measure='iou')], claim


def many_trajectories(n):
    """n trajectories in one stream: four long cyclists over all 24 slots, each with a short pedestrian copy on its last three slots
    that is appended last - the members of a pair are far apart in local index - and n - 8 short ones of classes 1 and 2, apart
    from each other, in eight groups of three slots"""
    rows = []
    for k in range(4):
        rows += track(k, range(24), 0.0, y=1000.0 + 100.0 * k, score=0.5, category=CYCLIST)
    for i in range(n - 8):
        rows += track(100 + i, range(3 * (i % 8), 3 * (i % 8) + 3), 40.0 * (i // 8), category=1 + i % 2)
    for k in range(4):
        rows += track(50 + k, range(21, 24), 0.0, y=1000.0 + 100.0 * k, score=0.25, category=PEDESTRIAN)
    res = result(by_slot(rows))

    def claim(refs):
        assert len(refs[0]['keep']) == n and refs[0]['n_dropped'] == [4]
        assert refs[0]['dropped'] == [(50 + k, k, 3) for k in range(4)]
        gone = [t for t in range(n) if not refs[0]['keep'][t]]
        assert all(t - refs[0]['by'][t] > n // 2 for t in gone)
        assert refs[1]['n_dropped'] == [0]
    return [0, 24], res, [job({(2, 4): (3, 0.7, 0.5)}), job({(2, 4): (4, 0.7, 0.5)})], claim


def streams():
    """a cyclist in stream 0 and a pedestrian on the same box in stream 2 are untouched; stream 1 is empty; stream 2 holds a real pair"""
    rows = track(1, range(4), 0.0, category=CYCLIST) + track(2, range(4, 8), 0.0, category=PEDESTRIAN, score=0.4) + track(3, range(4, 8), 0.0, category=CYCLIST)
    res = result(by_slot(rows))

    def claim(refs):
        assert refs[0]['traj_offsets'] == [0, 1, 1, 3] and refs[0]['keep'] == [1, 0, 1] and refs[0]['n_dropped'] == [0, 0, 1]
        assert refs[0]['by'] == [-1, 1, -1]                                                  # local to its stream
    return [0, 4, 4, 8], res, [job({(2, 4): (3, 0.9, 0.5)})], claim


def empty_result():
    def claim(refs):
        assert refs[0]['object_id'] == [] and refs[0]['n_dropped'] == [0, 0] and refs[0]['keep'] == [] and refs[0]['traj_offsets'] == [0, 0, 0]
    return [0, 2, 4], result([]), [job({(2, 4): (3, 0.9, 0.5)})], claim


CASES = {
    'rider_in_cyclist': rider_in_cyclist,
    'priority_beats_length': priority_beats_length,
    'weaker_ones_rows': weaker_ones_rows,
    'pairs_on_and_off': pairs_on_and_off,
    'iomin_at_threshold': iomin_at_threshold,
    'degenerate_boxes': degenerate_boxes,
    'cross_class_chain': cross_class_chain,
    'strongest_kept_suppressor': strongest_kept_suppressor,
    'first_rows_class': first_rows_class,
    'inert_categories': inert_categories,
    'slot_of_64': lambda: slot_of(64),
    'slot_of_65': lambda: slot_of(65),
    'slot_of_130': lambda: slot_of(130),
    'many_trajectories_200': lambda: many_trajectories(200),
    'streams': streams,
    'empty_result': empty_result,
}
# cases whose categories the Python layer and the host form refuse: the GPU test writes them into the device form's columns
DEVICE_ONLY = ('inert_categories',)
