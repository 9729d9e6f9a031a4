"""Adversarial inputs for the track deduplication.  Every case is (stream_frame_offsets, result, jobs, claim):
`result` has the columns utils.track_packed returns, `jobs` are dicts as tracking/dedup.py takes them and claim(refs) - given the
list of dedup_ref.dedup() outputs, one per job - asserts that the case is in the class its name says, with the reference alone.
tests/test_dedup_cases.py runs the claims; tests/test_gpu_track_dedup.py compares the kernel with the reference."""
import math

import dedup_ref
from track_cases import N_CLASSES, by_slot, result

NAN = float('nan')


def job(min_frames=0, dup_iou=0.7, dup_frac=0.5):
    per_class = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * N_CLASSES
    return {'min_frames': per_class(min_frames), 'dup_iou': per_class(dup_iou), 'dup_frac': per_class(dup_frac)}


def track(object_id, slots, x, y=0.0, w=10.0, h=10.0, category=1, score=0.5):
    """one row per slot; x may be a function of the slot"""
    return [(slot, category, [float(x(slot)) if callable(x) else float(x), float(y), float(w), float(h)], score, object_id) for slot in slots]


def stream_trajectories(offsets, res, stream=0):
    return dedup_ref.trajectories(offsets, res).get(stream, [])


def equal_twins():
    """two identical tracks, equal length, equal score sum: the lower local index wins"""
    rows = by_slot(track(7, range(5), 3.0) + track(4, range(5), 3.0))
    res = result(rows)

    def claim(refs):
        a, b = stream_trajectories([0, 5], res)
        assert a.n == b.n and a.score_sum == b.score_sum and a.object_id == 7
        assert refs[0]['keep'] == [1, 0] and refs[0]['by'] == [-1, 0] and refs[0]['match'] == [0, 5] and refs[0]['dropped'] == [(4, 7, 5)]
        assert refs[0]['object_id'] == [7] * 5 and refs[0]['row_keep'] == [1, 0] * 5
    return [0, 5], res, [job(min_frames=3)], claim


def score_tie_break():
    """equal length: the higher score sum wins although its local index is higher"""
    rows = by_slot(track(1, range(5), 3.0, score=0.5) + track(2, range(5), 3.5, score=0.75))

    def claim(refs):
        assert refs[0]['keep'] == [0, 1] and refs[0]['by'] == [1, -1] and refs[0]['dropped'] == [(1, 2, 5)]
    return [0, 5], result(rows), [job(min_frames=3)], claim


def length_before_score():
    """the longer track wins against a shorter one of much higher score"""
    rows = by_slot(track(1, range(1, 6), 3.0, score=0.99) + track(2, range(6), 3.0, score=0.25))
    res = result(rows)

    def claim(refs):
        short, long_ = sorted(stream_trajectories([0, 6], res), key=lambda t: t.n)
        assert short.score_sum > long_.score_sum and short.n == 5 and long_.n == 6
        assert refs[0]['dropped'] == [(1, 2, 5)] and refs[0]['object_id'] == [2] * 6
    return [0, 6], res, [job(min_frames=3)], claim


def greedy_chain():
    """A > B > C by length; A / B and B / C overlap by 8 / 12, A / C by 6 / 14: B goes, and C - whose only stronger duplicate was
    suppressed - stays.  A rule that lets suppressed tracks suppress would drop C too."""
    rows = by_slot(track(1, range(8), 0.0) + track(2, range(7), 2.0) + track(3, range(6), 4.0))
    res, jobs = result(rows), [job(min_frames=3, dup_iou=0.6)]

    def claim(refs):
        assert refs[0]['keep'] == [1, 0, 1] and refs[0]['by'] == [-1, 0, -1] and refs[0]['match'] == [0, 7, 0]
        other = dedup_ref.dedup([0, 8], res, jobs[0], suppressed_suppress=True)
        assert other['keep'] == [1, 0, 0] and other['by'] == [-1, 0, 1]
    return [0, 8], res, jobs, claim


def deep_chain(depth=40):
    """trajectory k at x = 2 k, one row shorter than k - 1: neighbours are duplicates, no others.  Every second one is kept and the
    decision of k waits for that of k - 1: a matcher that works in rounds takes one round per link."""
    rows = []
    for k in range(depth):
        rows += track(100 + k, range(depth + 5 - k), 2.0 * k)
    res, jobs = result(by_slot(rows)), [job(min_frames=3, dup_iou=0.6)]

    def claim(refs):
        trajs = stream_trajectories([0, depth + 5], res)
        dups = dedup_ref.duplicates(trajs, jobs[0])
        assert sorted(dups) == [(k, k + 1) for k in range(depth - 1)]
        keep, by, match, rounds = dedup_ref.suppress_in_rounds(trajs, dups)
        assert rounds == depth and (keep, by, match) == (refs[0]['keep'], refs[0]['by'], refs[0]['match'])
        assert refs[0]['keep'] == [1 - k % 2 for k in range(depth)] and refs[0]['by'] == [k - 1 if k % 2 else -1 for k in range(depth)]
    return [0, depth + 5], res, jobs, claim


def strongest_kept_suppressor():
    """T (index 2) duplicates two kept tracks that are no duplicates of each other: by is the stronger one - index 1, the longer -
    and match is that pair's count, 8, not the 7 of the other pair"""
    rows = by_slot(track(20, range(9), 6.0) + track(10, range(10), 0.0) + track(30, range(2, 10), 3.0))
    res, jobs = result(rows), [job(min_frames=3, dup_iou=0.5)]

    def claim(refs):
        dups = dedup_ref.duplicates(stream_trajectories([0, 10], res), jobs[0])
        assert dups == {(0, 2): 7, (1, 2): 8}
        assert refs[0]['keep'] == [1, 1, 0] and refs[0]['by'] == [-1, -1, 1] and refs[0]['match'] == [0, 0, 8]
        assert refs[0]['dropped'] == [(30, 10, 8)]
    return [0, 10], res, jobs, claim


def iou_at_threshold():
    """[0, 0, 2, 1] against [0, 0, 1, 1] is 0.5 exactly: a duplicate at dup_iou 0.5 and one ulp below, none one ulp above"""
    rows = by_slot(track(1, range(4), 0.0, w=2.0, h=1.0) + track(2, range(3), 0.0, w=1.0, h=1.0))
    jobs = [job(min_frames=1, dup_iou=0.5), job(min_frames=1, dup_iou=math.nextafter(0.5, 1.0)), job(min_frames=1, dup_iou=math.nextafter(0.5, 0.0))]

    def claim(refs):
        assert dedup_ref.iou_dd([0.0, 0.0, 2.0, 1.0], [0.0, 0.0, 1.0, 1.0]) == 0.5
        assert [r['n_dropped'] for r in refs] == [[1], [0], [1]] and refs[0]['match'] == [0, 3]
    return [0, 4], result(rows), jobs, claim


def frac_and_frames_edges():
    """m = 3 of min(n) = 6: a duplicate at dup_frac 0.5, none one ulp above; at min_frames 3, not at 4"""
    far = lambda slot: 0.0 if slot < 3 else 500.0
    rows = by_slot(track(1, range(8), 0.0) + track(2, range(6), far))
    jobs = [job(min_frames=1, dup_frac=0.5), job(min_frames=1, dup_frac=math.nextafter(0.5, 1.0)), job(min_frames=3, dup_frac=0.0),
            job(min_frames=4, dup_frac=0.0)]

    def claim(refs):
        assert [r['n_dropped'] for r in refs] == [[1], [0], [1], [0]]
        assert refs[0]['match'] == [0, 3] and refs[2]['dropped'] == [(2, 1, 3)]
        assert 0.5 * 6.0 == 3.0 and math.nextafter(0.5, 1.0) * 6.0 > 3.0
    return [0, 8], result(rows), jobs, claim


def crossing_objects():
    """two real objects pass each other: 25 / 35 of overlap in two slots of twenty.  They survive min_frames 3; a setting that asks
    for two frames and a tenth of the track loses one of them."""
    rows = by_slot(track(1, range(20), lambda s: 5.0 * s, w=30.0) + track(2, range(20), lambda s: 5.0 * (19 - s), w=30.0))
    res, jobs = result(rows), [job(min_frames=3, dup_frac=0.1), job(min_frames=2, dup_frac=0.1)]

    def claim(refs):
        a, b = stream_trajectories([0, 20], res)
        assert dedup_ref.match_count(a, b, 0.7) == 2
        assert refs[0]['n_dropped'] == [0] and refs[0]['row_keep'] == [1] * 40 and refs[1]['dropped'] == [(2, 1, 2)]
    return [0, 20], res, jobs, claim


def holes():
    """class 1: two tracks on one box whose observed slots alternate - they never meet.  Class 2: a track with holes shares five
    of its seven slots with a full one: m counts those five only."""
    rows = track(1, range(0, 14, 2), 0.0) + track(2, range(1, 14, 2), 0.0)
    rows += track(3, range(10), 100.0, category=2) + track(4, (0, 2, 4, 5, 6, 12, 13), 100.0, category=2)
    res = result(by_slot(rows))

    def claim(refs):
        assert [t.object_id for t in stream_trajectories([0, 14], res)] == [1, 3, 4, 2]     # by first appearance
        assert refs[0]['keep'] == [1, 1, 0, 1] and refs[0]['match'] == [0, 0, 5, 0] and refs[0]['dropped'] == [(4, 3, 5)]
        assert refs[1]['n_dropped'] == [0]                                                  # 5 < 0.75 * 7
    return [0, 14], res, [job(min_frames=1, dup_frac=0.5), job(min_frames=1, dup_frac=0.75)], claim


def classes():
    """identical tracks: 1 and 2 of classes 1 and 2 (untouched); 3 and 4 of class 3 (min_frames 0 in job 0: untouched); 5 whose
    first row is class 4 and whose later rows say 1, with 6 of class 4 (duplicates: the class is the first row's) and 7 of class 1
    on the same box (not a duplicate of 5, whatever its later rows say)"""
    rows = track(1, range(5), 0.0, category=1) + track(2, range(5), 0.0, category=2)
    rows += track(3, range(5), 100.0, category=3) + track(4, range(5), 100.0, category=3)
    mixed = track(5, range(6), 200.0, category=1)
    mixed[0] = (0, 4) + mixed[0][2:]
    rows += mixed + track(6, range(5), 200.0, category=4) + track(7, range(5), 200.0, category=1)
    res = result(by_slot(rows))

    def claim(refs):
        assert [t.category for t in stream_trajectories([0, 6], res)] == [1, 2, 3, 3, 4, 4, 1]
        assert refs[0]['keep'] == [1, 1, 1, 1, 1, 0, 1] and refs[0]['dropped'] == [(6, 5, 5)]
        assert refs[1]['keep'] == [1, 1, 1, 0, 1, 0, 1]
    return [0, 6], res, [job(min_frames=[3, 3, 0, 3]), job(min_frames=3)], claim


def degenerate_boxes():
    """zero-area boxes (IoU 0 / 0), boxes with a NaN coordinate and an infinite one, each twice on the same place: no pair ever
    matches and everything survives"""
    rows = track(1, range(4), 5.0, w=0.0, h=0.0) + track(2, range(4), 5.0, w=0.0, h=0.0)
    rows += track(3, range(4), NAN) + track(4, range(4), NAN)
    rows += track(5, range(4), 50.0, w=NAN) + track(6, range(4), 50.0, w=NAN)
    rows += track(7, range(4), 90.0, w=float('inf'), h=float('inf')) + track(8, range(4), 90.0, w=float('inf'), h=float('inf'))
    res = result(by_slot(rows))

    def claim(refs):
        nan = lambda v: v != v
        assert nan(dedup_ref.iou_dd([5.0, 0.0, 5.0, 0.0], [5.0, 0.0, 5.0, 0.0])) and nan(dedup_ref.iou_dd([NAN, 0.0, NAN, 10.0], [NAN, 0.0, NAN, 10.0]))
        assert refs[0]['keep'] == [1] * 8 and refs[0]['row_keep'] == [1] * 32 and refs[0]['n_dropped'] == [0]
    return [0, 4], res, [job(min_frames=1, dup_iou=0.0, dup_frac=0.0)], claim


def streams():
    """identical tracks in streams 0 and 2 are untouched; stream 1 is empty; stream 2 holds a real pair"""
    rows = track(1, range(4), 0.0) + track(2, range(4, 8), 0.0) + track(3, range(4, 8), 0.0)
    res = result(by_slot(rows))

    def claim(refs):
        assert refs[0]['traj_offsets'] == [0, 1, 1, 3] and refs[0]['keep'] == [1, 1, 0] and refs[0]['n_dropped'] == [0, 0, 1]
        assert refs[0]['by'] == [-1, -1, 0]                                                  # local to its stream
    return [0, 4, 4, 8], res, [job(min_frames=3)], claim


def empty_result():
    def claim(refs):
        assert refs[0]['object_id'] == [] and refs[0]['n_dropped'] == [0, 0] and refs[0]['keep'] == [] and refs[0]['traj_offsets'] == [0, 0, 0]
    return [0, 2, 4], result([]), [job(min_frames=3)], claim


def slot_of(n):
    """n trajectories with a row in every one of three slots: more rows in a slot than a wavefront has lanes.  The last one
    sits on the first (their rows are in different 64-row blocks of the slot when n > 64), 2 sits on 1."""
    rows = []
    for k in range(n):
        x = 40.0 * k
        if k == n - 1:
            x = 0.0
        if k == 2:
            x = 40.0
        rows += track(k, range(3), x, score=0.5 - 0.001 * k)
    res = result(by_slot(rows))

    def claim(refs):
        assert refs[0]['dropped'] == [(2, 1, 3), (n - 1, 0, 3)] and len(refs[0]['keep']) == n and sum(refs[0]['keep']) == n - 2
        assert res['frame'].count(0) == n
    return [0, 3], res, [job(min_frames=3)], claim


def many_trajectories(n):
    """n trajectories in one stream: four long ones over all 24 slots, each with a short copy on its last three slots that is
    appended last - the members of a pair are far apart in local index - and n - 8 short ones, apart from each other, in eight
    groups of three slots"""
    rows = []
    for k in range(4):
        rows += track(k, range(24), 0.0, y=1000.0 + 100.0 * k, score=0.5)
    for i in range(n - 8):
        rows += track(100 + i, range(3 * (i % 8), 3 * (i % 8) + 3), 40.0 * (i // 8), category=1 + i % 2)
    for k in range(4):
        rows += track(50 + k, range(21, 24), 0.0, y=1000.0 + 100.0 * k, score=0.25)
    res = result(by_slot(rows))

    def claim(refs):
        assert len(refs[0]['keep']) == n and refs[0]['n_dropped'] == [4]
        assert refs[0]['dropped'] == [(50 + k, k, 3) for k in range(4)]
        gone = [t for t in range(n) if not refs[0]['keep'][t]]
        assert all(t - refs[0]['by'][t] > n // 2 for t in gone)
        assert refs[1]['n_dropped'] == [0]
    return [0, 24], res, [job(min_frames=3, dup_frac=0.5), job(min_frames=4)], claim


CASES = {
    'equal_twins': equal_twins,
    'score_tie_break': score_tie_break,
    'length_before_score': length_before_score,
    'greedy_chain': greedy_chain,
    'deep_chain_40': deep_chain,
    'strongest_kept_suppressor': strongest_kept_suppressor,
    'iou_at_threshold': iou_at_threshold,
    'frac_and_frames_edges': frac_and_frames_edges,
    'crossing_objects': crossing_objects,
    'holes': holes,
    'classes': classes,
    'degenerate_boxes': degenerate_boxes,
    'streams': streams,
    'empty_result': empty_result,
    'slot_of_64': lambda: slot_of(64),
    'slot_of_65': lambda: slot_of(65),
    'slot_of_130': lambda: slot_of(130),
    'many_trajectories_200': lambda: many_trajectories(200),
}
