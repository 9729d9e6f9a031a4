"""Adversarial inputs for the track refinement.  Every case is (stream_frame_offsets, result, jobs, claim):
`result` has the columns utils.track_packed returns, `jobs` are dicts as tracking/refine.py takes them and claim(refined) - given
the list of refine_ref.refine() outputs, one per job - asserts that the case is in the class its name says.
tests/test_refine_cases.py runs the claims on the reference alone; tests/test_gpu_track_refine.py compares the kernel with it."""
import random

from track_cases import N_CLASSES, result


def job(max_gap=0, min_len=1, score_mode='keep'):
    per_class = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * N_CLASSES
    return {'max_gap': per_class(max_gap), 'min_len': per_class(min_len), 'score_mode': score_mode}


def box(i, slot):
    """a box of object i at a slot: fractional, different in every coordinate, moving"""
    return [10.0 + 7.3 * i + 1.7 * slot, 20.0 + 3.1 * i - 0.9 * slot, 30.0 + 0.37 * (i % 11) + 0.2 * slot, 40.0 + 0.53 * (i % 7)]


def fills(r):
    return [i for i, s in enumerate(r['source']) if s < 0]


def fills_at(r, slot):
    return [i for i in fills(r) if r['frame'][i] == slot]


def same_gap_slot(n):
    """n trajectories of one stream, all in a gap at slot 1: the order of the filled rows must hold across 64-lane chunks"""
    rows = [(0, 1, box(i, 0), 0.5 + 0.001 * i, 100 + i) for i in range(n)] + [(2, 1, box(i, 2), 0.6, 100 + i) for i in reversed(range(n))]

    def claim(refined):
        r = refined[0]
        at = fills_at(r, 1)
        assert len(at) == n and len(r['frame']) == 3 * n
        assert [r['object_id'][i] for i in at] == [100 + i for i in range(n)]           # ascending trajectory index = first appearance
        assert [-1 - r['source'][i] for i in at] == [2 * n - 1 - i for i in range(n)]    # the later endpoints came in reversed
        assert refined[1]['frame'] == [0] * n + [2] * n
    return [0, 3], result(rows), [job(max_gap=1), job(max_gap=0)], claim


def crowded_slot(n=65):
    """n observed rows in one slot, every second one of a trajectory that the length filter removes"""
    rows = [(1, 1 + i % 2, box(i, 1), 0.9, i) for i in range(n)] + [(2, 1, box(i, 2), 0.8, i) for i in range(0, n, 2)]

    def claim(refined):
        assert refined[0]['source'] == list(range(len(rows)))
        r = refined[1]
        assert [s for s in r['source'] if s < n] == list(range(0, n, 2))                 # interleaved survivors keep their input order
        assert len(r['frame']) == 2 * len(range(0, n, 2)) and r['frame_row_offsets'] == [0, 0, (n + 1) // 2, 2 * ((n + 1) // 2)]
    return [0, 3], result(rows), [job(), job(min_len=2)], claim


def gap_limits():
    """holes of max_gap and max_gap + 1, several gaps in one trajectory on both sides of the limit, first and last slot of a stream"""
    slots = {1: [0, 3], 2: [0, 4], 3: [0, 2, 5, 6, 10, 11]}
    rows = [(s, 1, box(i, s), 0.5 + 0.01 * s, i) for i, ss in slots.items() for s in ss]
    rows.sort(key=lambda r: r[0])

    def claim(refined):
        r = refined[0]                                                                    # max_gap 2
        got = sorted((r['object_id'][i], r['frame'][i]) for i in fills(r))
        assert got == [(1, 1), (1, 2), (3, 1), (3, 3), (3, 4)]
        assert r['frame'][0] == 0 and r['frame'][-1] == 11 and r['frame_row_offsets'][-1] == len(r['frame'])
        assert sorted((refined[1]['object_id'][i], refined[1]['frame'][i]) for i in fills(refined[1])) == sorted(
            got + [(2, 1), (2, 2), (2, 3), (3, 7), (3, 8), (3, 9)])                       # max_gap 3
    return [0, 12], result(rows), [job(max_gap=2), job(max_gap=3)], claim


def neighbouring_streams():
    """the same object id, and so the same local index, at the end of one stream and the start of the next; a stream without frames"""
    rows = [(0, 1, box(0, 0), 0.9, 7), (2, 1, box(0, 2), 0.9, 7), (3, 1, box(1, 3), 0.8, 7), (5, 1, box(1, 5), 0.8, 7), (5, 2, box(2, 5), 0.7, 8)]

    def claim(refined):
        r = refined[0]
        assert sorted(r['frame'][i] for i in fills(r)) == [1, 4]                          # nothing at slot 3 - 2: the streams do not link
        assert len(refined[1]['frame']) == 4 and 8 not in refined[1]['object_id']         # 7 has two observations in EACH stream, not four
        assert len(refined[2]['frame']) == 0
    return [0, 3, 3, 6], result(rows), [job(max_gap=5), job(min_len=2), job(min_len=3)], claim


def empty_result():
    def claim(refined):
        assert refined[0]['frame'] == [] and refined[0]['frame_row_offsets'] == [0] * 5
    return [0, 2, 4], result([]), [job(max_gap=3, min_len=2, score_mode='mean')], claim


def classes():
    """a trajectory of class 2 between class-1 neighbours, per-class parameters; the class of the first observation governs"""
    rows = [(0, 1, box(0, 0), 0.9, 0), (0, 2, box(1, 0), 0.8, 1), (0, 1, box(2, 0), 0.7, 2), (0, 2, box(3, 0), 0.6, 3),
            (3, 1, box(0, 3), 0.9, 0), (3, 2, box(1, 3), 0.8, 1), (3, 1, box(2, 3), 0.7, 2), (3, 1, box(3, 3), 0.6, 3),
            (4, 1, box(0, 4), 0.9, 0)]

    def claim(refined):
        r = refined[0]                                                                    # class 1: no filling, 3 observations; class 2: gap 2
        assert sorted(set(r['object_id'])) == [0, 1, 3]
        assert sorted((r['object_id'][i], r['frame'][i], r['category'][i]) for i in fills(r)) == [(1, 1, 2), (1, 2, 2), (3, 1, 2), (3, 2, 2)]
    return [0, 5], result(rows), [job(max_gap=[0, 2, 0, 0], min_len=[3, 1, 1, 1])], claim


def length_filter():
    """lengths min_len - 1, min_len, min_len + 1; the removed trajectory had fillable gaps"""
    slots = {1: [0, 2], 2: [0, 2, 4], 3: [0, 1, 2, 4]}
    rows = [(s, 1, box(i, s), 0.5, i) for i, ss in slots.items() for s in ss]
    rows.sort(key=lambda r: r[0])

    def claim(refined):
        r = refined[0]
        assert sorted(set(r['object_id'])) == [2, 3]
        assert sorted((r['object_id'][i], r['frame'][i]) for i in fills(r)) == [(2, 1), (2, 3), (3, 3)]
        assert sorted((x['object_id'][i], x['frame'][i]) for x in [refined[1]] for i in fills(x)) == [(1, 1), (2, 1), (2, 3), (3, 3)]
    return [0, 5], result(rows), [job(max_gap=1, min_len=3), job(max_gap=1, min_len=2)], claim


def fractional_thirds(seed=5, n=40):
    """3-slot gaps between random fractional boxes: values where a fused multiply-add would round differently"""
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        for s in (0, 3):
            rows.append((s, 1 + i % 2, [rng.uniform(0, 1900), rng.uniform(0, 1200), rng.uniform(1, 300), rng.uniform(1, 300)], rng.random(), i))
    rows.sort(key=lambda r: r[0])

    def claim(refined):
        assert len(fills(refined[0])) == 2 * n
    return [0, 4], result(rows), [job(max_gap=2)], claim


def mean_scores(seed=9, n=70):
    """mean score over 3 .. 6 observations with gaps: sums that depend on the order of the additions"""
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        for s in sorted(rng.sample(range(8), 3 + i % 4)):
            rows.append((s, 1, box(i, s), rng.random(), i))
    rows.sort(key=lambda r: (r[0], -r[4]))

    def claim(refined):
        r = refined[0]
        per = {}
        for o, s in zip(r['object_id'], r['score']):
            per.setdefault(o, set()).add(s)
        assert all(len(v) == 1 for v in per.values()) and len(fills(r)) > n
    return [0, 8], result(rows), [job(max_gap=2, score_mode='mean'), job(max_gap=0, min_len=4, score_mode='mean')], claim


def many_trajectories(n):
    """n trajectories in one stream, one row each, plus a few with a gap: sizes on either side of the LDS limit of the tables"""
    rows = [(i % 3, 1 + (i % 2), box(i % 97, i % 3), 0.25 + (i % 50) * 0.01, i) for i in range(n)]
    late = [0, 1, 63, 64, n // 2, n - 2, n - 1]
    rows += [((i % 3) + 2, 1 + (i % 2), box(i % 97, 5), 0.75, i) for i in late]
    rows.sort(key=lambda r: r[0])

    def claim(refined):
        r = refined[0]
        assert len(r['frame']) == n + 2 * len(late) and sorted(set(r['object_id'][i] for i in fills(r))) == sorted(set(late))
        assert sorted(set(refined[1]['object_id'])) == sorted(set(late))
    return [0, 5], result(rows), [job(max_gap=1, score_mode='mean'), job(max_gap=1, min_len=2)], claim


CASES = {
    'same_gap_slot_65': lambda: same_gap_slot(65),
    'same_gap_slot_129': lambda: same_gap_slot(129),
    'crowded_slot_65': crowded_slot,
    'gap_limits': gap_limits,
    'neighbouring_streams': neighbouring_streams,
    'empty_result': empty_result,
    'classes': classes,
    'length_filter': length_filter,
    'fractional_thirds': fractional_thirds,
    'mean_scores': mean_scores,
}
