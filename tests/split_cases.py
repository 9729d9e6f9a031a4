"""Adversarial inputs for the track splitting.  Every case is (stream_frame_offsets, result, jobs, claim):
`result` has the columns utils.track_packed returns, `jobs` are dicts as tracking/split.py takes them and claim(done) - given the
list of split_ref.split() outputs, one per job - asserts that the case is in the class its name says, with the reference alone.
tests/test_split_cases.py runs the claims; tests/test_gpu_track_split.py compares the kernels with the reference."""
import math
import random
from fractions import Fraction

import split_ref
from track_cases import N_CLASSES, by_slot, result

NAN = float('nan')


def job(split_iou=0.0, split_gap=0, motion='linear', first_new_id=None):
    per_class = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * N_CLASSES
    j = {'split_iou': per_class(split_iou), 'split_gap': per_class(split_gap), 'motion': motion}
    if first_new_id is not None:
        j['first_new_id'] = first_new_id
    return j


def line(oid, slots, v=40.0, y=0.0, cls=1, jump=None):
    """one object on a line: box [v * f, y, 50, 40] at every slot of `slots`; jump = {slot: dx}"""
    return [(f, cls, [v * f + (jump or {}).get(f, 0.0), y, 50.0, 40.0], 0.9, oid) for f in slots]


def pieces_of(done, res, oid):
    """the pieces of the rows that carried `oid` in the input, in slot order"""
    rows = sorted((res['frame'][i], done['piece'][i]) for i in range(len(res['frame'])) if res['object_id'][i] == oid)
    return [p for _, p in rows]


def threshold_edge():
    """Boxes [0, 0, 3, 1] and [1, 0, 3, 1] meet in 2 of 4: the IoU is exactly 0.5.  A pair breaks when a < split_iou: not at 0.5, and
    at the next float64 above it."""
    rows = [(0, 1, [0.0, 0.0, 3.0, 1.0], 0.9, 7), (1, 1, [1.0, 0.0, 3.0, 1.0], 0.9, 7)]
    above = math.nextafter(0.5, 1.0)
    jobs = [job(0.5, motion='hold'), job(above, motion='hold'), job(0.5), job(above)]
    res = result(rows)

    def claim(done):
        assert above > 0.5 and above - 0.5 == 2.0 ** -53
        for k, d in enumerate(done):
            assert d['test'] == [[-1.0, -1.0], [0.5, -1.0]]              # two rows: the hold test under either motion
            assert d['piece'] == [0, k % 2] and d['n_new'] == k % 2 and d['object_id'] == [7, 7 + k % 2]
    return [0, 2], res, jobs, claim


def exact_tests(rows_of_traj, n_pair, motion='linear'):
    """the two tests of pair (i - 1, i) = n_pair of one trajectory [(slot, [x, y, w, h])] as Fractions of the exactly extrapolated
    position rounded once: what a fused rate * n + v gives"""
    i = n_pair
    n = rows_of_traj[i][0] - rows_of_traj[i - 1][0]

    def fused(v, other, slots):
        rate = (v - other) / float(slots)
        return float(Fraction(rate) * n + Fraction(v))

    found = [None, None]
    if i >= 2:
        p = rows_of_traj[i - 1][0] - rows_of_traj[i - 2][0]
        x, y, w, h = rows_of_traj[i - 1][1]
        px, py = fused(x, rows_of_traj[i - 2][1][0], p), fused(y, rows_of_traj[i - 2][1][1], p)
        found[0] = split_ref.iou_dd([px, py, px + w, py + h], split_ref.corners(rows_of_traj[i][1]))
    if i + 1 < len(rows_of_traj):
        q = rows_of_traj[i + 1][0] - rows_of_traj[i][0]
        x, y, w, h = rows_of_traj[i][1]
        px, py = fused(x, rows_of_traj[i + 1][1][0], q), fused(y, rows_of_traj[i + 1][1][1], q)
        found[1] = split_ref.iou_dd([px, py, px + w, py + h], split_ref.corners(rows_of_traj[i - 1][1]))
    return found


def contraction():
    """Fractional boxes a few hundredths of a pixel wide that move several pixels per slot and pass the origin, with holes of
    1..3 slots around a middle pair of n = 3: the move rate * n is larger than the position it leads to and than the box, so
    rate * n + v rounded once (a fused multiply-add) differs from the two roundings of the definition in the last bits of out_test.
    claim.differing(done) counts the values that tell the two apart."""
    rng = random.Random(11)
    rows, trajs = [], {}
    for oid in range(24):
        p, q = rng.choice((1, 2, 3)), rng.choice((1, 2, 3))
        rx, ry = rng.uniform(2.0, 7.0) / 3.0, rng.uniform(2.0, 7.0) / 7.0
        w, h = rng.uniform(0.02, 0.05), rng.uniform(0.02, 0.05)
        x1, y1 = 3.0 * rx + rng.uniform(-0.01, 0.01), 3.0 * ry + rng.uniform(-0.01, 0.01)
        x2, y2 = (x1 - 3.0 * rx) + rng.uniform(-0.004, 0.004), (y1 - 3.0 * ry) + rng.uniform(-0.004, 0.004)
        f0 = rng.randrange(2)
        obs = [(f0, [x1 + rx * p, y1 + ry * p, w, h]), (f0 + p, [x1, y1, w, h]), (f0 + p + 3, [x2, y2, w, h]),
               (f0 + p + 3 + q, [x2 - rx * q, y2 - ry * q, w, h])]
        rows += [(f, 1 + oid % 2, box, 0.9, oid) for f, box in obs]
        trajs[oid] = obs
    n_slots = max(r[0] for r in rows) + 1
    res = result(by_slot(rows))
    jobs = [job(0.05)]

    def differing(done):
        changed, of = 0, 0
        for i in range(len(res['frame'])):
            obs = trajs[res['object_id'][i]]
            k = [f for f, _ in obs].index(res['frame'][i])
            if k == 0:
                continue
            for got, other in zip(done['test'][i], exact_tests(obs, k)):
                if other is not None:
                    assert got >= 0.0
                    of += 1
                    changed += got != other
        return changed, of

    def claim(done):
        changed, of = differing(done[0])
        assert of == 24 * 4 and changed > 0
        assert done[0]['n_new'] == 0                                     # smooth motion: the values differ, no decision does
    claim.differing = differing
    return [0, n_slots], res, jobs, claim


def holes():
    """p, q and n each 1..3: a trajectory of six rows at slots 0, 1, 1 + p, 1 + p + n, 1 + p + n + q and the next on a line of
    constant velocity - every test of the middle pair is 1.0 whatever the holes - and the same with the line's second half moved
    away: one break, at the middle pair."""
    rows, oid = [], 0
    for p in (1, 2, 3):
        for n in (1, 2, 3):
            for q in (1, 2, 3):
                slots = [0, 1, 1 + p, 1 + p + n, 1 + p + n + q, 2 + p + n + q]
                rows += line(oid, slots, v=8.0, y=100.0 * oid)
                rows += line(oid + 1, slots, v=8.0, y=100.0 * oid + 50.0, jump={f: 300.0 for f in slots[3:]})
                oid += 2
    res = result(by_slot(rows))
    jobs = [job(0.9)]

    def claim(done):
        for o in range(0, oid, 2):
            assert pieces_of(done[0], res, o) == [0] * 6 and pieces_of(done[0], res, o + 1) == [0, 0, 0, 1, 1, 1]
        mid = [done[0]['test'][i] for i in range(len(res['frame'])) if res['object_id'][i] % 2 == 0]
        assert sum(1 for t in mid if t == [1.0, 1.0]) == 27 * 3          # the pairs 2, 3, 4 of every straight trajectory have both tests
        assert done[0]['n_new'] == 27
    return [0, 12], res, jobs, claim


def ends():
    """Trajectories of 1, 2, 3 and 4 rows: which tests exist.  1: none.  2: hold.  3: backward at the first pair, forward at the
    second.  4: the middle pair has both."""
    rows = []
    for m in (1, 2, 3, 4):
        rows += line(m, range(m), v=6.0, y=100.0 * m, cls=m)
    res = result(by_slot(rows))
    jobs = [job(0.3), job(0.3, motion='hold')]

    def claim(done):
        shape = lambda d, oid: [tuple(v >= 0.0 for v in d['test'][i]) for i in sorted(range(len(res['frame'])), key=lambda i: res['frame'][i])
                                if res['object_id'][i] == oid]
        lin = done[0]
        assert shape(lin, 1) == [(False, False)]
        assert shape(lin, 2) == [(False, False), (True, False)]
        assert shape(lin, 3) == [(False, False), (False, True), (True, False)]
        assert shape(lin, 4) == [(False, False), (False, True), (True, True), (True, False)]
        for m in (1, 2, 3, 4):
            assert shape(done[1], m) == [(False, False)] + [(True, False)] * (m - 1)
        assert lin['n_new'] == 0 and done[1]['n_new'] == 0
    return [0, 4], res, jobs, claim


def disagreement():
    """Object 1 stands still for three slots and then moves 60 px per slot: at the pair (1, 2) the forward test (velocity 0) passes
    and the backward test (velocity 60) fails, at the pair (2, 3) it is the reverse.  Object 2 moves, then stands: the same two
    disagreements in the other order.  Neither breaks, and with hold every moving pair would."""
    xs1 = [0.0, 0.0, 0.0, 60.0, 120.0, 180.0]
    xs2 = [0.0, 60.0, 120.0, 180.0, 180.0, 180.0]
    rows = [(f, 1, [xs1[f], 0.0, 50.0, 40.0], 0.9, 1) for f in range(6)] + [(f, 1, [xs2[f], 200.0, 50.0, 40.0], 0.9, 2) for f in range(6)]
    res = result(by_slot(rows))
    jobs = [job(0.3), job(0.3, motion='hold')]

    def claim(done):
        test = lambda oid, f: [done[0]['test'][i] for i in range(12) if res['object_id'][i] == oid and res['frame'][i] == f][0]
        assert test(1, 2) == [1.0, 0.0] and test(1, 3) == [0.0, 1.0] and test(2, 3) == [1.0, 0.0] and test(2, 4) == [0.0, 1.0]
        assert done[0]['n_new'] == 0 and done[0]['piece'] == [0] * 12
        assert done[1]['n_new'] == 6                                     # hold: every moving pair breaks
    return [0, 6], res, jobs, claim


def gap_rule():
    """Observations at slots 0, 1, 2, 5, 6, 7 (n = 3 in the middle) on a straight line, and one whose second half is elsewhere.
    split_gap 3: n = split_gap does not break; split_gap 2: n = split_gap + 1 does; with the IoU rule on, either rule breaks."""
    slots = [0, 1, 2, 5, 6, 7]
    rows = line(1, slots, v=5.0) + line(2, slots, v=5.0, y=100.0, jump={5: 400.0, 6: 400.0, 7: 400.0})
    res = result(by_slot(rows))
    jobs = [job(0.0, 3), job(0.0, 2), job(0.3, 3), job(0.3, 2), job(0.3, 0), job(0.0, 0)]

    def claim(done):
        got = [(pieces_of(d, res, 1), pieces_of(d, res, 2)) for d in done]
        whole, cut = [0] * 6, [0, 0, 0, 1, 1, 1]
        assert got[0] == (whole, whole) and got[1] == (cut, cut)
        assert got[2] == (whole, cut) and got[3] == (cut, cut)
        assert got[4] == got[2] and got[5] == got[0]
        for d in done[:2] + done[5:]:                                    # IoU rule off: no test is reported
            assert all(t == [-1.0, -1.0] for t in d['test'])
        assert done[1]['new'] == [-1] * 6 + [0, 1] * 3 and done[1]['n_new_pieces'] == [2]
    return [0, 8], res, jobs, claim


def classes():
    """The same jump in classes 1 and 2, the rule on for class 1 only; a trajectory that starts in class 2 and changes to class 1
    (it is of class 2: off); one that starts in class 1 and changes to class 3 (of class 1: on)."""
    jump = {f: 400.0 for f in range(4, 8)}
    rows = line(1, range(8), cls=1, jump=jump) + line(2, range(8), y=100.0, cls=2, jump=jump)
    rows += [(f, 2 if f < 2 else 1, b, s, 3) for f, _, b, s, _ in line(0, range(8), y=200.0, jump=jump)]
    rows += [(f, 1 if f < 2 else 3, b, s, 4) for f, _, b, s, _ in line(0, range(8), y=300.0, jump=jump)]
    res = result(by_slot(rows))
    jobs = [job([0.3, 0.0, 0.0, 0.0]), job([0.0, 0.3, 0.3, 0.3])]

    def claim(done):
        cut, whole = [0] * 4 + [1] * 4, [0] * 8
        assert [pieces_of(done[0], res, o) for o in (1, 2, 3, 4)] == [cut, whole, whole, cut]
        assert [pieces_of(done[1], res, o) for o in (1, 2, 3, 4)] == [whole, cut, cut, whole]
        assert done[0]['breaks'] == [1, 0, 0, 1] and done[0]['object_id'].count(5) == 4 and done[0]['object_id'].count(6) == 4
    return [0, 8], res, jobs, claim


def extremes(m=200):
    """200 rows: a zig-zag whose every pair fails all tests - every pair breaks, 199 new ids - and a straight line - none does."""
    rows = [(f, 1, [1000.0 * (f % 2) + 300.0 * (f % 3), 0.0, 50.0, 40.0], 0.9, 1) for f in range(m)] + line(2, range(m), v=3.0, y=100.0)
    res = result(by_slot(rows))
    jobs = [job(0.3), job(0.3, motion='hold')]

    def claim(done):
        for d in done:
            assert pieces_of(d, res, 1) == list(range(m)) and pieces_of(d, res, 2) == [0] * m
            assert d['breaks'] == [m - 1, 0] and d['n_new'] == m - 1 and sorted(v for v in d['new'] if v >= 0) == list(range(m - 1))
            assert sorted(set(d['object_id'])) == [1, 2] + list(range(3, 3 + m - 1))
    return [0, m], res, jobs, claim


def non_finite():
    """A NaN coordinate: every test it enters is NaN, and a NaN never breaks.  An infinite x: the box's width inf - inf is NaN, so
    is every test.  An infinite width: the union is infinite, the IoU 0 - the row is cut out like any outlier."""
    rows = line(1, range(6), v=5.0) + line(2, range(6), v=5.0, y=100.0) + line(3, range(6), v=5.0, y=200.0)
    rows = [list(r) for r in rows]
    rows[3][2][0] = NAN                                                  # object 1, slot 3
    rows[6 + 3][2][0] = math.inf                                         # object 2, slot 3
    rows[12 + 3][2][2] = math.inf                                        # object 3, slot 3: infinite width
    res = result(by_slot([tuple(r) for r in rows]))
    jobs = [job(0.3), job(0.3, motion='hold')]

    def claim(done):
        for d in done:
            nan_tests = sum(1 for t in d['test'] for v in t if v != v)
            assert nan_tests > 0
            for i in range(len(res['frame'])):                           # a pair whose every test is NaN does not break
                t = [v for v in d['test'][i] if v != -1.0]
                if t and all(v != v for v in t):
                    prev = [k for k in range(len(res['frame'])) if res['object_id'][k] == res['object_id'][i] and res['frame'][k] == res['frame'][i] - 1][0]
                    assert d['piece'][i] == d['piece'][prev]
        for d in done:
            assert pieces_of(d, res, 1) == [0] * 6 and pieces_of(d, res, 2) == [0] * 6 and pieces_of(d, res, 3) == [0, 0, 0, 1, 2, 2]
    return [0, 6], res, jobs, claim


def stream_sharing():
    """The same object ids in two streams are different trajectories: the one of stream 0 jumps, the one of stream 1 does not; new
    pieces are numbered stream after stream."""
    rows = line(1, range(6), jump={f: 400.0 for f in (3, 4, 5)}) + line(2, range(6), y=100.0)
    rows += line(1, range(6, 12), y=0.0) + line(2, range(6, 12), y=100.0, jump={f: 400.0 for f in (9, 10, 11)})
    rows += line(2, range(12, 18), y=100.0, jump={15: 400.0, 16: 400.0, 17: 400.0})
    res = result(by_slot(rows))
    jobs = [job(0.3), job(0.3, first_new_id=100)]

    def claim(done):
        assert done[0]['n_new_pieces'] == [1, 1, 1] and done[0]['traj_offsets'] == [0, 2, 4, 5] and done[0]['breaks'] == [1, 0, 0, 1, 1]
        ids = lambda d, lo, hi, oid: sorted(set(d['object_id'][i] for i in range(len(res['frame'])) if lo <= res['frame'][i] < hi and res['object_id'][i] == oid))
        assert ids(done[0], 0, 6, 1) == [1, 3] and ids(done[0], 6, 12, 1) == [1] and ids(done[0], 6, 12, 2) == [2, 4] and ids(done[0], 12, 18, 2) == [2, 5]
        assert ids(done[1], 0, 6, 1) == [1, 100] and ids(done[1], 12, 18, 2) == [2, 102]
    return [0, 6, 12, 18], res, jobs, claim


def many_in_a_slot(n, breaks_of=lambda k: k % 3, empty_stream=False):
    """n trajectories side by side, all present in every slot; trajectory k has breaks_of(k) jumps.  With empty_stream: the same n
    again in a third stream, behind one without rows - the scans of the breaks then cross lane, chunk and stream edges."""
    def stream(first, base_id):
        rows = []
        for k in range(n):
            b = breaks_of(k)
            jump = {f: (400.0 if (b >= 1 and f >= 3) else 0.0) + (400.0 if (b >= 2 and f >= 6) else 0.0) for f in range(10)}
            rows += [(first + f, 1 + k % 4, box, s, base_id + k) for f, _, box, s, _ in line(0, range(10), v=4.0, y=60.0 * k, jump=jump)]
        return rows
    rows = stream(0, 0)
    offsets = [0, 10]
    if empty_stream:
        rows += stream(12, n)
        offsets = [0, 10, 12, 22]
    res = result(by_slot(rows))
    jobs = [job(0.3), job([0.3, 0.0, 0.3, 0.3], motion='hold')]

    def claim(done):
        expect = [breaks_of(k) for k in range(n)]
        assert done[0]['breaks'] == expect * (2 if empty_stream else 1)
        assert done[0]['n_new_pieces'] == ([sum(expect), 0, sum(expect)] if empty_stream else [sum(expect)])
        fresh = sorted(set(v for v in done[0]['new'] if v >= 0))
        assert fresh == list(range(done[0]['n_new']))                    # every new piece has its own number, none missing
        assert [b for k, b in enumerate(done[1]['breaks'][:n]) if k % 4 == 1] == [0] * len(range(1, n, 4))
    return offsets, res, jobs, claim


CASES = {
    'threshold_edge': threshold_edge,
    'contraction': contraction,
    'holes': holes,
    'ends': ends,
    'disagreement': disagreement,
    'gap_rule': gap_rule,
    'classes': classes,
    'extremes': extremes,
    'non_finite': non_finite,
    'stream_sharing': stream_sharing,
}
