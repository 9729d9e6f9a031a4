"""Adversarial inputs for the track smoothing.  Every case is (stream_frame_offsets, result, jobs, claim):
`result` has the columns utils.track_packed returns, `jobs` are dicts as tracking/smooth.py takes them and claim(smoothed) - given
the list of smooth_ref.smooth() outputs, one per job - asserts that the case is in the class its name says, with the reference
alone.  tests/test_smooth_cases.py runs the claims; tests/test_gpu_track_smooth.py compares the kernel with the reference."""
import math
import random

import smooth_ref
from track_cases import N_CLASSES, result


def job(window=0, weights=None, sigma=1.0, kernel='gaussian', n_weights=None):
    """window: one value or one per class; weights: one table for every class, or kernel / sigma as tracking/smooth.py computes them"""
    w = list(window) if isinstance(window, (list, tuple)) else [window] * N_CLASSES
    n = n_weights or max(w) + 1
    if weights is None:
        weights = smooth_ref.box(n) if kernel == 'box' else smooth_ref.gaussian(sigma, n)
    return {'window': w, 'weights': [list(weights) for _ in range(N_CLASSES)]}


def box_of(i, slot, rng=None):
    """a box that depends on trajectory and slot, with fractions that are not dyadic"""
    jitter = (lambda: rng.uniform(-1.5, 1.5)) if rng else (lambda: 0.0)
    return [37.3 * i + 3.1 * slot + jitter(), 11.7 + 1.9 * slot + jitter(), 41.3 + 0.7 * (slot % 5) + jitter(), 29.9 + 0.3 * (slot % 3) + jitter()]


def rows_of(res, oid):
    """{slot: caller's row} of one object id"""
    return dict((res['frame'][i], i) for i in range(len(res['frame'])) if res['object_id'][i] == oid)


def same_bits(a, b):
    return a == b and math.copysign(1.0, a) == math.copysign(1.0, b) if a == a or b == b else True


def unchanged(res, smoothed, i):
    return smoothed['pairs'][i] == 0 and all(same_bits(a, b) for a, b in zip(smoothed['bbox'][i], res['bbox'][i]))


def contraction(seed=5, n_traj=5, n_slots=18):
    """fractional boxes, Gaussian sigma 1.5, W = 3, about 15 % holes: values where a fused multiply-add, the descending order of the
    distances or k * a + k * b in place of k * (a + b) would round differently"""
    rng = random.Random(seed)
    rows = []
    for i in range(n_traj):
        for slot in range(n_slots):
            if rng.random() < 0.15:
                continue
            rows.append((slot, 1 + i % 2, box_of(i, slot, rng), 0.9, i))
    rows.sort(key=lambda r: r[0])
    res = result(rows)
    jobs = [job(window=3, sigma=1.5)]

    def differing(smoothed, variant):
        other = smooth_ref.smooth([0, n_slots], res, jobs[0], variant)
        return sum(1 for a, b in zip(smoothed['bbox'], other['bbox']) for u, v in zip(a, b) if u != v), 4 * len(rows)

    def claim(smoothed):
        holes = n_traj * n_slots - len(rows)
        assert 0.08 * n_traj * n_slots < holes < 0.25 * n_traj * n_slots
        counts = dict((v, differing(smoothed[0], v)[0]) for v in ('fused', 'descending', 'split'))
        assert all(n > 0 for n in counts.values()), counts
        assert counts == CONTRACTION_DIFFERING, counts
        assert sorted(set(smoothed[0]['pairs'])) == [0, 1, 2, 3]
    claim.differing = differing
    return [0, n_slots], res, jobs, claim


CONTRACTION_DIFFERING = {'fused': 55, 'descending': 48, 'split': 37}      # of the 292 values of contraction(): how many each variant changes


def holes():
    """W = 3 around slot 10: for every distance 1..3 one trajectory misses the row before and one the row after.  The other side is
    there, so a walk along the chain must step over it without counting it and still find the next distance."""
    rows, oid = [], 0
    for d in (1, 2, 3):
        for side in (-1, 1):
            rows += [(slot, 1, box_of(oid, slot), 0.9, oid) for slot in range(7, 14) if slot != 10 + side * d]
            oid += 1
    rows += [(slot, 1, box_of(oid, slot), 0.9, oid) for slot in range(7, 14)]
    rows.sort(key=lambda r: r[0])
    res = result(rows)
    jobs = [job(window=3, sigma=2.0)]

    def claim(smoothed):
        for t in range(6):
            d = t // 2 + 1
            centre = rows_of(res, t)[10]
            assert smoothed[0]['pairs'][centre] == 2
            # the answer is the one of the distances that are left
            k = jobs[0]['weights'][0]
            for col in range(4):
                values = dict((s, res['bbox'][i][col]) for s, i in rows_of(res, t).items())
                acc, den = k[0] * values[10], k[0]
                for e in (1, 2, 3):
                    if e != d:
                        acc = acc + k[e] * (values[10 - e] + values[10 + e])
                        den = den + (k[e] + k[e])
                assert smoothed[0]['bbox'][centre][col] == acc / den
        assert smoothed[0]['pairs'][rows_of(res, 6)[10]] == 3
    return [0, 16], res, jobs, claim


def ends(W=3):
    """trajectories of 1, 2, 3 and 2 W + 1 rows (the first two are shorter than W): the first and the last row never move"""
    lengths = [1, 2, 3, 2 * W + 1]
    rows = [(2 + slot, 1 + t % 2, box_of(t, slot), 0.9, t) for t, n in enumerate(lengths) for slot in range(n)]
    rows.sort(key=lambda r: r[0])
    res = result(rows)
    jobs = [job(window=W, sigma=1.0), job(window=W, kernel='box')]

    def claim(smoothed):
        for s in smoothed:
            for t, n in enumerate(lengths):
                at = rows_of(res, t)
                assert unchanged(res, s, at[2]) and unchanged(res, s, at[2 + n - 1])
                assert [s['pairs'][at[2 + k]] for k in range(n)] == [min(k, n - 1 - k, W) for k in range(n)]
        mid = rows_of(res, 2)[3]
        assert smoothed[1]['bbox'][mid][0] == (res['bbox'][mid][0] + (res['bbox'][rows_of(res, 2)[2]][0] + res['bbox'][rows_of(res, 2)[4]][0])) / 3.0
    return [0, 12], res, jobs, claim


def window_edges():
    """W = 0 for class 1 next to W > 0 for class 2; W = 32, the largest, with exactly W + 1 weights; and a trajectory whose rows
    change category: its class is that of its first observation"""
    rows = [(slot, 1, box_of(0, slot), 0.9, 0) for slot in range(6)]
    rows += [(slot, 2, box_of(1, slot), 0.9, 1) for slot in range(6)]
    rows += [(slot, 3, box_of(2, slot), 0.9, 2) for slot in range(67)]
    rows += [(slot, 2 if slot == 0 else 1, box_of(3, slot), 0.9, 3) for slot in range(6)]
    rows += [(slot, 1 if slot == 0 else 2, box_of(4, slot), 0.9, 4) for slot in range(6)]
    rows.sort(key=lambda r: r[0])
    res = result(rows)
    jobs = [job(window=[0, 2, 32, 1], sigma=9.0), job(window=[0, 2, 32, 1], kernel='box')]

    def claim(smoothed):
        assert all(len(k) == 33 for k in jobs[0]['weights']) and smooth_ref.MAX_WINDOW == 32
        for s in smoothed:
            assert all(unchanged(res, s, i) for i in rows_of(res, 0).values())
            assert [s['pairs'][rows_of(res, 1)[k]] for k in range(6)] == [0, 1, 2, 2, 1, 0]
            assert [s['pairs'][rows_of(res, 2)[k]] for k in (31, 32, 33, 34, 35)] == [31, 32, 32, 32, 31]
            assert [s['pairs'][rows_of(res, 3)[k]] for k in range(6)] == [0, 1, 2, 2, 1, 0]       # rows of category 1, a trajectory of class 2
            assert all(unchanged(res, s, i) for i in rows_of(res, 4).values())                    # and the other way round
    return [0, 67], res, jobs, claim


def lanes(n):
    """n trajectories in every one of three slots: the rows of a slot fill a wavefront exactly, or fall one short, or spill over"""
    rows = [(slot, 1 + t % 4, box_of(t, slot), 0.9, 100 + t) for slot in (1, 2, 3) for t in range(n)]
    res = result(rows)
    jobs = [job(window=1, kernel='box'), job(window=[2, 1, 2, 0], sigma=0.8)]

    def claim(smoothed):
        assert len(rows) == 3 * n
        assert smoothed[0]['pairs'] == [0] * n + [1] * n + [0] * n
        assert smoothed[1]['pairs'] == [0] * n + [0 if t % 4 == 3 else 1 for t in range(n)] + [0] * n
    return [0, 5], res, jobs, claim


def many_trajectories(n):
    """n trajectories of three rows in one stream, starting at slots i % 6: sizes on either side of the LDS limit of the link table"""
    rows = [(i % 6 + k, 1 + i % 2, [40.0 * i + 3.7 * k * k, 0.5 * k + 0.1 * (i % 7), 30.0 + k, 20.0 + 0.3 * k], 0.9, i) for i in range(n) for k in range(3)]
    rows.sort(key=lambda r: r[0])
    res = result(rows)
    jobs = [job(window=2, sigma=1.0)]

    def claim(smoothed):
        assert len(set(res['object_id'])) == n and sum(smoothed[0]['pairs']) == n
        last = rows_of(res, n - 1)
        mid = last[(n - 1) % 6 + 1]
        assert smoothed[0]['pairs'][mid] == 1 and smoothed[0]['bbox'][mid][0] != res['bbox'][mid][0]
    return [0, 8], res, jobs, claim


def two_streams():
    """slot 4 ends stream 0 and slot 5 starts stream 1; the same object ids - and so the same local indices - live in both: a row
    never pairs across the boundary"""
    rows = [(slot, 1, box_of(t, slot), 0.9, t) for slot in range(2, 9) for t in (0, 1)]
    res = result(rows)
    jobs = [job(window=2, kernel='box')]

    def claim(smoothed):
        for t in (0, 1):
            at = rows_of(res, t)
            assert [smoothed[0]['pairs'][at[s]] for s in range(2, 9)] == [0, 1, 0, 0, 1, 1, 0]
        one = smooth_ref.smooth([0, 10], res, jobs[0])                                            # the same rows as one stream
        assert [one['pairs'][rows_of(res, 0)[s]] for s in range(2, 9)] == [0, 1, 2, 2, 2, 1, 0]
    return [0, 5, 10], res, jobs, claim


def non_finite():
    """one NaN x at slot 4 of a trajectory over slots 0..8, W = 1: the row and its two neighbours turn NaN in x, nothing else does;
    an infinite y at slot 6 of another one"""
    rows = [(slot, 1, box_of(0, slot), 0.9, 0) for slot in range(9)] + [(slot, 2, box_of(1, slot), 0.9, 1) for slot in range(9)]
    rows.sort(key=lambda r: r[0])
    res = result(rows)
    res['bbox'][rows_of(res, 0)[4]][0] = float('nan')
    res['bbox'][rows_of(res, 1)[6]][1] = float('inf')
    jobs = [job(window=1, kernel='box'), job(window=2, sigma=1.0)]

    def claim(smoothed):
        at = rows_of(res, 0)
        nan_rows = [s for s in range(9) if smoothed[0]['bbox'][at[s]][0] != smoothed[0]['bbox'][at[s]][0]]
        assert nan_rows == [3, 4, 5]
        assert all(v == v for s in range(9) for v in smoothed[0]['bbox'][at[s]][1:])
        wide = [s for s in range(9) if smoothed[1]['bbox'][at[s]][0] != smoothed[1]['bbox'][at[s]][0]]
        assert wide == [2, 3, 4, 5, 6]
        other = rows_of(res, 1)
        assert [s for s in range(9) if math.isinf(smoothed[0]['bbox'][other[s]][1])] == [5, 6, 7]
    return [0, 9], res, jobs, claim


def empty_result():
    def claim(smoothed):
        assert smoothed[0]['bbox'] == [] and smoothed[0]['pairs'] == []
    return [0, 2, 4], result([]), [job(window=3)], claim


CASES = {
    'contraction': contraction,
    'holes': holes,
    'ends': ends,
    'window_edges': window_edges,
    'lanes_63': lambda: lanes(63),
    'lanes_64': lambda: lanes(64),
    'lanes_65': lambda: lanes(65),
    'many_trajectories_200': lambda: many_trajectories(200),
    'two_streams': two_streams,
    'non_finite': non_finite,
    'empty_result': empty_result,
}
