"""Adversarial inputs for the track stitching.  Every case is (stream_frame_offsets, result, jobs, claim):
`result` has the columns utils.track_packed returns, `jobs` are dicts as tracking/stitch.py takes them and claim(stitched) - given
the list of stitch_ref.stitch() outputs, one per job - asserts that the case is in the class its name says, with the reference
alone.  tests/test_stitch_cases.py runs the claims; tests/test_gpu_track_stitch.py compares the kernel with the reference."""
import math
import random
from fractions import Fraction

import stitch_ref
from track_cases import N_CLASSES, result


def job(max_link=0, link_iou=0.3, motion='hold'):
    per_class = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * N_CLASSES
    return {'max_link': per_class(max_link), 'link_iou': per_class(link_iou), 'motion': motion}


def stream_candidates(offsets, res, j, stream=0):
    return stitch_ref.candidates(stitch_ref.trajectories(offsets, res).get(stream, []), j)


def links_of(stitched):
    return sorted((f, t) for f, t, _, _ in stitched['links'])


def domino(n=70):
    """n tails end at slot 0, n heads start at slot 1, hold.  Head k = [20k, 20k + 10]; tail k reaches c_k into head k and
    c_k + 0.01 into head k - 1, c_k = 9 - 0.05 k: the affinities form one strictly descending chain a(0,0) > a(1,0) > a(1,1) >
    a(2,1) > ..., so that every tail but the first prefers a head whose best tail is the one before it - a matcher that works
    in rounds of mutually best pairs accepts exactly one pair per round, more rounds than a wavefront has lanes."""
    c = [9 - 0.05 * k for k in range(n)]
    rows = []
    for k in range(n):
        x0 = 0.0 if k == 0 else 20 * (k - 1) + 10 - (c[k] + 0.01)
        rows.append((0, 1, [x0, 0.0, 20 * k + c[k] - x0, 10.0], 0.9, k))
    rows += [(1, 1, [20.0 * k, 0.0, 10.0, 10.0], 0.8, n + k) for k in range(n)]
    jobs = [job(max_link=1, link_iou=0.05)]
    res = result(rows)

    def claim(stitched):
        cands = stream_candidates([0, 2], res, jobs[0])
        assert len(cands) == 2 * n - 1
        chain = sorted(cands, key=stitch_ref.order_key)
        assert all(chain[i][0] > chain[i + 1][0] for i in range(len(chain) - 1))             # strictly descending, no ties
        assert [(i, j - n) for _, _, i, j in chain] == [(k // 2 + k % 2, k // 2) for k in range(2 * n - 1)]
        links, rounds = stitch_ref.match_mutual_best(cands)
        assert rounds == n and n > 64
        assert links == stitch_ref.match_greedy(cands) and sorted((t, h) for h, (t, _, _) in links.items()) == [(k, n + k) for k in range(n)]
        assert links_of(stitched[0]) == [(k, n + k) for k in range(n)] and stitched[0]['n_links'] == [n]
    return [0, 2], res, jobs, claim


def ties():
    """Integer geometry in which every candidate shares its affinity with others, so that the answer rests on (n, i, j).
    Class 1: eight single-observation trajectories with one and the same box at slots 0, 0, 2, 3, 3, 3, 5, 5 - every affinity is 1.
    Walking (n, i, j): n = 1 gives 2 -> 3 (not 4, 5: the smaller head); n = 2 gives 0 -> 2 (not 1 -> 2: the smaller tail), 3 -> 6
    and 4 -> 7; n = 3 gives 1 -> 4.  Class 2: two per slot at x = 0 and x = 5, affinities 1 and 1/3."""
    box = [50.0, 50.0, 10.0, 10.0]
    rows = [(slot, 1, box, 0.9, i) for i, slot in enumerate((0, 0, 2, 3, 3, 3, 5, 5))]
    rows += [(i // 2, 2, [5.0 * (i % 2), 0.0, 10.0, 10.0], 0.9, 100 + i) for i in range(16)]
    rows.sort(key=lambda r: r[0])
    jobs = [job(max_link=3, link_iou=0.2), job(max_link=3, link_iou=0.2, motion='linear')]
    res = result(rows)

    def claim(stitched):
        cands = stream_candidates([0, 8], res, jobs[0])
        values = [c[0] for c in cands]
        assert sorted(set(values)) == [50.0 / 150.0, 1.0]
        tied = sum(1 for v in values if values.count(v) > 1)
        assert tied == len(cands) == 19 + 72                                                # every candidate shares its affinity
        first = [(0, 2), (1, 4), (2, 3), (3, 6), (4, 7)]
        assert links_of(stitched[0]) == first + [(100 + k, 102 + k) for k in range(14)]
        assert stitched[0]['object_id'].count(0) == 4 and stitched[0]['object_id'].count(1) == 3 and stitched[0]['object_id'].count(5) == 1
        for other in (lambda c: (-c[0], -c[1], c[2], c[3]), lambda c: (-c[0], c[1], -c[2], c[3]), lambda c: (-c[0], c[1], c[2], -c[3])):
            assert links_of(stitch_ref.stitch([0, 8], res, jobs[0], key=other))[:5] != first
        links, rounds = stitch_ref.match_mutual_best(cands)
        assert links == stitch_ref.match_greedy(cands) and rounds > 1
        assert stitched[1]['pred'] == stitched[0]['pred']                                   # single observations are held
    return [0, 8], res, jobs, claim


def row_of_trajectories(n):
    """n trajectories in one stream: the first half end at slot 0, the rest start at slot 2; tail i sits on head i, shifted a
    little more for every i, and reaches weakly into head i + 1"""
    tails = n // 2
    rows = [(0, 1 + i % 2, [40.0 * i + 0.05 * (i % 9), 1.0, 30.0, 20.0], 0.9, i) for i in range(tails)]
    rows += [(2, 1 + k % 2, [40.0 * k, 0.0, 30.0 + 12.0 * (k % 2), 20.0], 0.9, 1000 + k) for k in range(n - tails)]
    jobs = [job(max_link=2, link_iou=0.0), job(max_link=1, link_iou=0.0)]

    def claim(stitched):
        assert len(stitched[0]['pred']) == n
        assert links_of(stitched[0]) == [(i, 1000 + i) for i in range(tails)] and stitched[1]['n_links'] == [0]
    return [0, 3], result(rows), jobs, claim


def one_tail_many_heads(n=65):
    """one wide tail, n small heads inside it whose area - and with it the affinity - grows with the index: the best is the last"""
    rows = [(0, 1, [0.0, 0.0, 15.0 * n, 10.0], 0.9, 500)]
    rows += [(1, 1, [15.0 * k, 0.0, 10.0 + 0.01 * k, 10.0], 0.9, k) for k in range(n)]
    jobs = [job(max_link=1, link_iou=0.0)]
    res = result(rows)

    def claim(stitched):
        cands = stream_candidates([0, 2], res, jobs[0])
        assert len(cands) == n and len(set(c[0] for c in cands)) == n and all(c[2] == 0 for c in cands)
        assert max(cands)[3] == n and links_of(stitched[0]) == [(500, n - 1)]
    return [0, 2], res, jobs, claim


def best_head_in_another_chunk(tails=64, heads=66):
    """tail i sits on head heads - 1 - i: with the heads behind the tails in the index, the best head of tail 0 is index
    tails + heads - 1 (the third chunk of 64) and that of the last tail is in the second"""
    rows = [(0, 1, [20.0 * (heads - 1 - i) + 1.0 + 0.01 * i, 0.0, 10.0, 10.0], 0.9, i) for i in range(tails)]
    rows += [(1, 1, [20.0 * h, 0.0, 10.0, 10.0], 0.9, 100 + h) for h in range(heads)]
    jobs = [job(max_link=1, link_iou=0.3)]

    def claim(stitched):
        assert links_of(stitched[0]) == [(i, 100 + heads - 1 - i) for i in range(tails)]
        assert stitched[0]['pred'][tails + heads - 1] == 0 and stitched[0]['pred'][tails + heads - tails] == tails - 1 and tails + heads > 128
    return [0, 2], result(rows), jobs, claim


def threshold_edges():
    """link_iou equal to the pair's affinity and one ulp on either side of it; max_link equal to the gap and one below it"""
    rows = [(1, 2, [10.3, 20.7, 33.1, 41.9], 0.9, 1), (4, 2, [13.9, 18.2, 30.7, 44.3], 0.9, 2)]
    a = stitch_ref.affinity([(1, rows[0][2])], [(4, rows[1][2])], 'hold')
    jobs = [job(max_link=3, link_iou=a), job(max_link=3, link_iou=math.nextafter(a, 2.0)), job(max_link=3, link_iou=math.nextafter(a, 0.0)),
            job(max_link=2, link_iou=0.1), job(max_link=4, link_iou=0.1)]

    def claim(stitched):
        assert 0.5 < a < 0.9 and a != round(a, 6)
        assert [s['n_links'] for s in stitched] == [[1], [0], [1], [0], [1]]
        assert stitched[0]['affinity'] == [-1.0, a] and stitched[0]['links'] == [(1, 2, 3, a)]
    return [0, 6], result(rows), jobs, claim


def contraction(seed=11, n=40):
    """linear extrapolation of fractional boxes over 3 slots from a step measured over 2: values where a fused multiply-add in
    px = x + rate * n would round differently"""
    rng = random.Random(seed)
    rows, tracks = [], []
    for i in range(n):
        # a small x and a large step: the rounding of rate * n is of the size of the sum's last bit
        x, y, w, h = rng.uniform(0, 8), 1000.0 * i + rng.uniform(0, 5), rng.uniform(200, 300), rng.uniform(200, 300)
        dx, dy = rng.uniform(20, 60), rng.uniform(-3, 3)
        obs = [(0, [x, y, w, h]), (2, [x + 2 * dx, y + 2 * dy, w, h]), (5, [x + 5 * dx + rng.uniform(-1, 1), y + 5 * dy + rng.uniform(-1, 1), w, h])]
        tracks.append(obs)
        rows += [(obs[0][0], 1 + i % 2, obs[0][1], 0.9, i), (obs[1][0], 1 + i % 2, obs[1][1], 0.9, i), (obs[2][0], 1 + i % 2, obs[2][1], 0.9, 100 + i)]
    rows.sort(key=lambda r: r[0])
    jobs = [job(max_link=3, link_iou=0.3, motion='linear'), job(max_link=3, link_iou=0.3, motion='hold')]

    def fused(v, v_before, e, p, k):
        rate = (v - v_before) / float(e - p)
        return float(Fraction(rate) * k + Fraction(v))                                      # exact, rounded once

    def differing(stitched):
        count = 0
        for obs, a in zip(tracks, stitched['affinity'][n:]):
            (p, before), (e, (x, y, w, h)), (s, head) = obs
            px, py = fused(x, before[0], e, p, s - e), fused(y, before[1], e, p, s - e)
            count += stitch_ref.iou_dd([px, py, px + w, py + h], [head[0], head[1], head[0] + head[2], head[1] + head[3]]) != a
        return count

    def claim(stitched):
        assert stitched[0]['n_links'] == [n] and links_of(stitched[0]) == [(i, 100 + i) for i in range(n)]
        assert stitched[0]['pred'] == [-1] * n + list(range(n))                              # the tails appear first: tail i, head n + i
        assert differing(stitched[0]) == CONTRACTION_DIFFERING > 0
        assert stitched[0]['affinity'] != stitched[1]['affinity']
    claim.differing = differing
    return [0, 6], result(rows), jobs, claim


CONTRACTION_DIFFERING = 5                            # of the 40 accepted affinities of contraction(): how many a fused px, py changes


def isolation():
    """perfectly overlapping pieces of different classes, and of different streams (slot 2 ends stream 0, slot 3 starts stream 1),
    never link; the same pair of one class and stream does; per-class parameters"""
    box = [100.0, 50.0, 40.0, 30.0]
    rows = [(0, 1, box, 0.9, 1), (1, 2, box, 0.9, 2), (2, 4, [300.0, 50.0, 40.0, 30.0], 0.9, 3),
            (3, 4, [300.0, 50.0, 40.0, 30.0], 0.9, 4), (4, 1, box, 0.9, 5), (5, 1, box, 0.9, 6), (4, 2, box, 0.9, 7), (5, 2, box, 0.9, 8)]
    jobs = [job(max_link=1, link_iou=0.9), job(max_link=[0, 1, 1, 1], link_iou=0.9), job(max_link=2, link_iou=[0.9, 1.5, 0.9, 0.9])]

    def claim(stitched):
        assert links_of(stitched[0]) == [(5, 6), (7, 8)] and stitched[0]['n_links'] == [0, 2]
        assert links_of(stitched[1]) == [(7, 8)]
        assert links_of(stitched[2]) == [(5, 6)]                                            # no IoU reaches 1.5
        assert stitched[0]['object_id'] == [1, 2, 3, 4, 5, 5, 7, 7]
    return [0, 3, 6], result(rows), jobs, claim


def chain_of_five():
    """one object moving on a line, cut into 5 pieces of 2 observations with 2 empty slots between them; a second object nearby"""
    rows = []
    for piece in range(5):
        for k in range(2):
            slot = 4 * piece + k
            rows.append((slot, 1, [10.0 + 3.5 * slot, 20.0 + 1.25 * slot, 30.0, 40.0], 0.9, 10 * (piece + 1)))
    rows += [(slot, 1, [10.0 + 3.5 * slot, 75.0 + 1.25 * slot, 30.0, 40.0], 0.8, 7) for slot in range(0, 18, 3)]
    rows.sort(key=lambda r: r[0])
    jobs = [job(max_link=3, link_iou=0.8, motion='linear'), job(max_link=2, link_iou=0.3, motion='linear'), job(max_link=3, link_iou=0.8)]

    def claim(stitched):
        assert links_of(stitched[0]) == [(10, 20), (20, 30), (30, 40), (40, 50)]
        assert sorted(set(stitched[0]['object_id'])) == [7, 10] and stitched[0]['object_id'].count(10) == 10
        assert sorted(set(stitched[0]['root'])) == [0, 1] and stitched[1]['n_links'] == [0] and stitched[2]['n_links'] == [0]
    return [0, 18], result(rows), jobs, claim


def empty_result():
    def claim(stitched):
        assert stitched[0]['object_id'] == [] and stitched[0]['n_links'] == [0, 0] and stitched[0]['pred'] == []
    return [0, 2, 4], result([]), [job(max_link=3)], claim


def many_trajectories(n):
    """n single-observation trajectories in one stream at slots i % 8, groups of 8 forming chains along x: sizes on either side of
    the LDS limit of the match tables; local indices run slot-major, so a chain's links cross the whole index range"""
    groups = (n + 7) // 8
    rows = [(i % 8, 1 + (i // 8) % 2, [40.0 * (i // 8) + 3.7 * (i % 8), 0.5 * (i % 8), 30.0, 20.0], 0.9, i) for i in range(n)]
    rows.sort(key=lambda r: r[0])
    jobs = [job(max_link=1, link_iou=0.5), job(max_link=2, link_iou=0.5, motion='linear')]

    def claim(stitched):
        s = stitched[0]
        assert len(s['pred']) == n and s['n_links'] == [n - groups]
        assert sorted(set(s['object_id'])) == list(range(0, n, 8)) and sorted(set(s['root'])) == list(range(groups))
        assert stitched[1]['n_links'] == [n - groups]
    return [0, 8], result(rows), jobs, claim


CASES = {
    'domino_70': domino,
    'ties': ties,
    'trajectories_63': lambda: row_of_trajectories(63),
    'trajectories_64': lambda: row_of_trajectories(64),
    'trajectories_65': lambda: row_of_trajectories(65),
    'one_tail_65_heads': one_tail_many_heads,
    'best_head_in_another_chunk': best_head_in_another_chunk,
    'threshold_edges': threshold_edges,
    'contraction': contraction,
    'isolation': isolation,
    'chain_of_five': chain_of_five,
    'empty_result': empty_result,
    'many_trajectories_200': lambda: many_trajectories(200),
}
