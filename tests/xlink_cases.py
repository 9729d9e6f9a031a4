"""Adversarial inputs for the cross-class track linking.  Every case is (stream_frame_offsets, result, jobs,
claim): `result` has the columns utils.track_packed returns, `jobs` are dicts as tracking/xlink.py takes them and claim(linked) -
given the list of xlink_ref.xlink() outputs, one per job - asserts that the case is in the class its name says, with the reference
alone.  tests/test_xlink_cases.py runs the claims; tests/test_gpu_track_xlink.py compares the kernel with the reference.
Every case has 4 classes but sixteen_classes(), which the tests run with n_classes = 16."""
import math

import numpy as np

import stitch_ref
import xlink_ref
from track_cases import N_CLASSES, result

WAVE = 64                                            # lanes of a wavefront: a lane owns the tails i, i + 64, ...


def pair(max_link=1, link_iou=0.3):
    return {'max_link': max_link, 'link_iou': link_iou}


def job(pairs, prio=0, motion='hold'):
    return {'pairs': dict(pairs), 'prio': prio, 'motion': motion}


def stream_candidates(offsets, res, j, stream=0, n_classes=N_CLASSES):
    return xlink_ref.candidates(stitch_ref.trajectories(offsets, res).get(stream, []), j, n_classes)


def links_of(linked):
    return sorted((f, t) for f, t, _, _ in linked['links'])


def greedy_equals_mutual_best(offsets, res, jobs, n_classes=N_CLASSES):
    """on every stream and job of a case: the rounds of mutually best pairs give the greedy answer; returns the rounds per job of stream 0"""
    rounds = []
    for j in jobs:
        for s in range(len(offsets) - 1):
            cands = stream_candidates(offsets, res, j, s, n_classes)
            links, n = stitch_ref.match_mutual_best(cands)
            assert links == stitch_ref.match_greedy(cands), (s, j)
            if s == 0:
                rounds.append(n)
    return rounds


def one_tail_many_heads(n=65):
    """one wide tail of class 2, n small heads inside it whose classes alternate 4, 2, 4, ... and whose area - and with it the
    affinity - grows with the index: the best is the last, a class-4 head in the second chunk of 64; with only (2, 2) on it is
    the last class-2 head"""
    rows = [(0, 2, [0.0, 0.0, 15.0 * n, 10.0], 0.9, 500)]
    rows += [(1, 4 if k % 2 == 0 else 2, [15.0 * k, 0.0, 10.0 + 0.01 * k, 10.0], 0.9, k) for k in range(n)]
    jobs = [job({(2, 4): pair(1, 0.0), (2, 2): pair(1, 0.0)}), job({(2, 2): pair(1, 0.0)}), job({(2, 4): pair(1, 0.0)}, prio=[0, 0, 0, 1])]
    res = result(rows)

    def claim(linked):
        cands = stream_candidates([0, 2], res, jobs[0])
        assert len(cands) == n and len(set(c[0] for c in cands)) == n and all(c[2] == 0 for c in cands)
        assert max(cands)[3] == n and n // WAVE != 0 // WAVE                                # tail 0, best head n: another chunk
        assert n % 2 == 1 and links_of(linked[0]) == [(500, n - 1)] and links_of(linked[1]) == [(500, n - 2)] and links_of(linked[2]) == [(500, n - 1)]
        assert linked[0]['cls'][0] == linked[0]['cls'][n] == 2 and linked[0]['n_relabelled'] == [1]    # one row each: the root's class
        assert linked[1]['n_relabelled'] == [0] and linked[2]['cls'][n] == 4 and linked[2]['category'][0] == 4
        assert greedy_equals_mutual_best([0, 2], res, jobs) == [1, 1, 1]
    return [0, 2], res, jobs, claim


def best_head_in_another_chunk(tails=64, heads=66):
    """tail i (class 2) sits on head heads - 1 - i (class 4 or 2 in turn): with the heads behind the tails in the index, the best
    head of tail 0 is index tails + heads - 1 (the third chunk of 64) and that of the last tail is in the second"""
    rows = [(0, 2, [20.0 * (heads - 1 - i) + 1.0 + 0.01 * i, 0.0, 10.0, 10.0], 0.9, i) for i in range(tails)]
    rows += [(1, 4 if h % 2 else 2, [20.0 * h, 0.0, 10.0, 10.0], 0.9, 100 + h) for h in range(heads)]
    jobs = [job({(2, 4): pair(1, 0.3), (2, 2): pair(1, 0.3)}), job({(2, 4): pair(1, 0.3)})]
    res = result(rows)

    def claim(linked):
        assert links_of(linked[0]) == [(i, 100 + heads - 1 - i) for i in range(tails)]
        assert linked[0]['pred'][tails + heads - 1] == 0 and linked[0]['pred'][heads] == tails - 1 and tails + heads > 2 * WAVE
        assert links_of(linked[1]) == [(i, 100 + heads - 1 - i) for i in range(tails) if (heads - 1 - i) % 2]
        assert linked[0]['n_relabelled'] == [tails // 2]                                     # a class-4 head behind a class-2 root
        greedy_equals_mutual_best([0, 2], res, jobs)
    return [0, 2], res, jobs, claim


def domino(n=70):
    """A chain of n pieces of two rows, classes 2, 4, 2, ...: piece k has its first box H_k at slot 2k and its last box T_k at
    slot 2k + 1, hold.  H_k = [20(k - 1), 20(k - 1) + 10]; T_k reaches c_k + 0.01 into H_(k+1) and c_k into H_(k+2), c_k = 9 - 0.05 k:
    the affinities form one strictly descending chain a(0,1) > a(0,2) > a(1,2) > a(1,3) > ..., so that every head but the first is
    offered more by the tail two pieces back than by the one before it, which prefers its own next piece - rounds of mutually best
    pairs accept exactly one pair per round, more rounds than a wavefront has lanes; the one chain has n pieces: a deep root walk
    and a vote over n pieces with as many rows in either class."""
    c = [9 - 0.05 * k for k in range(n)]
    rows = []
    for k in range(n):
        cls = 2 if k % 2 == 0 else 4
        rows.append((2 * k, cls, [20.0 * (k - 1), 0.0, 10.0, 10.0] if k else [-1000.0, 0.0, 10.0, 10.0], 0.9, k))
        x0 = 20 * k + 10 - (c[k] + 0.01)
        rows.append((2 * k + 1, cls, [x0, 0.0, 20 * (k + 1) + c[k] - x0, 10.0], 0.9, k))
    on = {(2, 4): pair(3, 0.05), (2, 2): pair(3, 0.05), (4, 4): pair(3, 0.05)}
    jobs = [job(on), job(on, prio=[0, 0, 0, 1]), job({(2, 4): pair(3, 0.05)})]
    res = result(rows)

    def claim(linked):
        cands = stream_candidates([0, 2 * n], res, jobs[0])
        assert len(cands) == 2 * n - 3
        chain = sorted(cands, key=stitch_ref.order_key)
        assert all(chain[i][0] > chain[i + 1][0] for i in range(len(chain) - 1))             # strictly descending, no ties
        assert [(i, j) for _, _, i, j in chain] == [(k // 2, k // 2 + 1 + k % 2) for k in range(2 * n - 3)]
        links, rounds = stitch_ref.match_mutual_best(cands)
        assert rounds == n - 1 and n - 1 > WAVE
        assert links == stitch_ref.match_greedy(cands) and sorted((t, h) for h, (t, _, _) in links.items()) == [(k, k + 1) for k in range(n - 1)]
        for k in (0, 1):
            assert links_of(linked[k]) == [(i, i + 1) for i in range(n - 1)] and linked[k]['n_links'] == [n - 1]
            assert set(linked[k]['root']) == {0} and set(linked[k]['object_id']) == {0}
        assert n % 2 == 0 and set(linked[0]['cls']) == {2} and set(linked[1]['cls']) == {4}   # n rows against n rows: the root's class, or prio
        assert linked[0]['n_relabelled'] == [n] and linked[1]['n_relabelled'] == [n]
        # without the pairs inside a class every tail has one candidate: one round
        assert greedy_equals_mutual_best([0, 2 * n], res, jobs) == [n - 1, n - 1, 1] and links_of(linked[2]) == links_of(linked[0])
    return [0, 2 * n], res, jobs, claim


def _chains(spec):
    """spec: per chain a list of (class, rows); chain k lies at y = 100 k, its pieces follow one another without a gap, all with
    the same box: every link has affinity 1 and gap 1, and chains never meet.  Returns the rows; piece ids are 100 k + position."""
    rows = []
    for k, pieces in enumerate(spec):
        slot = 0
        for pos, (cls, n) in enumerate(pieces):
            rows += [(slot + f, cls, [10.0, 100.0 * k, 40.0, 30.0], 0.9, 100 * k + pos) for f in range(n)]
            slot += n
    return sorted(rows, key=lambda r: r[0])


ALL_124 = {(1, 2): pair(1, 0.9), (2, 4): pair(1, 0.9), (1, 4): pair(1, 0.9), (1, 1): pair(1, 0.9), (2, 2): pair(1, 0.9), (4, 4): pair(1, 0.9)}


def vote_edges():
    """Eight chains in one stream, one per way the vote tuple (rows, prio, is the root's class, -class) can decide:
      0  [2 x2, 4 x2]            rows tie, prio ties: the root's class 2          (prio for 4: 4)
      1  [4 x2, 2 x2]            the same with root 4: 4                          (prio for 2 in job 2: 2)
      2  [1 x1, 2 x2, 4 x2]      2 and 4 tie in rows and prio, neither is the root's: the lower class 2
      3  [2 x2, 1 x2, 4 x2]      three classes tie: the root's class 2; prio for 4 -> 4; prio for 1 -> 1
      4  [2 x1, 4 x3]            the winner is not the root's class: 4, whatever the prio of 2 is
      5  [4 x1, 2 x1, 4 x1]      two pieces against one: 4
      6  [1 x3]                  a chain of one piece keeps its class
      7  [2 x1, 4 x1, 1 x1, 2 x1]   2 has more rows than 4 and 1 together: 2 even when prio favours 4"""
    spec = [[(2, 2), (4, 2)], [(4, 2), (2, 2)], [(1, 1), (2, 2), (4, 2)], [(2, 2), (1, 2), (4, 2)], [(2, 1), (4, 3)], [(4, 1), (2, 1), (4, 1)],
            [(1, 3)], [(2, 1), (4, 1), (1, 1), (2, 1)]]
    rows = _chains(spec)
    jobs = [job(ALL_124), job(ALL_124, prio=[0, 0, 0, 1]), job(ALL_124, prio=[0, 5, 0, 0]), job(ALL_124, prio=[7, 0, 0, 0])]
    res = result(rows)
    want = [[2, 4, 2, 2, 4, 4, 1, 2], [4, 4, 4, 4, 4, 4, 1, 2], [2, 2, 2, 2, 4, 4, 1, 2], [2, 4, 2, 1, 4, 4, 1, 2]]

    def claim(linked):
        slots = max(r[0] for r in rows) + 1
        for got, classes in zip(linked, want):
            assert got['n_links'] == [sum(len(p) - 1 for p in spec)]
            by_id = dict(zip(got['object_id'], got['category']))
            assert [by_id[100 * k] for k in range(len(spec))] == classes
            assert sorted(set(got['object_id'])) == [100 * k for k in range(len(spec))]
            assert len(set(zip(got['object_id'], got['category']))) == len(spec)             # one category per id
            assert got['n_relabelled'] == [sum(n for pieces, c in zip(spec, classes) for cls, n in pieces if cls != c)]
        assert all(a == 1.0 for got in linked for a in got['affinity'] if a >= 0)
        greedy_equals_mutual_best([0, slots], res, jobs)
    return [0, max(r[0] for r in rows) + 1], res, jobs, claim


def sixteen_classes():
    """n_classes = 16: chains of the classes 16 and 1 / 15 / 16 - the winner is class 16, by rows, by prio, and as the root's"""
    spec = [[(1, 1), (16, 2)], [(15, 2), (16, 2)], [(16, 1), (15, 1)], [(15, 1), (16, 1)], [(3, 2), (16, 1)]]
    rows = _chains(spec)
    on = {(1, 16): pair(1, 0.9), (15, 16): pair(1, 0.9), (3, 16): pair(1, 0.9)}
    jobs = [job(on), job(on, prio=[0] * 15 + [1]), job({(15, 16): pair(1, 0.9)}, prio=[0] * 15 + [1])]
    res = result(rows)

    def claim(linked):
        ids = lambda got: dict(zip(got['object_id'], got['category']))
        assert [ids(linked[0])[100 * k] for k in range(5)] == [16, 15, 16, 15, 3]
        assert [ids(linked[1])[100 * k] for k in range(5)] == [16, 16, 16, 16, 3]
        assert linked[2]['n_links'] == [3] and sorted(set(linked[2]['object_id'])) == [0, 1, 100, 200, 300, 400, 401]
        greedy_equals_mutual_best([0, 4], res, jobs, 16)
    return [0, 4], res, jobs, claim


def equal_affinities():
    """One and the same box everywhere: every affinity is 1, the answer rests on (n, i, j) across classes.
    Left (x = 0): tail 0 (class 2, slot 0), heads 1 (class 4) and 2 (class 2) at slot 1: equal a and n, the lower head index - the
    class-4 head - wins; head 2 stays a root.
    Right (x = 100): tail 3 (class 4, slot 0), head 4 (class 4) at slot 2 and head 5 (class 2) at slot 1... numbered by first
    appearance the class-2 head comes first: the smaller gap wins, whatever the class.
    Far (x = 200): tails 6 (class 2) and 7 (class 4) at slot 3, one head 8 (class 4) at slot 4: the lower tail index wins."""
    box = lambda x: [x, 0.0, 10.0, 10.0]
    rows = [(0, 2, box(0.0), 0.9, 10), (1, 4, box(0.0), 0.9, 11), (1, 2, box(0.0), 0.9, 12),
            (0, 4, box(100.0), 0.9, 20), (2, 4, box(100.0), 0.9, 21), (1, 2, box(100.0), 0.9, 22),
            (3, 2, box(200.0), 0.9, 30), (3, 4, box(200.0), 0.9, 31), (4, 4, box(200.0), 0.9, 32)]
    rows.sort(key=lambda r: r[0])
    on = {(2, 4): pair(2, 0.5), (2, 2): pair(2, 0.5), (4, 4): pair(2, 0.5)}
    jobs = [job(on), job({(2, 2): pair(2, 0.5), (4, 4): pair(2, 0.5)})]
    res = result(rows)

    def claim(linked):
        cands = stream_candidates([0, 5], res, jobs[0])
        assert cands and all(c[0] == 1.0 for c in cands)
        assert links_of(linked[0]) == [(10, 11), (20, 22), (22, 21), (30, 32)]
        for other in (lambda c: (-c[0], -c[1], c[2], c[3]), lambda c: (-c[0], c[1], -c[2], c[3]), lambda c: (-c[0], c[1], c[2], -c[3])):
            assert links_of(xlink_ref.xlink([0, 5], res, jobs[0], key=other)) != links_of(linked[0])
        assert links_of(linked[1]) == [(10, 12), (20, 21), (31, 32)]                         # inside the classes only: the other head, gap, tail
        greedy_equals_mutual_best([0, 5], res, jobs)
    return [0, 5], res, jobs, claim


def threshold_edges():
    """The same tail and head boxes three times over, 10 slots apart in time so that the affinity is the same double: class
    2 -> 4, class 2 -> 2, class 4 -> 4.  link_iou equal to the affinity links, one ulp above does not, per pair; a == 0 does not
    link under threshold 0 or -1 (ids 31, 32: boxes that do not meet)."""
    t, h = [10.3, 20.7, 33.1, 41.9], [13.9, 18.2, 30.7, 44.3]
    a = stitch_ref.affinity([(1, t)], [(4, h)], 'hold')
    rows = []
    for k, (ct, ch) in enumerate(((2, 4), (2, 2), (4, 4))):
        rows += [(10 * k + 1, ct, t, 0.9, 10 * k + 1), (10 * k + 4, ch, h, 0.9, 10 * k + 2)]
    rows += [(1, 2, [5000.0, 0.0, 10.0, 10.0], 0.9, 31), (2, 4, [9000.0, 0.0, 10.0, 10.0], 0.9, 32)]
    rows.sort(key=lambda r: r[0])
    up, down = math.nextafter(a, 2.0), math.nextafter(a, 0.0)
    jobs = [job({(2, 4): pair(3, a), (2, 2): pair(3, up), (4, 4): pair(3, down)}),
            job({(2, 4): pair(3, up), (2, 2): pair(3, a), (4, 4): pair(3, up)}),
            job({(2, 4): pair(3, 0.0), (2, 2): pair(3, 0.0), (4, 4): pair(3, 0.0)}),
            job({(2, 4): pair(3, -1.0)})]
    res = result(rows)

    def claim(linked):
        assert 0.5 < a < 0.9 and a != round(a, 6)
        assert links_of(linked[0]) == [(1, 2), (21, 22)] and links_of(linked[1]) == [(11, 12)]
        assert [lk[3] for lk in linked[0]['links']] == [a, a] and linked[0]['links'][0][2] == 3
        assert links_of(linked[2]) == [(1, 2), (11, 12), (21, 22)]                           # threshold 0: none of the a == 0 pairs
        assert links_of(linked[3]) == [(1, 2)] and linked[3]['n_relabelled'] == [1]
        zero = [c for c in xlink_ref.candidates(stitch_ref.trajectories([0, 26], res)[0], dict(jobs[3], pairs={}), N_CLASSES)]
        assert zero == [] and stitch_ref.iou_dd([5000.0, 0.0, 5010.0, 10.0], [9000.0, 0.0, 9010.0, 10.0]) == 0.0
        greedy_equals_mutual_best([0, 26], res, jobs)
    return [0, 26], res, jobs, claim


def gaps_per_pair():
    """Class 2's row of the table has different gaps: (2, 2) links over 1 slot, (2, 4) over 3.  Four tails of class 2 at slot 0,
    100 px apart, each with one head on it: class 4 at n = 3 (links), class 4 at n = 4 (one over), class 2 at n = 1 (links),
    class 2 at n = 2 (one over, though inside the range the tail scans)."""
    box = lambda k: [100.0 * k, 0.0, 40.0, 30.0]
    rows = [(0, 2, box(k), 0.9, k) for k in range(4)]
    rows += [(3, 4, box(0), 0.9, 10), (4, 4, box(1), 0.9, 11), (1, 2, box(2), 0.9, 12), (2, 2, box(3), 0.9, 13)]
    rows.sort(key=lambda r: r[0])
    jobs = [job({(2, 4): pair(3, 0.5), (2, 2): pair(1, 0.5)}), job({(2, 4): pair(4, 0.5), (2, 2): pair(2, 0.5)}), job({(2, 4): pair(1, 0.5), (2, 2): pair(3, 0.5)})]
    res = result(rows)

    def claim(linked):
        assert links_of(linked[0]) == [(0, 10), (2, 12)]
        assert links_of(linked[1]) == [(0, 10), (1, 11), (2, 12), (3, 13)]
        assert links_of(linked[2]) == [(2, 12), (3, 13)]
        assert [lk[2] for lk in linked[1]['links']] == [1, 2, 3, 4]                        # ascending head index: heads by first slot
        greedy_equals_mutual_best([0, 5], res, jobs)
    return [0, 5], res, jobs, claim


def off_pairs():
    """a pair that is off, and a same-class candidate when (a, a) is not listed: neither links; the listed pair does"""
    box = [100.0, 50.0, 40.0, 30.0]
    rows = [(0, 1, box, 0.9, 1), (1, 2, box, 0.9, 2), (2, 2, box, 0.9, 3), (3, 4, box, 0.9, 4), (4, 4, box, 0.9, 5)]
    jobs = [job({(2, 4): pair(1, 0.9)}), job({}), job({(1, 2): pair(1, 0.9), (2, 4): pair(0, 0.0)})]
    res = result(rows)

    def claim(linked):
        assert links_of(linked[0]) == [(3, 4)] and linked[0]['object_id'] == [1, 2, 3, 3, 5] and linked[0]['category'] == [1, 2, 2, 2, 4]
        assert linked[1]['n_links'] == [0] and linked[1]['category'] == res['category'] and linked[1]['n_relabelled'] == [0]
        assert links_of(linked[2]) == [(1, 2)] and linked[2]['category'] == [1, 1, 2, 4, 4]
    return [0, 5], res, jobs, claim


def isolation():
    """perfectly overlapping pieces of different streams (slot 2 ends stream 0, slot 3 starts stream 1) never link; the same pair
    inside a stream does"""
    box = [100.0, 50.0, 40.0, 30.0]
    rows = [(1, 2, box, 0.9, 1), (2, 4, box, 0.9, 2), (3, 2, box, 0.9, 3), (4, 4, box, 0.9, 4), (5, 2, box, 0.9, 5)]
    jobs = [job({(2, 4): pair(2, 0.9)}), job({(2, 4): pair(2, 0.9), (2, 2): pair(2, 0.9)})]

    def claim(linked):
        assert links_of(linked[0]) == [(1, 2), (3, 4), (4, 5)] and linked[0]['n_links'] == [1, 2]
        assert linked[0]['object_id'] == [1, 1, 3, 3, 3] and linked[0]['category'] == [2, 2, 2, 2, 2] and linked[0]['n_relabelled'] == [1, 1]
        assert links_of(linked[1]) == [(1, 2), (3, 4), (4, 5)]                               # (2, 3) and (3, 5) never: another stream, a head taken
    return [0, 3, 6], result(rows), jobs, claim


def flicker_chain():
    """The issue's picture: cyclist rows in slots 0-2, pedestrian rows in slots 3-4, cyclist rows in slots 5-7, (2, 4) on at gap 1:
    one id, class 4, two rows relabelled, two links"""
    rows = [(f, 4, [10.0 + f, 20.0, 30.0, 40.0], 0.9, 7) for f in range(3)] + [(f, 2, [10.0 + f, 20.0, 30.0, 40.0], 0.9, 8) for f in (3, 4)]
    rows += [(f, 4, [10.0 + f, 20.0, 30.0, 40.0], 0.9, 9) for f in range(5, 8)]
    jobs = [job({(2, 4): pair(1, 0.3)}), job({(2, 4): pair(1, 0.3)}, motion='linear')]

    def claim(linked):
        for got in linked:
            assert set(got['object_id']) == {7} and set(got['category']) == {4} and got['n_relabelled'] == [2] and got['n_links'] == [2]
            assert got['pred'] == [-1, 0, 1] and got['root'] == [0, 0, 0] and got['cls'] == [4, 4, 4]
        assert linked[1]['affinity'][1:] == [1.0, 1.0] and linked[0]['affinity'][1] < 1.0
    return [0, 8], result(rows), jobs, claim


def empty_result():
    def claim(linked):
        assert linked[0]['object_id'] == [] and linked[0]['n_links'] == [0, 0] and linked[0]['pred'] == [] and linked[0]['n_relabelled'] == [0, 0]
    return [0, 2, 4], result([]), [job({(2, 4): pair(3, 0.1)})], claim


def many_trajectories(n):
    """n single-row trajectories in one stream at slots i % 8, groups of 8 forming chains along x whose classes alternate 2, 4:
    sizes on either side of the LDS limit of the match tables; local indices run slot-major, so a chain's links cross the whole
    index range.  A whole group votes 4 rows against 4: the root's class 2."""
    groups = (n + 7) // 8
    rows = [(i % 8, 2 if i % 2 == 0 else 4, [40.0 * (i // 8) + 3.7 * (i % 8), 0.5 * (i % 8), 30.0, 20.0], 0.9, i) for i in range(n)]
    rows.sort(key=lambda r: r[0])
    jobs = [job({(2, 4): pair(1, 0.5)}), job({(2, 4): pair(2, 0.5), (2, 2): pair(2, 0.5), (4, 4): pair(2, 0.5)}, prio=[0, 0, 0, 1], motion='linear')]

    def claim(linked):
        s = linked[0]
        assert len(s['pred']) == n and s['n_links'] == [n - groups]
        assert sorted(set(s['object_id'])) == list(range(0, n, 8)) and sorted(set(s['root'])) == list(range(groups))
        assert set(s['category']) == {2} and s['n_relabelled'] == [n // 2]
        assert linked[1]['n_links'] == [n - groups] and linked[1]['n_relabelled'][0] >= (n // 8) * 4
    return [0, 8], result(rows), jobs, claim


CASES = {
    'one_tail_65_heads': one_tail_many_heads,
    'best_head_in_another_chunk': best_head_in_another_chunk,
    'domino_70': domino,
    'vote_edges': vote_edges,
    'equal_affinities': equal_affinities,
    'threshold_edges': threshold_edges,
    'gaps_per_pair': gaps_per_pair,
    'off_pairs': off_pairs,
    'isolation': isolation,
    'flicker_chain': flicker_chain,
    'empty_result': empty_result,
    'many_trajectories_200': lambda: many_trajectories(200),
}


# ---- the tracked fixtures with injected flicker ----

def inject_flicker(out):
    """Class flicker as a tracker under max_age 1 leaves it: in every third trajectory of at least six rows, the middle third of its
    rows moves to a fresh id and the other class of {2, 4} (class 2 otherwise), and the last third to a second fresh id in the
    trajectory's own class - one object, three trajectories.  (Moving the middle third alone leaves the first and last third one
    trajectory that never ended, which is the case DESIGN.md section 31 lists as not built.)  Returns a result of the same form."""
    frame, cat, oid = np.asarray(out['frame']), np.asarray(out['category']).copy(), np.asarray(out['object_id']).copy()
    fresh = int(oid.max()) + 1 if oid.size else 1
    long_ones = [i for i in dict.fromkeys(oid.tolist()) if int((oid == i).sum()) >= 6]
    for i in long_ones[::3]:
        rows = np.nonzero(oid == i)[0]
        rows = rows[np.argsort(frame[rows], kind='stable')]
        n = rows.size
        mid, last = rows[n // 3:2 * n // 3], rows[2 * n // 3:]
        cls = int(cat[rows[0]])
        cat[mid] = {2: 4, 4: 2}.get(cls, 2)
        oid[mid] = fresh
        oid[last] = fresh + 1
        fresh += 2
    return dict(out, category=cat, object_id=oid)


# four jobs from loosest to strictest
FLICKER_JOBS = [
    job({(2, 4): pair(3, 0.05), (1, 2): pair(3, 0.05), (1, 1): pair(3, 0.05), (2, 2): pair(3, 0.05), (4, 4): pair(3, 0.05)}, motion='linear'),
    job({(2, 4): pair(2, 0.3), (1, 2): pair(2, 0.3)}, prio=[0, 0, 0, 1]),
    job({(2, 4): pair(1, 0.5)}),
    job({(2, 4): pair(1, 1.5), (1, 2): pair(1, 1.5)}),
]


def most_slots(packed, out):
    """the most distinct slots the rows of `out` fill in one stream: no chain there has more pieces"""
    offsets = np.asarray(packed['stream_frame_offsets'])
    frames = np.unique(np.asarray(out['frame']))
    return int(np.bincount(np.searchsorted(offsets, frames, side='right') - 1).max()) if frames.size else 0


def flicker_condition(refs, pieces=3):
    """what makes the fixture a test: under the loosest job the reference forms a chain of at least three pieces and relabels a
    row; under the strictest it links nothing.  `pieces`: min(3, most_slots()) - the g5 fixture has six detections in streams of at
    most two slots, so whatever is injected its longest chain has two pieces."""
    roots = refs[0]['root']
    offsets = refs[0]['traj_offsets']
    sizes = {}
    for s in range(len(offsets) - 1):
        for t in range(offsets[s], offsets[s + 1]):
            sizes[(s, roots[t])] = sizes.get((s, roots[t]), 0) + 1
    assert max(sizes.values()) >= pieces, 'no chain of %d pieces' % pieces
    assert sum(refs[0]['n_relabelled']) >= 1, 'no row relabelled'
    assert sum(refs[-1]['n_links']) == 0 and sum(refs[-1]['n_relabelled']) == 0, 'the strictest job links'
    made = [sum(r['n_links']) for r in refs]
    assert made == sorted(made, reverse=True), made
