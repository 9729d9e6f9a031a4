"""Adversarial inputs for the two track layout steps.

LAYOUT_CASES - for wt_tracks_layout_*: name -> () -> (stream_frame_offsets, [result, ...], claim); a `result` has the columns
utils.track_packed returns, rows ascending by frame slot, and claim(p) - given _trackset.prepare() of the results - asserts that
the case is in the class its name says.
EVAL_CASES - for wt_tracks_to_eval_*: name -> () -> (stream_frame_offsets, [result, ...], gt_json, claim); claim(aligned) is given
evaluate._align() of every result against the ground truth, [(order, frame_hyp_offsets, h_id), ...].
REFUSALS - inputs the layout must refuse: name -> () -> (stream_frame_offsets, [result, ...], [row count per result], status name).
tests/test_layout_cases.py runs the claims on the host code alone; tests/test_gpu_tracks_layout.py compares the kernels with it."""
import itertools
import random

from track_cases import N_CLASSES, result


def box(i, slot):
    """a box of object i at a slot: fractional, different in every coordinate"""
    return [10.0 + 7.3 * (i % 97) + 1.7 * slot, 20.0 + 3.1 * (i % 89) - 0.9 * slot, 30.0 + 0.37 * (i % 11) + 0.2 * slot, 40.0 + 0.53 * (i % 7)]


def rows_of(pairs):
    """(slot, object id) pairs -> rows: category 1 + position % 4 except 3, distinct boxes and scores"""
    return [(s, (1, 2, 4)[k % 3], box(k, s), 0.25 + 0.001 * k, oid) for k, (s, oid) in enumerate(pairs)]


def first_appearance(offsets, res):
    """Restatement: per row its trajectory numbered per stream by first appearance in row order, and the count per stream."""
    seen = [dict() for _ in offsets[1:]]
    local = []
    for f, oid in zip(res['frame'], res['object_id']):
        s = max(i for i, lo in enumerate(offsets[:-1]) if lo <= f and f < offsets[i + 1])
        local.append(seen[s].setdefault(oid, len(seen[s])))
    return local, [len(d) for d in seen]


def locals_of(p, r):
    lo, hi = int(p['set_row_offsets'][r]), int(p['set_row_offsets'][r + 1])
    return p['local'][lo:hi].tolist()


# ---- wt_tracks_layout_* ----

def empty_result():
    def claim(p):
        assert p['n_rows'] == 0 and p['n_traj_total'] == 0 and p['max_traj'] == 0 and p['frame_row_offsets'].tolist() == [[0, 0, 0, 0]]
    return [0, 3], [result([])], claim


def empty_in_the_middle():
    a = rows_of([(0, 5), (1, 5), (1, 6)])
    c = rows_of([(2, 6)])

    def claim(p):
        assert p['set_row_offsets'].tolist() == [0, 3, 3, 4] and p['n_traj'].tolist() == [[2], [0], [1]]
        assert p['frame_row_offsets'][1].tolist() == [0, 0, 0, 0]
    return [0, 3], [result(a), result([]), result(c)], claim


def streams_without_rows():
    """five streams; the first, the middle and the last one have no rows"""
    rows = rows_of([(2, 8), (2, 9), (3, 8), (6, 9), (7, 4), (7, 9)])

    def claim(p):
        assert p['n_traj'].tolist() == [[0, 2, 0, 2, 0]] and locals_of(p, 0) == [0, 1, 0, 0, 1, 0]
    return [0, 2, 4, 6, 8, 10], [result(rows)], claim


def one_row():
    def claim(p):
        assert p['n_rows'] == 1 and p['n_traj'].tolist() == [[0, 1]] and locals_of(p, 0) == [0]
    return [0, 2, 4], [result(rows_of([(3, 12)]))], claim


def ids_not_in_birth_order():
    """first appearance descends in id: numbering by value would reverse the indices"""
    rows = rows_of([(0, 90), (0, 70), (1, 30), (1, 90), (2, 10), (2, 30), (2, 70)])

    def claim(p):
        assert locals_of(p, 0) == [0, 1, 2, 0, 3, 2, 1]
        by_value = sorted(set(r[4] for r in rows))
        assert [by_value.index(r[4]) for r in rows] != locals_of(p, 0)
    return [0, 3], [result(rows)], claim


def same_id_elsewhere():
    """id 7 in both streams and in both results: four different trajectories; the second result meets it second"""
    a = rows_of([(0, 7), (1, 7), (2, 7), (3, 8), (3, 7)])
    b = rows_of([(0, 3), (0, 7), (2, 7)])

    def claim(p):
        assert p['n_traj'].tolist() == [[1, 2], [2, 1]] and locals_of(p, 0) == [0, 0, 0, 1, 0] and locals_of(p, 1) == [0, 1, 0]
        assert p['traj_offsets'].tolist() == [0, 1, 3, 5, 6]
    return [0, 2, 4], [result(a), result(b)], claim


def wide_ids():
    """negative ids, and ids that differ only above bit 32"""
    ids = [-1, 5, -(1 << 40), 5 + (1 << 32), 5 + (1 << 33), -1 - (1 << 32), (1 << 62), -(1 << 63)]
    rows = rows_of([(0, i) for i in ids] + [(1, i) for i in reversed(ids)])

    def claim(p):
        n = len(ids)
        assert p['n_traj'].tolist() == [[n]] and locals_of(p, 0) == list(range(n)) + list(reversed(range(n)))
        assert len(set(i & 0xffffffff for i in ids)) < n                          # the low words alone do not tell them apart
    return [0, 2], [result(rows)], claim


def colliding_ids(probe, capacity):
    """three ids whose first probe is the same slot of a table of `capacity` slots - and one id that probes the slot behind it -
    in every order of first appearance: one result per order.  probe(id, capacity) is the library's wt_tracks_layout_probe."""
    by_slot = {}
    trio = None
    for i in range(1, 1 << 20):
        group = by_slot.setdefault(probe(i, capacity), [])
        group.append(i)
        if len(group) == 3:
            trio = group
            break
    behind = next(i for i in range(1, 1 << 20) if probe(i, capacity) == (probe(trio[0], capacity) + 1) % capacity)
    results = []
    for order in itertools.permutations(trio + [behind]):
        results.append(result(rows_of([(0, i) for i in order] + [(1, i) for i in trio + [behind]])))

    def claim(p):
        assert len(set(probe(i, capacity) for i in trio)) == 1 and len(set(trio)) == 3
        assert p['R'] == 24 and p['n_traj'].tolist() == [[4]] * 24
        seen = set()
        for r, order in enumerate(itertools.permutations(trio + [behind])):
            want = [order.index(i) for i in trio + [behind]]
            assert locals_of(p, r) == [0, 1, 2, 3] + want
            seen.add(tuple(want))
        assert len(seen) == 24
    return [0, 2], results, claim


def many_rows(n, repeats=16):
    """one stream with n rows: n - repeats trajectories with pseudo-random 64-bit ids in slot 0, `repeats` of them again in slot 1"""
    rng = random.Random(n)
    ids = []
    taken = set()
    while len(ids) < n - repeats:
        i = rng.getrandbits(64) - (1 << 63)
        if i not in taken:
            taken.add(i)
            ids.append(i)
    again = rng.sample(range(len(ids)), repeats)
    rows = rows_of([(0, i) for i in ids] + [(1, ids[k]) for k in again])

    def claim(p):
        assert p['n_rows'] == n and p['n_traj'].tolist() == [[n - repeats]] and locals_of(p, 0) == list(range(n - repeats)) + again
    return [0, 2], [result(rows)], claim


def scan_seam(n):
    """one stream with n rows, first and later rows of a trajectory mixed: the running count must cross the seams of the scan"""
    a = (n + 1) // 2
    pairs = [(0, 1000 - i) for i in range(a)]
    for k in range(n - a):
        pairs.append((1, 1000 - (k * 7) % a) if k % 2 == 0 else (1, 5000 + k))
    seen, pairs1 = set(), []
    for s, oid in pairs[a:]:                                  # a trajectory is in a slot once
        pairs1.append((s, oid if oid not in seen else 9000 + len(pairs1)))
        seen.add(pairs1[-1][1])
    rows = rows_of(pairs[:a] + pairs1)

    def claim(p):
        res = result(rows)
        local, counts = first_appearance([0, 2], res)
        assert p['n_rows'] == n and locals_of(p, 0) == local and p['n_traj'].tolist() == [counts]
        assert any(v < a for v in local[a:]) and any(v >= a for v in local[a:])          # slot 1 mixes known and new trajectories
    return [0, 2], [result(rows)], claim


def second_row_is_last():
    """a trajectory whose second row is its stream's last row; the next stream begins with the other id"""
    rows = rows_of([(0, 5), (0, 6), (1, 5), (2, 6), (3, 5)])

    def claim(p):
        assert p['frame_row_offsets'].tolist() == [[0, 2, 3, 4, 5]] and locals_of(p, 0) == [0, 1, 0, 0, 1] and p['n_traj'].tolist() == [[2, 2]]
    return [0, 2, 4], [result(rows)], claim


LAYOUT_CASES = {'empty_result': empty_result, 'empty_in_the_middle': empty_in_the_middle, 'streams_without_rows': streams_without_rows,
                'one_row': one_row, 'ids_not_in_birth_order': ids_not_in_birth_order, 'same_id_elsewhere': same_id_elsewhere, 'wide_ids': wide_ids,
                'second_row_is_last': second_row_is_last}
SEAMS = (63, 64, 65)                                          # and one row more than a workgroup scans per step (wt_tracks_layout_limits)


# ---- wt_tracks_to_eval_* ----

def image_id(stream, slot):
    """the image of a slot counted inside its stream, as track_stage_support.packed_for names it"""
    return 'seg%d/%d/FRONT' % (stream, slot * 10 + 5)


def ground_truth(frames):
    """a ground truth with exactly the images (stream, slot inside the stream) of `frames`, streams numbered in the order given,
    one annotation per image"""
    return {'images': [{'id': image_id(s, f)} for s, f in frames],
            'annotations': [{'image_id': image_id(s, f), 'bbox': box(3, f), 'category_id': 1, 'object_id': 'g%d' % s} for s, f in frames]}


def part(aligned, k):
    order, offsets, _ = aligned[k]
    n_on = int(offsets[-1])
    return order[:n_on].tolist(), order[n_on:].tolist()


def unknown_slots():
    """the ground truth lacks the first, a middle and the last slot of the stream"""
    rows = rows_of([(0, 1), (0, 2), (1, 1), (2, 2), (3, 1), (3, 2), (4, 1), (5, 2), (5, 1)])

    def claim(aligned):
        on, off = part(aligned, 0)
        assert on == [2, 3, 6] and off == [0, 1, 4, 5, 7, 8] and aligned[0][1].tolist() == [0, 1, 2, 3]
    return [0, 6], [result(rows)], ground_truth([(0, 1), (0, 2), (0, 4)]), claim


def unknown_stream():
    """the ground truth has the second stream only"""
    rows = rows_of([(0, 1), (1, 1), (2, 1), (2, 3), (3, 3)])

    def claim(aligned):
        on, off = part(aligned, 0)
        assert on == [2, 3, 4] and off == [0, 1] and aligned[0][1].tolist() == [0, 2, 3]
    return [0, 2, 4], [result(rows)], ground_truth([(1, 0), (1, 1)]), claim


def foreign_categories():
    """rows of category 0 and N_CLASSES + 1 inside known slots, between rows that count"""
    rows = rows_of([(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3)])
    rows[1] = rows[1][:1] + (0,) + rows[1][2:]
    rows[3] = rows[3][:1] + (N_CLASSES + 1,) + rows[3][2:]

    def claim(aligned):
        on, off = part(aligned, 0)
        assert on == [0, 2, 4, 5] and off == [1, 3] and aligned[0][1].tolist() == [0, 2, 4]
    return [0, 2], [result(rows)], ground_truth([(0, 0), (0, 1)]), claim


def streams_in_another_order():
    """the ground truth numbers the streams the other way round: the rows on its frames move"""
    rows = rows_of([(0, 1), (1, 1), (1, 2), (2, 4), (3, 4), (3, 1)])

    def claim(aligned):
        on, off = part(aligned, 0)
        assert on == [3, 4, 5, 0, 1, 2] and off == [] and aligned[0][1].tolist() == [0, 1, 3, 4, 6]
    return [0, 2, 4], [result(rows)], ground_truth([(1, 0), (1, 1), (0, 0), (0, 1)]), claim


def only_ignored_rows():
    """three results: one on unknown slots only, one without rows, one that takes part"""
    a = rows_of([(0, 1), (2, 1), (2, 2)])
    c = rows_of([(0, 1), (1, 1), (1, 2)])

    def claim(aligned):
        assert part(aligned, 0) == ([], [0, 1, 2]) and part(aligned, 1) == ([], []) and part(aligned, 2) == ([1, 2], [0])
    return [0, 3], [result(a), result([]), result(c)], ground_truth([(0, 1)]), claim


EVAL_CASES = {'unknown_slots': unknown_slots, 'unknown_stream': unknown_stream, 'foreign_categories': foreign_categories,
              'streams_in_another_order': streams_in_another_order, 'only_ignored_rows': only_ignored_rows}


# ---- refusals ----

def descending_slots():
    return [0, 3], [result(rows_of([(0, 1), (2, 1), (1, 1)]))], [3], 'WT_ERR_INVALID'


def slot_beyond_the_set():
    return [0, 3], [result(rows_of([(0, 1), (3, 1)]))], [2], 'WT_ERR_INVALID'


def negative_row_count():
    """the second of three results carries the tracker's error status 5 in place of its row count"""
    one = result(rows_of([(0, 1), (1, 1)]))
    return [0, 3], [one, one, one], [2, -5, 2], 'WT_ERR_NUMERIC'


REFUSALS = {'descending_slots': descending_slots, 'slot_beyond_the_set': slot_beyond_the_set, 'negative_row_count': negative_row_count}
