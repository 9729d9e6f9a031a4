"""The plain-Python restatement of the tracking metric (tests/mot_ref.py) against answers worked out by hand.

tests/test_gpu_mot.py compares the HIP evaluator with mot_ref; this file is what pins mot_ref itself to the definition in
DESIGN.md ("Tracking metric").  No GPU."""
import math

import numpy as np

import mot_ref

SEG = 'segment-a_with_camera_labels'


def image_id(frame, camera='FRONT', segment=SEG):
    return '%s/%d/%s' % (segment, frame, camera)


def ann(frame, bbox, oid, cat=1, level=1, **kw):
    a = {'image_id': image_id(frame, **kw), 'bbox': list(bbox), 'category_id': cat, 'object_id': oid}
    if level is not None:
        a['tracking_difficulty_level'] = level
    return a


def res(frame, bbox, oid, cat=1, **kw):
    return {'image_id': image_id(frame, **kw), 'bbox': list(bbox), 'score': 0.9, 'category_id': cat, 'object_id': str(oid)}


def counts(row):
    return tuple(row[f] for f in mot_ref.FIELDS)


A0, B0 = [0, 0, 10, 10], [100, 0, 10, 10]


def test_iou_is_the_sort_formula():
    assert mot_ref.iou([0., 0., 10., 10.], [0., 0., 10., 7.5]) == 0.75
    assert mot_ref.iou([0., 0., 10., 10.], [20., 0., 30., 10.]) == 0.0
    assert mot_ref.iou([0., 0., 10., 10.], [10., 0., 20., 10.]) == 0.0          # touching boxes


def test_perfect_tracks_mota_1_and_motp_is_the_known_iou():
    gt = [ann(f, A0, 'A') for f in range(3)] + [ann(f, B0, 'B') for f in range(3)]
    # every hypothesis covers the upper three quarters of its object: IoU = 75 / 100 exactly, above the vehicle threshold 0.7
    hyp = [res(f, [0, 0, 10, 7.5], 1) for f in range(3)] + [res(f, [100, 0, 10, 7.5], 2) for f in range(3)]
    r = mot_ref.evaluate(gt, hyp)
    for lv in (1, 2):
        row = r['table'][1][lv]
        assert counts(row) == (6, 6, 0, 0, 0)
        assert row['MOTA'] == 1.0 and row['MOTP'] == 0.75
        assert r['table']['ALL'][lv] == row
    assert r['hyp_match'] == [0, 1, 2, 3, 4, 5] and r['hyp_switch'] == [0] * 6 and r['ignored_rows'] == 0
    # the same boxes as pedestrians' (threshold 0.5) and below the vehicle threshold: nothing matches
    low = [res(f, [0, 0, 10, 6], 1) for f in range(3)]                         # IoU 0.6 < 0.7
    r = mot_ref.evaluate([ann(f, A0, 'A') for f in range(3)], low)
    assert counts(r['table'][1][2]) == (3, 0, 3, 3, 0) and r['table'][1][2]['MOTA'] == -1.0
    assert math.isnan(r['table'][1][2]['MOTP'])


def test_two_tracks_that_exchange_ids_once_are_two_switches():
    gt = [ann(f, A0, 'A') for f in range(4)] + [ann(f, B0, 'B') for f in range(4)]
    hyp = []
    for f in range(4):
        a, b = (1, 2) if f < 2 else (2, 1)
        hyp += [res(f, A0, a), res(f, B0, b)]
    r = mot_ref.evaluate(gt, hyp)
    row = r['table']['ALL'][2]
    assert counts(row) == (8, 8, 0, 0, 2)
    assert row['MOTA'] == 0.75 and row['MOTP'] == 1.0
    assert r['hyp_switch'] == [0, 0, 0, 0, 1, 1, 0, 0]


def test_carry_over_keeps_the_old_pairs_where_hungarian_alone_would_swap():
    # pedestrians (threshold 0.5).  Frame 1: the objects have come close; each old hypothesis still overlaps its object by
    # 7.5 of 10 columns (IoU 75 / 125 = 0.6) but overlaps the OTHER object by 9.5 columns (IoU 95 / 105)
    a1, b1 = [50, 0, 10, 10], [52, 0, 10, 10]
    h1, h2 = [52.5, 0, 10, 10], [49.5, 0, 10, 10]
    gt = [ann(0, A0, 'A', 2), ann(0, B0, 'B', 2), ann(1, a1, 'A', 2), ann(1, b1, 'B', 2)]
    hyp = [res(0, A0, 1, 2), res(0, B0, 2, 2), res(1, h1, 1, 2), res(1, h2, 2, 2)]
    G = mot_ref.gated_matrix([mot_ref.xyxy(a1), mot_ref.xyxy(b1)], [mot_ref.xyxy(h1), mot_ref.xyxy(h2)], 0.5)
    assert (G > 0).all() and mot_ref.assign(G) == [(0, 1), (1, 0)]              # Hungarian alone swaps them
    r = mot_ref.evaluate(gt, hyp)
    row = r['table'][2][2]
    assert counts(row) == (4, 4, 0, 0, 0)
    assert row['iou_sum'] == 1.0 + 1.0 + 0.6 + 0.6
    assert r['hyp_match'] == [0, 1, 2, 3]
    # an old pair that falls below the threshold is not carried: h1 moved on to 54..64 overlaps A (50..60) by 6 columns,
    # IoU 60 / 140 < 0.5; B keeps h2 (carried), so A is missed and h1 is a false positive - no switch
    r = mot_ref.evaluate(gt, hyp[:2] + [res(1, [54, 0, 10, 10], 1, 2), res(1, h2, 2, 2)])
    assert r['hyp_match'] == [0, 1, -1, 3] and counts(r['table'][2][2]) == (4, 3, 1, 1, 0)
    # with both old pairs below the threshold Hungarian decides alone: objects apart, each hypothesis on the other's box
    gt2 = gt[:2] + [ann(1, a1, 'A', 2), ann(1, [80, 0, 10, 10], 'B', 2)]
    r = mot_ref.evaluate(gt2, hyp[:2] + [res(1, [80, 0, 10, 10], 1, 2), res(1, a1, 2, 2)])
    assert r['hyp_match'] == [0, 1, 3, 2] and counts(r['table'][2][2]) == (4, 4, 0, 0, 2)


def test_object_lost_for_three_frames_and_found_under_a_new_id():
    gt = [ann(f, A0, 'A') for f in range(6)]
    hyp = [res(0, A0, 1), res(1, A0, 1), res(5, A0, 9)]
    r = mot_ref.evaluate(gt, hyp)
    row = r['table'][1][2]
    assert counts(row) == (6, 3, 3, 0, 1)
    assert row['MOTA'] == 1.0 - 4 / 6
    assert r['hyp_switch'] == [0, 0, 1]


def test_level_2_object_leaves_level_1_unchanged():
    easy_gt = [ann(f, A0, 'A') for f in range(4)]
    easy_hyp = [res(f, A0, 1) for f in range(4)]
    # B is hard to track: matched (frame 0), missed (1), found under another id (2: a switch), matched (3)
    hard_gt = [ann(f, B0, 'B', level=2) for f in range(4)]
    hard_hyp = [res(0, B0, 2), res(2, B0, 3), res(3, B0, 3)]
    alone = mot_ref.evaluate(easy_gt, easy_hyp)
    both = mot_ref.evaluate(easy_gt + hard_gt, easy_hyp + hard_hyp)
    assert counts(both['table'][1][2]) == (8, 7, 1, 0, 1)
    assert counts(both['table'][1][1]) == (4, 4, 0, 0, 0) and both['table'][1][1]['MOTA'] == 1.0
    assert both['table'][1][1] == alone['table'][1][1]
    # a hypothesis that matches nothing is a false positive at both levels
    extra = mot_ref.evaluate(easy_gt + hard_gt, easy_hyp + hard_hyp + [res(1, [500, 500, 10, 10], 7)])
    assert counts(extra['table'][1][1]) == (4, 4, 0, 1, 0) and counts(extra['table'][1][2]) == (8, 7, 1, 1, 1)
    # tracking_difficulty_level absent = 1
    plain = mot_ref.evaluate([ann(f, A0, 'A', level=None) for f in range(4)], easy_hyp)
    assert plain['table'][1][1] == alone['table'][1][1]


def test_result_rows_on_frames_outside_images_are_ignored_not_false_positives():
    # ground truth exported every tenth frame
    gt = {'images': [{'id': image_id(0)}, {'id': image_id(10)}, {'id': image_id(20)}],
          'annotations': [ann(0, A0, 'A'), ann(10, A0, 'A')]}
    hyp = [res(f, A0, 1) for f in (0, 5, 10, 15, 20)] + [res(0, A0, 1, camera='SIDE_LEFT')]
    r = mot_ref.evaluate(gt, hyp)
    assert r['ignored_rows'] == 3 and r['hyp_match'] == [0, -2, 1, -2, -1, -2]
    assert counts(r['table'][1][2]) == (2, 2, 0, 1, 0)                          # frame 20 is in `images`: its row is a false positive
    # without `images` the frames are those that carry an annotation: frame 20 is not one of them
    r = mot_ref.evaluate(gt['annotations'], hyp)
    assert r['ignored_rows'] == 4 and counts(r['table'][1][2]) == (2, 2, 0, 0, 0)


def test_boxes_thinner_than_one_pixel_are_dropped_from_the_ground_truth():
    gt = [ann(0, A0, 'A'), ann(0, [50, 50, 0.5, 10], 'B'), ann(0, [70, 50, 10, 0], 'C')]
    r = mot_ref.evaluate(gt, [res(0, A0, 1)])
    assert counts(r['table'][1][2]) == (1, 1, 0, 0, 0)


def test_empty_result():
    gt = [ann(f, A0, 'A') for f in range(3)] + [ann(0, B0, 'B', 4, level=2)]
    r = mot_ref.evaluate(gt, [])
    assert counts(r['table']['ALL'][2]) == (4, 0, 4, 0, 0) and r['table']['ALL'][2]['MOTA'] == 0.0
    assert counts(r['table']['ALL'][1]) == (3, 0, 3, 0, 0)
    assert math.isnan(r['table']['ALL'][2]['MOTP']) and r['hyp_match'] == []


def test_empty_ground_truth():
    hyp = [res(0, A0, 1), res(1, A0, 1)]
    r = mot_ref.evaluate({'images': [{'id': image_id(0)}, {'id': image_id(1)}], 'annotations': []}, hyp)
    assert counts(r['table']['ALL'][2]) == (0, 0, 0, 2, 0)
    assert math.isnan(r['table']['ALL'][2]['MOTA']) and math.isnan(r['table']['ALL'][2]['MOTP'])
    r = mot_ref.evaluate([], hyp)                                               # no frames at all: nothing takes part
    assert r['ignored_rows'] == 2 and counts(r['table']['ALL'][2]) == (0, 0, 0, 0, 0)


def test_all_is_the_sum_of_the_three_evaluated_types():
    gt = [ann(0, A0, 'A', 1), ann(0, B0, 'B', 2), ann(0, [200, 0, 10, 10], 'C', 3), ann(0, [300, 0, 10, 10], 'D', 4)]
    hyp = [res(0, A0, 1, 1), res(0, [200, 0, 10, 10], 3, 3)]
    r = mot_ref.evaluate(gt, hyp)
    assert counts(r['table'][3][2]) == (1, 1, 0, 0, 0)
    assert counts(r['table']['ALL'][2]) == (3, 1, 2, 0, 0)                      # class 3 (sign) is not part of ALL


def random_gated_problem(rng):
    """1-40 boxes a side: ground-truth boxes, hypotheses = a random subset of them moved by 12 px jitter plus clutter."""
    n_g = int(rng.integers(1, 41))
    n_h = int(rng.integers(1, 41))
    w = rng.uniform(20, 300, n_g)
    h = rng.uniform(20, 300, n_g)
    x = rng.uniform(0, 1920 - w)
    y = rng.uniform(0, 1280 - h)
    g = np.stack([x, y, x + w, y + h], axis=1)
    src = rng.integers(0, n_g, n_h)
    hb = g[src] + rng.normal(0, 12.0, (n_h, 4))
    hb[:, 2:] = np.maximum(hb[:, 2:], hb[:, :2] + 1)
    thr = 0.5 if rng.integers(0, 2) == 0 else 0.7
    return [list(map(float, b)) for b in g], [list(map(float, b)) for b in hb], thr


def test_kept_pairs_do_not_depend_on_the_solver():
    """On random gated matrices the pairs kept (G > 0) equal those of scipy's linear_sum_assignment on -G in float64."""
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(0)
    agree = 0
    for _ in range(200):
        g, h, thr = random_gated_problem(rng)
        G = mot_ref.gated_matrix(g, h, thr)
        ours = mot_ref.assign(G)
        rows, cols = linear_sum_assignment(-G.astype(np.float64))
        theirs = sorted((int(i), int(j)) for i, j in zip(rows, cols) if G[i, j] > 0)
        assert sorted(ours) == theirs
        agree += 1
    assert agree == 200
