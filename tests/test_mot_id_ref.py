"""The plain-Python identity metric tests/mot_id_ref.py on hand-worked cases, and its matching against
brute force and scipy.  No GPU: the device kernel is compared with this file in tests/test_gpu_mot_identity.py."""
import itertools
import math

import numpy as np
import pytest

import mot_id_ref as R

BOX = [100.0, 100.0, 40.0, 40.0]


def ann(frame, bbox, oid, cat=1, level=1, stream='seg', camera='FRONT'):
    return {'image_id': '%s/%d/%s' % (stream, frame, camera), 'bbox': list(bbox), 'category_id': cat, 'object_id': oid,
            'tracking_difficulty_level': level}


def row(frame, bbox, oid, cat=1, stream='seg', camera='FRONT'):
    return {'image_id': '%s/%d/%s' % (stream, frame, camera), 'bbox': list(bbox), 'score': 0.9, 'category_id': cat, 'object_id': oid}


def shifted(k):
    """A box that overlaps only itself among shifted(0), shifted(1), ..."""
    return [100.0 + 200 * k, 100.0, 40.0, 40.0]


def test_one_object_followed_by_two_ids():
    gt = [ann(f, BOX, 'o') for f in range(10)]
    rows = [row(f, BOX, 'A' if f <= 5 else 'B') for f in range(10)]
    t = R.evaluate(gt, rows)['table']
    for lv in (1, 2):
        r = t[1][lv]
        assert (r['idtp'], r['gt'], r['hyp'], r['idfn'], r['idfp']) == (6, 10, 10, 4, 4)
        assert r['idf1'] == 0.6 and r['idp'] == 0.6 and r['idr'] == 0.6
        assert t['ALL'][lv] == r


def test_row_greedy_would_be_wrong():
    """n(o1,A)=5, n(o1,B)=4, n(o2,A)=4, n(o2,B)=0: the best map is o1-B, o2-A = 8; taking o1's best first gives 5."""
    gt, rows = [], []
    f = 0
    for _ in range(5):                                 # o1 with A
        gt.append(ann(f, shifted(0), 'o1')); rows.append(row(f, shifted(0), 'A')); f += 1
    for _ in range(4):                                 # o1 with B, o2 with A
        gt.append(ann(f, shifted(0), 'o1')); rows.append(row(f, shifted(0), 'B'))
        gt.append(ann(f, shifted(1), 'o2')); rows.append(row(f, shifted(1), 'A')); f += 1
    r = R.evaluate(gt, rows)['table'][1][2]
    assert (r['idtp'], r['gt'], r['hyp']) == (8, 13, 13)
    assert R.max_overlap([[5, 4], [4, 0]]) == 8


def test_level_1_dont_care_rule():
    # frame 0: a hypothesis on a level-2 box only; frame 1: a hypothesis that reaches a level-2 box AND a counted box
    big = [100.0, 100.0, 40.0, 40.0]
    gt = [ann(0, big, 'hard', level=2), ann(0, shifted(2), 'easy'),
          ann(1, big, 'hard', level=2), ann(1, [102.0, 100.0, 40.0, 40.0], 'easy')]
    rows = [row(0, big, 'A'), row(0, shifted(2), 'B'), row(1, [101.0, 100.0, 40.0, 40.0], 'A')]
    res = R.evaluate(gt, rows)
    l1, l2 = res['table'][1][1], res['table'][1][2]
    assert (l2['gt'], l2['hyp']) == (4, 3)
    assert (l1['gt'], l1['hyp']) == (2, 2)             # A in frame 0 left out, A in frame 1 stays
    assert l2['idtp'] == 3                             # hard-A twice, easy-B once
    assert l1['idtp'] == 1                             # easy-B once and easy-A once: one object, one of them
    # without the counted box next to it, frame 1's hypothesis leaves LEVEL_1 as well
    res = R.evaluate([a for a in gt if not (a['object_id'] == 'easy' and a['image_id'] == 'seg/1/FRONT')], rows)
    assert res['table'][1][1]['hyp'] == 1 and res['table'][1][2]['hyp'] == 3


def test_threshold_is_inclusive():
    # IoU of [0,0,10,10] and [0,0,10,5] (xywh) is exactly 0.5; class 2's threshold is 0.5, class 1's 0.7
    gt = [ann(0, [0.0, 0.0, 10.0, 10.0], 'o', cat=2)]
    assert R.evaluate(gt, [row(0, [0.0, 0.0, 10.0, 5.0], 'A', cat=2)])['table'][2][2]['idtp'] == 1
    below = [0.0, 0.0, 10.0, float(np.nextafter(5.0, 0.0))]
    assert R.iou(R.xyxy(gt[0]['bbox']), R.xyxy(below)) < 0.5
    assert R.evaluate(gt, [row(0, below, 'A', cat=2)])['table'][2][2]['idtp'] == 0
    assert R.evaluate(gt, [row(0, [0.0, 0.0, 10.0, 5.0], 'A', cat=2)], (0.7, 0.7, 0.5, 0.5))['table'][2][2]['idtp'] == 0


def test_rows_outside_the_ground_truth_frames_are_ignored():
    gt = {'images': [{'id': 'seg/0/FRONT'}, {'id': 'seg/2/FRONT'}],
          'annotations': [ann(0, BOX, 'o'), ann(1, BOX, 'o'), ann(2, BOX, 'o')]}
    rows = [row(0, BOX, 'A'), row(1, BOX, 'A'), row(2, BOX, 'A'), row(0, BOX, 'A', stream='other'), row(0, BOX, 'Z', cat=9)]
    res = R.evaluate(gt, rows)
    assert res['ignored_rows'] == 3
    r = res['table'][1][2]
    assert (r['idtp'], r['gt'], r['hyp'], r['idf1']) == (2, 2, 2, 1.0)


def test_empty_sides_give_nan():
    gt = [ann(0, BOX, 'o')]
    r = R.evaluate(gt, [])['table'][1][2]
    assert (r['idtp'], r['gt'], r['hyp']) == (0, 1, 0) and r['idr'] == 0.0 and math.isnan(r['idp']) and r['idf1'] == 0.0
    r = R.evaluate(gt, [row(0, BOX, 'A', cat=2)])['table']
    assert math.isnan(r[2][2]['idr']) and r[2][2]['idp'] == 0.0 and r[2][2]['idf1'] == 0.0
    assert all(math.isnan(r[4][2][k]) for k in ('idp', 'idr', 'idf1'))


def test_the_same_hypothesis_id_in_two_classes_is_two_trajectories():
    gt = [ann(f, shifted(0), 'v', cat=1) for f in range(3)] + [ann(f, shifted(1), 'p', cat=2) for f in range(3)]
    rows = [row(f, shifted(0), '7', cat=1) for f in range(3)] + [row(f, shifted(1), '7', cat=2) for f in range(3)]
    t = R.evaluate(gt, rows)['table']
    assert t[1][2]['idtp'] == 3 and t[2][2]['idtp'] == 3
    assert (t['ALL'][2]['idtp'], t['ALL'][2]['gt'], t['ALL'][2]['hyp'], t['ALL'][2]['idf1']) == (6, 6, 6, 1.0)


def _brute(n):
    n = np.asarray(n)
    if n.shape[0] > n.shape[1]:
        n = n.T
    return max(sum(int(n[i, p[i]]) for i in range(n.shape[0])) for p in itertools.permutations(range(n.shape[1]), n.shape[0]))


def test_matching_equals_brute_force_on_small_matrices():
    rng = np.random.default_rng(5)
    for trial in range(120):
        a, b = int(rng.integers(1, 7)), int(rng.integers(1, 8))
        n = rng.integers(0, 6, (a, b)) * (rng.random((a, b)) < 0.6)
        assert R.max_overlap(n) == _brute(n), n


def test_matching_equals_scipy_on_sparse_matrices():
    opt = pytest.importorskip('scipy.optimize')
    rng = np.random.default_rng(6)
    for trial in range(25):
        a, b = int(rng.integers(1, 61)), int(rng.integers(1, 91))
        n = rng.integers(1, 30, (a, b)) * (rng.random((a, b)) < 0.08)
        r, c = opt.linear_sum_assignment(n, maximize=True)
        assert R.max_overlap(n) == int(n[r, c].sum())
