"""HIP HOTA metric (csrc/mot_hota.hip through tracking/evaluate.py) against the plain-Python restatement tests/hota_ref.py.

hota_counts (gt, hyp, tp[19]) and hyp_match must be EQUAL to the restatement for every stream, class and level.  Of hota_sums, loc
is added in the restatement's order (frame, then ground-truth row) and must be equal too; ass / assre / asspr are sums of
non-negative terms that are bit-equal on both sides and differ only in the order they are added in (the kernel: per lane over the
cells, then over the lanes), so they may differ by the standard bound for such a sum, relative 2 n 2^-53 with n its number of terms.
Table values are a handful of correctly rounded operations on those sums (a quotient, a product, a square root, a mean of 19
non-negative values): the same bound with 64 added to n covers them.  The comparator that holds these bounds is
tests/mot_support.py's assert_hota_equals_reference: the sweep tests of the track post-passes use it too."""
import ctypes
import json
import math
import time

import numpy as np
import pytest

import hota_ref
from mot_support import EPS, SETTINGS, _copy_as_result, _track, assert_hota_equals_reference as assert_equals_reference, same_number

pytestmark = pytest.mark.gpu

THR = hota_ref.DEFAULT_IOU_THRESHOLD


def assert_rows_equal_reference(gt_json, rows, got, ref, n_classes=4):
    """hyp_match of one result equals the restatement's matching (the assignment is the same Munkres with the same tie-breaks), rows
    that took no part or are removed at a level are -2, and the matched pairs, IoU recomputed here, give tp at every threshold."""
    annotations = gt_json['annotations'] if isinstance(gt_json, dict) else gt_json
    assert got.hyp_match.shape == (len(rows), 2)
    stream_of = dict((key, s) for s, key in enumerate(got.stream_keys))
    for li, lv in enumerate((1, 2)):
        tp = np.zeros(got.hota_counts.shape[:2] + (19,), np.int64)
        for i, r in enumerate(rows):
            m = int(got.hyp_match[i, li])
            if i not in ref['part'] or i in ref['removed'][lv]:
                assert m == -2, (lv, i, m)
                continue
            assert m == ref['matches'][lv].get(i, -1), (lv, i, m)
            if m < 0:
                continue
            a = annotations[m]
            assert a['image_id'] == r['image_id'] and a['category_id'] == r['category_id']
            assert lv == 2 or a.get('tracking_difficulty_level', 1) != 2
            v = hota_ref.iou(hota_ref.xyxy(a['bbox']), hota_ref.xyxy(r['bbox']))
            seg, _, cam = r['image_id'].split('/')
            for t in range(19):
                if v >= (t + 1) / 20.0:
                    tp[stream_of[(seg, cam)], r['category_id'] - 1, t] += 1
        assert np.array_equal(tp, got.hota_counts[:, :, li, 2:])


def check(anns, rows, thr=THR):
    """Host form with per-row output against the restatement; returns (result, reference)."""
    from waymo_2d_tracking_amd.tracking import evaluate as E
    ref = hota_ref.evaluate(anns, rows, thr)
    got = E.evaluate_hota(E.load_ground_truth(anns), [E.load_tracks(rows)], thr, per_row=True)[0]
    assert_equals_reference(got, ref, len(thr))
    assert_rows_equal_reference(anns, rows, got, ref, len(thr))
    return got, ref


@pytest.fixture(scope='module', params=[True, False], ids=['integer_boxes', 'fractional_boxes'])
def sequence(request):
    """Ground truth over two streams, the three tracked results and the reference's answer for each (computed once, never changed)."""
    from waymo_2d_tracking_amd import synthetic as syn
    dets, gt_json = syn.make_tracking_json(11 if request.param else 12, n_segments=1, n_frames=14, n_objects=24,
                                           cameras=('FRONT', 'SIDE_LEFT'), integer_boxes=request.param)
    results = [_track(dets, *s) for s in SETTINGS]
    refs = [hota_ref.evaluate(gt_json, r) for r in results]
    return gt_json, results, refs


def test_device_equals_reference_on_tracked_sequences(sequence):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    gt_json, results, refs = sequence
    # non-trivial by the reference's own numbers: three different results, association partly lost, LEVEL_1 a strict subset, tp falling with alpha
    assert len(set(json.dumps(r['table']['ALL'][2]['tp']) for r in refs)) == 3
    assert any(0 < r['table']['ALL'][2]['AssA'] < 1 for r in refs)
    assert all(r['table']['ALL'][1]['gt'] < r['table']['ALL'][2]['gt'] for r in refs)
    assert all(r['table']['ALL'][2]['tp'][0] > r['table']['ALL'][2]['tp'][18] for r in refs)
    assert all(math.isnan(r['table'][3][2]['HOTA']) for r in refs)            # a class with no rows on either side
    gt = E.load_ground_truth(gt_json)
    got = E.evaluate_hota(gt, [E.load_tracks(r) for r in results], per_row=True)
    assert len(got) == 3
    for g, r, rows in zip(got, refs, results):
        print(json.dumps(dict((n, g.table['ALL'][2][n]) for n in hota_ref.NAMES)), json.dumps(dict((n, r['table']['ALL'][2][n]) for n in hota_ref.NAMES)))
        assert_equals_reference(g, r)
        assert_rows_equal_reference(gt_json, rows, g, r)
        assert g.hota() == g.table['ALL'][2]['HOTA'] and g.as_json()['table']['ALL']['LEVEL_2']['tp'] == r['table']['ALL'][2]['tp']


def test_rows_on_frames_without_ground_truth_take_no_part(sequence):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    gt_json, results, _ = sequence
    sparse = dict(gt_json, images=gt_json['images'][::2])
    ref = hota_ref.evaluate(sparse, results[0])
    got = E.evaluate_hota(E.load_ground_truth(sparse), [E.load_tracks(results[0])], per_row=True)[0]
    assert got.ignored_rows == ref['ignored_rows'] > 0 and int((got.hyp_match[:, 1] == -2).sum()) == got.ignored_rows
    assert_equals_reference(got, ref)
    assert_rows_equal_reference(sparse, results[0], got, ref)


def _same_result(a, b):
    return (np.array_equal(a.hota_counts, b.hota_counts) and np.array_equal(a.hota_sums, b.hota_sums) and a.ignored_rows == b.ignored_rows and
            np.array_equal(a.hyp_match, b.hyp_match))


def test_k_sets_in_one_call_equal_k_calls_and_dev_equals_host(sequence):
    import torch
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import evaluate as E
    gt_json, results, refs = sequence
    gt = E.load_ground_truth(gt_json)
    tracks = [E.load_tracks(r) for r in results]
    together = E.evaluate_hota(gt, tracks, per_row=True)
    dev = E.DeviceHota(gt, tracks)
    dev.launch()
    from_dev = dev.results(per_row=True)
    # a limit that admits every single result and no two together: one set per call
    p = E.pack_results(gt, tracks, 4)
    _, g_ntraj, _, h_ntraj = E.trajectory_indices(gt, p, 4)
    cells = E._matrix_cells(g_ntraj, h_ntraj).reshape(3, -1).sum(axis=1)
    boxes = E.max_frame_boxes(gt, p, 4)
    limit = max(E._hota_workspace(_lib.lib(), 1, len(gt['stream_keys']), 4, boxes, int(g_ntraj.max()), int(h_ntraj[k].max()), int(cells[k]))
                for k in range(3))
    assert E._hota_calls(_lib.lib(), g_ntraj, h_ntraj, boxes, limit) == [(0, 1), (1, 2), (2, 3)]
    assert E._hota_calls(_lib.lib(), g_ntraj, h_ntraj, boxes, E.DEFAULT_WORKSPACE_LIMIT) == [(0, 3)]
    split = E.evaluate_hota(gt, tracks, per_row=True, workspace_limit_bytes=limit)
    for k, tr in enumerate(tracks):
        alone = E.evaluate_hota(gt, [tr], per_row=True)[0]
        for other in (together[k], from_dev[k], split[k]):
            assert _same_result(alone, other)                    # bit for bit: the order of every sum is fixed
        assert_equals_reference(split[k], refs[k])
    # a second launch on the same buffers gives the same answer (the call initialises everything it reads)
    dev.launch()
    again = dev.results(per_row=True)
    assert all(_same_result(a, b) for a, b in zip(from_dev, again))
    torch.cuda.synchronize()


def test_ground_truth_against_itself_and_against_nothing(sequence):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    gt_json, _, _ = sequence
    rows = _copy_as_result(gt_json)
    gt = E.load_ground_truth(gt_json)
    itself, nothing = E.evaluate_hota(gt, [E.load_tracks(rows), E.load_tracks([])], per_row=True)
    row = itself.table['ALL'][2]
    assert row['HOTA'] == 1.0 and row['DetA'] == 1.0 and row['AssA'] == 1.0 and row['LocA'] == 1.0 and row['tp'] == [row['gt']] * 19
    assert row['gt'] == row['hyp'] > 0
    assert_equals_reference(itself, hota_ref.evaluate(gt_json, rows))
    assert_equals_reference(nothing, hota_ref.evaluate(gt_json, []))
    for lv in (1, 2):
        row = nothing.table['ALL'][lv]
        assert row['tp'] == [0] * 19 and row['hyp'] == 0 and row['gt'] == itself.table['ALL'][lv]['gt']
        assert row['HOTA'] == 0.0 and row['DetRe'] == 0.0 and math.isnan(row['DetPr']) and math.isnan(row['LocA']) and row['AssA'] == 0.0
    assert nothing.hyp_match.shape == (0, 2)


def test_empty_sides_through_both_forms():
    """The early returns of the library: a result without rows, a result whose rows all lie on frames the ground truth does not
    have, and a ground truth without streams.  Host and device form, each against the reference."""
    from waymo_2d_tracking_amd.tracking import evaluate as E
    anns = [{'image_id': 'seg/%d/FRONT' % f, 'bbox': [100 * i + 3 * f, 10, 50, 60], 'category_id': 1 + i, 'object_id': 'o%d' % i,
             'tracking_difficulty_level': 1 + i} for f in range(3) for i in range(2)]
    rows = [{'image_id': 'seg/%d/FRONT' % f, 'bbox': [100 * i, 12, 50, 60], 'score': 0.9, 'category_id': 1 + i, 'object_id': str(i)}
            for f in (7, 8) for i in range(2)]
    for name, a, r, n_gt, ignored in (('empty_result', anns, [], 6, 0), ('rows_on_other_frames', anns, rows, 6, 4),
                                      ('empty_ground_truth', [], rows[:2], 0, 2)):
        exp = hota_ref.evaluate(a, r)
        assert (exp['table']['ALL'][2]['gt'], exp['ignored_rows']) == (n_gt, ignored), name
        gt, tracks = E.load_ground_truth(a), [E.load_tracks(r)]
        dev = E.DeviceHota(gt, tracks)
        dev.launch()
        both = [E.evaluate_hota(gt, tracks, per_row=True)[0], dev.results(per_row=True)[0]]
        for got in both:
            assert_equals_reference(got, exp)
            assert _same_result(got, both[0]), name
            assert got.hyp_match.shape == (len(r), 2) and (got.hyp_match == -2).all(), name
            assert math.isnan(got.table['ALL'][2]['HOTA']) == (n_gt == 0), name


def test_dont_care_boxes_that_trigger_the_removal_rule_and_some_that_do_not():
    anns, rows = [], []
    for f in range(4):
        im = 'seg/%d/FRONT' % f
        anns += [{'image_id': im, 'bbox': [0, 0, 40, 40], 'category_id': 2, 'object_id': 'easy', 'tracking_difficulty_level': 1},
                 {'image_id': im, 'bbox': [200, 0, 40, 40], 'category_id': 2, 'object_id': 'hard', 'tracking_difficulty_level': 2},
                 {'image_id': im, 'bbox': [30, 0, 40, 40], 'category_id': 2, 'object_id': 'hard_on_easy', 'tracking_difficulty_level': 2},
                 {'image_id': im, 'bbox': [400, 0, 40, 40], 'category_id': 2, 'object_id': 'hard_alone', 'tracking_difficulty_level': 2}]
        rows += [{'image_id': im, 'bbox': [2 + f, 0, 40, 40], 'score': 1., 'category_id': 2, 'object_id': 'a'},         # on the counted box
                 {'image_id': im, 'bbox': [203, f, 40, 40], 'score': 1., 'category_id': 2, 'object_id': 'b'},           # only on a removed box: removed
                 {'image_id': im, 'bbox': [15, 0, 40, 40], 'score': 1., 'category_id': 2, 'object_id': 'c'},            # reaches both at 0.5: stays
                 {'image_id': im, 'bbox': [400 + 8 * f, 0, 40, 40], 'score': 1., 'category_id': 2, 'object_id': 'd'},   # drifts off a removed box: removed while it reaches 0.5
                 {'image_id': im, 'bbox': [600, 0, 40, 40], 'score': 1., 'category_id': 2, 'object_id': 'e'}]           # clutter
    got, ref = check(anns, rows)
    removed = sorted(rows[i]['object_id'] for i in ref['removed'][1])
    assert removed.count('b') == 4 and 'c' not in removed and 'a' not in removed and removed.count('d') == 2
    assert got.table[2][1]['gt'] == 4 and got.table[2][2]['gt'] == 16 and got.table[2][1]['hyp'] == 20 - len(removed)
    assert got.table[2][1]['HOTA'] != got.table[2][2]['HOTA']


def _grid_boxes(n, f, jitter, rng, prefix, cat=1):
    out = []
    for i in range(n):
        x, y = 20 + 90 * (i % 40), 20 + 90 * (i // 40)
        d = rng.normal(0, jitter, 4) if jitter else np.zeros(4)
        out.append({'image_id': 'seg/%d/FRONT' % f, 'bbox': [x + d[0], y + d[1], 60 + (i % 7) + d[2], 60 + (i % 5) + d[3]], 'score': 0.9,
                    'category_id': cat, 'object_id': '%s%d' % (prefix, i), 'tracking_difficulty_level': 2 if i % 6 == 5 else 1})
    return out


@pytest.mark.parametrize('n_gt,n_hyp', [(3, 65), (3, 130), (70, 5)], ids=['65_hypotheses', '130_hypotheses', '70_objects_transposed'])
def test_several_lane_chunks(n_gt, n_hyp):
    """More than 64 boxes on one side: several lane chunks in the column sweep (hypotheses) or in the row-sum sweep (objects), and
    the transposed assignment.  The many boxes crowd on the few: overlapping copies shifted by a few pixels, two frames."""
    rng = np.random.default_rng(n_gt * 1000 + n_hyp)
    anns, rows = [], []
    few, many = min(n_gt, n_hyp), max(n_gt, n_hyp)
    for f in range(2):
        small = [{'image_id': 'seg/%d/FRONT' % f, 'bbox': [100. + 300 * i, 50., 80., 90.], 'category_id': 1, 'object_id': 's%d' % i,
                  'score': 0.9, 'tracking_difficulty_level': 1} for i in range(few)]
        big = [{'image_id': 'seg/%d/FRONT' % f, 'bbox': [100. + 300 * (j % few) + float(rng.integers(-30, 31)), 50. + float(rng.integers(-30, 31)),
                                                       80., 90.], 'category_id': 1, 'object_id': 'b%d' % ((j + f) % many), 'score': 0.9,
                'tracking_difficulty_level': 2 if j % 9 == 0 else 1} for j in range(many)]
        anns += small if n_gt == few else big
        rows += big if n_gt == few else small
    rows = json.loads(json.dumps(rows))
    got, ref = check(anns, rows)
    assert got.table[1][2]['tp'][0] == 2 * few and got.table[1][2]['gt'] == 2 * n_gt and got.table[1][2]['hyp'] == 2 * n_hyp
    assert 0 < got.table[1][2]['AssA'] < 1


def _limits():
    from waymo_2d_tracking_amd import _lib
    boxes, traj, frames = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    cost, zmask = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.lib().wt_mot_hota_limits(ctypes.byref(boxes), ctypes.byref(traj), ctypes.byref(frames), ctypes.byref(cost), ctypes.byref(zmask))
    return boxes.value, traj.value, frames.value, cost.value, zmask.value


@pytest.mark.parametrize('which', ['matrix_in_workspace', 'bitmaps_in_workspace'])
def test_one_frame_beyond_the_lds_share(which):
    """The smallest square frame whose cost matrix (n * (n | 1) floats) or whose zero bitmaps (n * ceil(n / 64) * 8 bytes) leave LDS.
    Near-diagonal: every hypothesis sits on its own object, a few ids are exchanged between neighbours in the second frame."""
    _, _, _, cost, zmask = _limits()
    if which == 'matrix_in_workspace':
        n = next(n for n in range(1, 4097) if n * (n | 1) > cost)
    else:
        n = next(n for n in range(1, 4097) if n * ((n + 63) // 64) * 8 > zmask)
    assert (which, n) in (('matrix_in_workspace', 91), ('bitmaps_in_workspace', 513))
    rng = np.random.default_rng(n)
    anns = _grid_boxes(n, 0, 0, rng, 'o') + _grid_boxes(6, 1, 0, rng, 'o')
    rows = _grid_boxes(n, 0, 1.5, rng, 'h') + _grid_boxes(6, 1, 1.5, rng, 'h')
    for r in rows[n:]:
        r['object_id'] = 'h%d' % ((int(r['object_id'][1:]) + 1) % 6)             # the second frame passes the ids on
    rows = json.loads(json.dumps(rows))
    t0 = time.time()
    got, ref = check(anns, rows)
    print(which, n, 'restatement and device together: %.1f s' % (time.time() - t0))
    assert got.table[1][2]['tp'][0] == n + 6 and got.table[1][1]['gt'] < got.table[1][2]['gt'] and got.table[1][2]['AssA'] < 1


def _wide(i, W, w, oid, gt):
    """Pair i has frame i to itself, at the origin: x + w and y + h are then w and h exactly."""
    d = {'image_id': 'seg/%d/FRONT' % i, 'bbox': [0., 0., W if gt else w, 10.], 'category_id': 1, 'object_id': oid}
    d.update({'tracking_difficulty_level': 1} if gt else {'score': 1.0})
    return d


def test_iou_exactly_at_representable_thresholds():
    pairs = [(40., 10., 0.25), (20., 10., 0.5), (40., 30., 0.75)]
    anns = [_wide(i, W, w, 'o%d' % i, True) for i, (W, w, _) in enumerate(pairs)]
    rows = [_wide(i, W, w, 'h%d' % i, False) for i, (W, w, _) in enumerate(pairs)]
    for a, r, (_, _, v) in zip(anns, rows, pairs):
        assert hota_ref.iou(hota_ref.xyxy(a['bbox']), hota_ref.xyxy(r['bbox'])) == v
    got, ref = check(anns, rows)
    # 0.25 = alpha_4, 0.5 = alpha_9, 0.75 = alpha_14: each pair still counts at its own threshold
    assert got.table[1][2]['tp'] == [3] * 5 + [2] * 5 + [1] * 5 + [0] * 4


def _ulp_pairs():
    """For thresholds that are no float64 (0.05, 0.1, 0.15, 0.3, 0.35, 0.55, 0.6, 0.7, 0.85, 0.95 as the nearest double): box widths
    whose IoU, computed by the definition's operations, is the threshold's double, the double below it and the double above it."""
    rng = np.random.default_rng(5)
    found = []
    for a in (0, 1, 2, 5, 6, 10, 11, 13, 16, 18):
        alpha = (a + 1) / 20.0
        for target in (np.nextafter(alpha, 0.0), alpha, np.nextafter(alpha, 1.0)):
            hit = None
            for _ in range(2000):
                W = float(rng.uniform(50., 150.))
                w = alpha * W
                for k in range(-6, 7):
                    wk = w
                    for _ in range(abs(k)):
                        wk = float(np.nextafter(wk, math.inf if k > 0 else 0.0))
                    if hota_ref.iou([0., 0., W, 10.], [0., 0., wk, 10.]) == target:
                        hit = (W, wk)
                        break
                if hit:
                    break
            assert hit is not None, (a, target)
            found.append((a, float(target), hit))
    return found


def test_one_ulp_on_either_side_of_a_threshold():
    found = _ulp_pairs()
    anns = [_wide(i, W, w, 'o%d' % i, True) for i, (_, _, (W, w)) in enumerate(found)]
    rows = [_wide(i, W, w, 'h%d' % i, False) for i, (_, _, (W, w)) in enumerate(found)]
    expected = [0] * 19
    for a, target, _ in found:
        for t in range(19):
            expected[t] += 1 if target >= (t + 1) / 20.0 else 0
    below = [target for a, target, _ in found if target < (a + 1) / 20.0]
    assert len(below) == 10 and len(found) == 30
    got, ref = check(anns, rows)
    assert got.table[1][2]['tp'] == expected == ref['table'][1][2]['tp']


def test_alignment_beats_iou():
    from test_hota_ref import case_5
    anns, rows = case_5()
    got, ref = check(anns, rows)
    assert got.hyp_match[:, 1].tolist() == [0, 1, 2, -1]
    assert got.table[1][2]['tp'] == [3] * 16 + [0] * 3 and got.table[1][2]['hyp'] == 4
    assert got.table[1][2]['HOTA'] == pytest.approx(16 / 19 * math.sqrt(0.75), rel=1e-14)


def test_capacity_and_workspace_refusals_launch_nothing(sequence):
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import evaluate as E
    boxes, traj, frames, _, _ = _limits()
    assert (boxes, traj, frames) == (4096, 4096, 65535)
    anns = [{'image_id': 'seg/7/FRONT', 'bbox': [i % 100 * 3, i // 100 * 3, 2, 2], 'category_id': 1, 'object_id': 'o%d' % i}
            for i in range(boxes + 1)]
    rows = [{'image_id': 'seg/7/FRONT', 'bbox': [0, 0, 2, 2], 'score': 1.0, 'category_id': 1, 'object_id': '1'}]
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY'):
        E.evaluate_hota(E.load_ground_truth(anns), [E.load_tracks(rows)])
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY'):
        E.DeviceHota(E.load_ground_truth(anns), [E.load_tracks(rows)])
    gt_json, results, _ = sequence
    gt, tracks = E.load_ground_truth(gt_json), [E.load_tracks(results[0])]
    need = E.DeviceHota(gt, tracks).ws_bytes
    small = E.DeviceHota(gt, tracks, workspace_bytes=need - 1)
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_INVALID.*workspace too small'):
        small.launch()
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_INVALID.*workspace too small'):
        E.evaluate_hota(gt, tracks, workspace_limit_bytes=need - 1)


def test_cli_hota_tables_equal_the_api(tmp_path, capsys):
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.tracking import evaluate as E, track
    dets, gt_json = syn.make_tracking_json(21, n_segments=1, n_frames=10, n_objects=20, cameras=('FRONT', 'SIDE_LEFT'))
    (tmp_path / 'det.json').write_text(json.dumps(dets))
    (tmp_path / 'gt.json').write_text(json.dumps(gt_json))
    out = str(tmp_path / 'tracks.json')
    assert track.main(['--input', str(tmp_path / 'det.json'), '--output', out, '--max-age=2', '--min-hits=0']) == 0
    gt = E.load_ground_truth(str(tmp_path / 'gt.json'))
    tracks = [E.load_tracks(out)]
    mot, hota = E.evaluate_tracks(gt, tracks)[0], E.evaluate_hota(gt, tracks)[0]
    capsys.readouterr()
    assert E.main(['--annotations', str(tmp_path / 'gt.json'), out]) == 0                      # without --hota: today's text
    assert capsys.readouterr().out == E.format_table(mot, out) + '\n'
    assert E.main(['--annotations', str(tmp_path / 'gt.json'), '--hota', '--json', str(tmp_path / 'h.json'), out]) == 0
    assert capsys.readouterr().out == E.format_table(mot, out) + '\n' + E.format_hota_table(hota, out) + '\n'
    ref = hota_ref.evaluate(gt_json, json.loads(open(out).read()))
    assert_equals_reference(hota, ref)
    saved = json.loads((tmp_path / 'h.json').read_text())[out]['hota']
    line = [ln for ln in E.format_hota_table(hota, out).split('\n') if ln.startswith('ALL    LEVEL_2')][0].split()
    assert len(line) == 12 and float(line[2]) == pytest.approx(ref['table']['ALL'][2]['HOTA'], abs=6e-6)
    for c in (1, 2, 4, 'ALL'):
        for lv in (1, 2):
            assert saved[str(c)]['LEVEL_%d' % lv]['tp'] == ref['table'][c][lv]['tp']
            assert same_number(float(saved[str(c)]['LEVEL_%d' % lv]['HOTA']), hota.table[c][lv]['HOTA'])


def test_sweep_ranked_by_hota_picks_what_hota_ref_picks(tmp_path, capsys):
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.tracking import evaluate as E
    dets, gt_json = syn.make_tracking_json(31, n_segments=1, n_frames=10, n_objects=20, cameras=('FRONT', 'FRONT_LEFT'), clutter=0.3)
    (tmp_path / 'det.json').write_text(json.dumps(dets))
    (tmp_path / 'gt.json').write_text(json.dumps(gt_json))
    grid = {'score': [0.2, 0.7], 'iou': [0.01, 0.3], 'max_age': [2], 'min_hits': [0]}
    res = E.sweep(str(tmp_path / 'det.json'), E.load_ground_truth(gt_json), grid, rank_by='hota')
    assert len(res['settings']) == 4 and len(res['hota_results']) == 4 and 'id_results' not in res
    refs = {}
    for score in grid['score']:
        for iou in grid['iou']:
            refs[score, iou] = hota_ref.evaluate(gt_json, _track(dets, 2, 0, [score] * 4, [iou] * 4))['table']
    assert len(set(json.dumps(t['ALL'][2]['tp']) for t in refs.values())) > 1
    for lv in (1, 2):
        gt_n = hyp_n = 0
        tp = [0] * 19
        sums = dict((n, [0.] * 19) for n in ('ass', 'assre', 'asspr', 'loc'))
        got = res['best'][lv]
        for c in (1, 2, 4):
            top = None
            for score in grid['score']:                               # grid order, the first of equals wins
                for iou in grid['iou']:
                    v = refs[score, iou][c][lv]['HOTA']
                    v = v if v == v else -math.inf
                    if top is None or v > top[0]:
                        top = (v, score, iou)
            assert (got['score_threshold'][c - 1], got['iou_threshold'][c - 1]) == (top[1], top[2]), (lv, c)
            row = refs[top[1], top[2]][c][lv]
            gt_n, hyp_n = gt_n + row['gt'], hyp_n + row['hyp']
            for a in range(19):
                tp[a] += row['tp'][a]
                for n in sums:
                    sums[n][a] = sums[n][a] + row['sums'][n][a]
        exp = hota_ref.finish(gt_n, hyp_n, tp, sums['ass'], sums['assre'], sums['asspr'], sums['loc'])
        assert (got['hota_counts']['gt'], got['hota_counts']['hyp'], got['hota_counts']['tp']) == (gt_n, hyp_n, tp)
        for n in ('HOTA', 'DetA', 'AssA', 'LocA'):
            assert same_number(got[n], exp[n], 2 * (len(gt_json['annotations']) + 64) * EPS), (lv, n, got[n], exp[n])
        assert got['score_threshold'][2] == 1.0 and got['iou_threshold'][2] == 1.0
    # --hota alone keeps the MOTA ranking and adds HOTA to every ranked setting; the last line is the flag line of the best
    by_mota = E.sweep(str(tmp_path / 'det.json'), E.load_ground_truth(gt_json), grid, hota=True)
    plain = E.sweep(str(tmp_path / 'det.json'), E.load_ground_truth(gt_json), grid)
    extra = ('HOTA', 'DetA', 'AssA', 'LocA', 'hota_counts')
    for lv in (1, 2):
        assert [dict((k, v) for k, v in r.items() if k not in extra) for r in by_mota['ranked'][lv]] == plain['ranked'][lv]
        assert all('HOTA' in r for r in by_mota['ranked'][lv]) and not any('HOTA' in r for r in plain['ranked'][lv])
    capsys.readouterr()
    assert E.main(['--annotations', str(tmp_path / 'gt.json'), '--sweep', str(tmp_path / 'det.json'), '--score-grid', '0.2,0.7',
                   '--iou-grid', '0.01,0.3', '--max-age', '2', '--min-hits', '0', '--rank-by', 'hota']) == 0
    lines = capsys.readouterr().out.rstrip('\n').split('\n')
    assert lines[-1] == E.flag_line(res['best'][2]) and '  HOTA ' in lines[1] and 'IDF1' not in lines[1]
