"""HIP identity metric (csrc/mot_identity.hip through tracking/evaluate.py) against the plain-Python restatement
tests/mot_id_ref.py: idtp, gt and hyp must be EQUAL for every stream, class and level.  The matching behind idtp is not unique,
so the per-row output is checked for consistency, never compared with the reference's matching."""
import ctypes
import json
import math

import numpy as np
import pytest

import mot_id_ref
from mot_support import SETTINGS, _copy_as_result, _track, assert_mot_equals_reference, same_number

pytestmark = pytest.mark.gpu

THR = mot_id_ref.DEFAULT_IOU_THRESHOLD


@pytest.fixture(scope='module', params=[True, False], ids=['integer_boxes', 'fractional_boxes'])
def sequence(request):
    """Ground truth, the three tracked results and the reference's answer for each (computed once, never changed)."""
    from waymo_2d_tracking_amd import synthetic as syn
    dets, gt_json = syn.make_tracking_json(11 if request.param else 12, n_segments=1, n_frames=24, n_objects=40,
                                           integer_boxes=request.param)
    results = [_track(dets, *s) for s in SETTINGS]
    refs = [mot_id_ref.evaluate(gt_json, r) for r in results]
    return gt_json, results, refs


def assert_equals_reference(got, ref, n_classes=4):
    """IdentityResult == mot_id_ref.evaluate() output: counts, table and ignored rows, exactly."""
    assert got.stream_keys == ref['stream_keys']
    for s, key in enumerate(got.stream_keys):
        for c in range(1, n_classes + 1):
            for li, lv in enumerate((1, 2)):
                exp = ref['per_stream'][key][c][lv]
                assert got.id_counts[s, c - 1, li].tolist() == [exp[f] for f in mot_id_ref.FIELDS], (key, c, lv)
    assert got.ignored_rows == ref['ignored_rows']
    assert set(got.table) == set(ref['table'])
    for c, rows in ref['table'].items():
        for lv, row in rows.items():
            assert set(got.table[c][lv]) == set(row)
            for name, v in row.items():
                assert same_number(got.table[c][lv][name], v), (c, lv, name, got.table[c][lv][name], v)


def test_device_equals_reference_on_tracked_sequences(sequence):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    gt_json, results, refs = sequence
    # non-trivial by the reference's own numbers: three different results, identities partly kept, LEVEL_1 a strict subset
    assert len(set(json.dumps(r['table']['ALL'], sort_keys=True) for r in refs)) == 3
    assert any(0 < r['table']['ALL'][2]['idtp'] < r['table']['ALL'][2]['gt'] for r in refs)
    assert all(r['table']['ALL'][1]['gt'] < r['table']['ALL'][2]['gt'] for r in refs)
    gt = E.load_ground_truth(gt_json)
    got = E.evaluate_identity(gt, [E.load_tracks(r) for r in results])
    assert len(got) == 3
    for g, r in zip(got, refs):
        print(json.dumps(g.table['ALL'][2]), json.dumps(r['table']['ALL'][2]))
        assert_equals_reference(g, r)
        assert g.as_json()['table']['ALL']['LEVEL_2']['idtp'] == r['table']['ALL'][2]['idtp']


def assert_rows_consistent(gt_json, rows, got, n_classes=4):
    """hyp_idmatch of one result: per problem and level the matched rows number idtp, each names a ground-truth row of the same
    frame and class with IoU >= thr, the implied trajectory pairs are a one-to-one map, rows that took no part are -2."""
    annotations = gt_json['annotations'] if isinstance(gt_json, dict) else gt_json
    images = gt_json.get('images') if isinstance(gt_json, dict) else None
    known = set(im['id'] for im in images) if images is not None else set(a['image_id'] for a in annotations)
    assert got.hyp_idmatch.shape == (len(rows), 2)
    stream_of = dict((key, s) for s, key in enumerate(got.stream_keys))
    for li in (0, 1):
        count = np.zeros(got.id_counts.shape[:2], np.int64)
        to_h, to_o = {}, {}
        for i, r in enumerate(rows):
            m = int(got.hyp_idmatch[i, li])
            part = r['image_id'] in known and 1 <= r['category_id'] <= n_classes
            if not part:
                assert m == -2
                continue
            assert m >= -1 or (li == 0 and m == -2)
            if m < 0:
                continue
            a = annotations[m]
            assert a['image_id'] == r['image_id'] and a['category_id'] == r['category_id']
            assert mot_id_ref.iou(mot_id_ref.xyxy(a['bbox']), mot_id_ref.xyxy(r['bbox'])) >= THR[r['category_id'] - 1]
            assert li == 1 or a.get('tracking_difficulty_level', 1) != 2
            seg, _, cam = r['image_id'].split('/')
            o = (seg, cam, r['category_id'], a['object_id'])
            h = (seg, cam, r['category_id'], r['object_id'])
            assert to_h.setdefault(o, h) == h and to_o.setdefault(h, o) == o
            count[stream_of[(seg, cam)], r['category_id'] - 1] += 1
        assert np.array_equal(count, got.id_counts[:, :, li, 0])


def test_per_row_output_is_consistent(sequence):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    gt_json, results, refs = sequence
    sparse = dict(gt_json, images=gt_json['images'][::2])            # ground truth for every other frame: the other rows take no part
    for gj in (gt_json, sparse):
        got = E.evaluate_identity(E.load_ground_truth(gj), [E.load_tracks(r) for r in results], per_row=True)
        for g, rows in zip(got, results):
            assert_rows_consistent(gj, rows, g)
            assert int((g.hyp_idmatch[:, 1] == -2).sum()) == g.ignored_rows
    assert got[0].ignored_rows > 0
    assert_equals_reference(got[0], mot_id_ref.evaluate(sparse, results[0]))


def test_k_sets_in_one_call_equal_k_calls_and_dev_equals_host(sequence):
    import torch
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import evaluate as E
    gt_json, results, refs = sequence
    gt = E.load_ground_truth(gt_json)
    tracks = [E.load_tracks(r) for r in results]
    together = E.evaluate_identity(gt, tracks, per_row=True)
    dev = E.DeviceIdentity(gt, tracks)
    dev.launch()
    from_dev = dev.results(per_row=True)
    # a limit that admits every single result and no two together: one set per call
    p = E.pack_results(gt, tracks, 4)
    _, g_ntraj, _, h_ntraj = E.trajectory_indices(gt, p, 4)
    floats = E._matrix_floats(g_ntraj, h_ntraj).reshape(3, -1).sum(axis=1)
    limit = max(E._identity_workspace(_lib.lib(), 1, len(gt['stream_keys']), 4, int(g_ntraj.max()), int(h_ntraj[k].max()), int(floats[k]))
                for k in range(3))
    assert E._identity_calls(_lib.lib(), g_ntraj, h_ntraj, limit) == [(0, 1), (1, 2), (2, 3)]
    assert E._identity_calls(_lib.lib(), g_ntraj, h_ntraj, E.DEFAULT_WORKSPACE_LIMIT) == [(0, 3)]
    split = E.evaluate_identity(gt, tracks, per_row=True, workspace_limit_bytes=limit)
    for k, tr in enumerate(tracks):
        alone = E.evaluate_identity(gt, [tr], per_row=True)[0]
        for other in (together[k], from_dev[k], split[k]):
            assert np.array_equal(alone.id_counts, other.id_counts) and alone.ignored_rows == other.ignored_rows
            assert other.table == alone.table or all(same_number(other.table[c][lv][n], v) for c, rows in alone.table.items()
                                                     for lv, row in rows.items() for n, v in row.items())
        assert_rows_consistent(gt_json, results[k], from_dev[k])
        assert_equals_reference(split[k], refs[k])
    # a second launch on the same buffers gives the same answer (the call initialises everything it reads)
    dev.launch()
    again = dev.results(per_row=True)
    assert all(np.array_equal(a.id_counts, b.id_counts) and np.array_equal(a.hyp_idmatch, b.hyp_idmatch) for a, b in zip(from_dev, again))
    torch.cuda.synchronize()


def _without_dont_care_on_counted(gt_json):
    """The ground truth without the level-2 boxes that reach the class's threshold with a counted box of their frame and class.
    A copy of such a box is a hypothesis that stays in LEVEL_1's hyp (it reaches a counted box) while its own box is not in
    LEVEL_1's gt, so against itself that ground truth has hyp > gt at LEVEL_1: by the definition, not by the kernel."""
    by_frame = {}
    for a in gt_json['annotations']:
        by_frame.setdefault((a['image_id'], a['category_id']), []).append(a)
    keep = []
    for a in gt_json['annotations']:
        if a.get('tracking_difficulty_level', 1) == 2 and 1 <= a['category_id'] <= 4 and any(
                g.get('tracking_difficulty_level', 1) != 2 and
                mot_id_ref.iou(mot_id_ref.xyxy(a['bbox']), mot_id_ref.xyxy(g['bbox'])) >= THR[a['category_id'] - 1]
                for g in by_frame[(a['image_id'], a['category_id'])]):
            continue
        keep.append(a)
    return dict(gt_json, annotations=keep)


def test_ground_truth_against_itself_and_against_nothing(sequence):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    gt_json, _, _ = sequence
    clean = _without_dont_care_on_counted(gt_json)
    assert len(gt_json['annotations']) - 40 < len(clean['annotations']) <= len(gt_json['annotations'])
    gt = E.load_ground_truth(clean)
    itself, nothing = E.evaluate_identity(gt, [E.load_tracks(_copy_as_result(clean)), E.load_tracks([])])
    for lv in (1, 2):
        row = itself.table['ALL'][lv]
        assert row['idtp'] == row['gt'] == row['hyp'] > 0 and row['idf1'] == 1.0 and row['idp'] == 1.0 and row['idr'] == 1.0
        row = nothing.table['ALL'][lv]
        assert row['idtp'] == 0 and row['gt'] == itself.table['ALL'][lv]['gt'] and row['hyp'] == 0
        assert row['idr'] == 0.0 and math.isnan(row['idp']) and row['idf1'] == 0.0
    assert itself.table['ALL'][1]['gt'] < itself.table['ALL'][2]['gt']
    # the unfiltered ground truth: every identity is kept (IDR 1), LEVEL_2 is 1.0, and LEVEL_1's hyp may exceed its gt (see above)
    rows = _copy_as_result(gt_json)
    full = E.evaluate_identity(E.load_ground_truth(gt_json), [E.load_tracks(rows)])[0]
    assert_equals_reference(full, mot_id_ref.evaluate(gt_json, rows))
    assert full.table['ALL'][2]['idf1'] == 1.0 and full.table['ALL'][1]['idr'] == 1.0
    assert full.table['ALL'][1]['hyp'] >= full.table['ALL'][1]['gt'] == full.table['ALL'][1]['idtp']


def test_empty_sides_through_all_four_forms():
    """The early returns of the library: a result without rows, a result whose rows all lie on frames the ground truth does not
    have, and a ground truth without streams.  Host and device form of both metrics, each against its reference."""
    import mot_ref
    from waymo_2d_tracking_amd.tracking import evaluate as E
    anns = [{'image_id': 'seg/%d/FRONT' % f, 'bbox': [100 * i + 3 * f, 10, 50, 60], 'category_id': 1 + i, 'object_id': 'o%d' % i,
             'tracking_difficulty_level': 1 + i} for f in range(3) for i in range(2)]
    rows = [{'image_id': 'seg/%d/FRONT' % f, 'bbox': [100 * i, 12, 50, 60], 'score': 0.9, 'category_id': 1 + i, 'object_id': str(i)}
            for f in (7, 8) for i in range(2)]
    for name, a, r, n_gt, ignored in (('empty_result', anns, [], 6, 0), ('rows_on_other_frames', anns, rows, 6, 4),
                                      ('empty_ground_truth', [], rows[:2], 0, 2)):
        mot_exp, id_exp = mot_ref.evaluate(a, r), mot_id_ref.evaluate(a, r)
        assert (mot_exp['table']['ALL'][2]['gt'], mot_exp['ignored_rows'], id_exp['table']['ALL'][2]['gt']) == (n_gt, ignored, n_gt), name
        gt, tracks = E.load_ground_truth(a), [E.load_tracks(r)]
        assert len(gt['stream_keys']) == (1 if a else 0)
        dev_mot, dev_id = E.DeviceEvaluation(gt, tracks), E.DeviceIdentity(gt, tracks)
        dev_mot.launch()
        dev_id.launch()
        mot = [E.evaluate_tracks(gt, tracks, per_row=True)[0], dev_mot.results(per_row=True)[0]]
        ident = [E.evaluate_identity(gt, tracks, per_row=True)[0], dev_id.results(per_row=True)[0]]
        for got in mot:
            assert_mot_equals_reference(got, mot_exp)
            assert np.array_equal(got.counts, mot[0].counts) and np.array_equal(got.iou_sum, mot[0].iou_sum), name
            assert np.array_equal(got.hyp_match, mot[0].hyp_match) and np.array_equal(got.hyp_switch, mot[0].hyp_switch), name
        for got in ident:
            assert_equals_reference(got, id_exp)
            assert np.array_equal(got.id_counts, ident[0].id_counts) and got.hyp_idmatch.shape == (len(r), 2), name
            assert (got.hyp_idmatch == -2).all(), name                       # no row took part
            assert_rows_consistent(a, r, got)


def _limits():
    from waymo_2d_tracking_amd import _lib
    n, stars, zmask = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.lib().wt_mot_identity_limits(ctypes.byref(n), ctypes.byref(stars), ctypes.byref(zmask))
    return n.value, stars.value, zmask.value


def _crowd(seed, n_gt, n_hyp, n_frames=2, cat=2):
    """Well-separated boxes on a grid over a few frames.  Hypothesis slot j sits on object j (slots beyond the objects sit on
    free grid cells); after frame 0 a third of the slots pass their id on to the next slot of that third, so a trajectory
    collects boxes of two objects and the best map is not 'slot j - object j'.  Ids are random labels."""
    rng = np.random.default_rng(seed)
    cells = max(n_gt, n_hyp)
    label = rng.permutation(10 * cells)[:cells]
    anns, rows = [], []
    for f in range(n_frames):
        ids = np.arange(n_hyp)
        if f > 0:
            moved = np.nonzero(rng.random(n_hyp) < 0.34)[0]
            ids[moved] = np.roll(moved, f)
        for i in range(cells):
            x, y = 20 + 90 * (i % 40), 20 + 90 * (i // 40)
            if i < n_gt:
                anns.append({'image_id': 'seg/%d/FRONT' % f, 'bbox': [x, y, 60 + (i % 7), 60 + (i % 5)], 'category_id': cat,
                             'object_id': 'o%d' % i, 'tracking_difficulty_level': 2 if i % 6 == 0 else 1})
            if i < n_hyp:
                jit = rng.normal(0, 1.5, 4)
                rows.append({'image_id': 'seg/%d/FRONT' % f, 'bbox': [x + jit[0], y + jit[1], 60 + (i % 7) + jit[2], 60 + (i % 5) + jit[3]],
                             'score': 0.9, 'category_id': cat, 'object_id': str(int(label[ids[i]]))})
    return anns, json.loads(json.dumps(rows))


def _storage_cases():
    """(name, objects, hypotheses): the smallest trajectory counts that cross each threshold of the implementation."""
    _, stars, zmask = _limits()
    n_z = next(n for n in range(1, 4097) if n * ((n + 63) // 64) * 8 > zmask)          # square problem whose bitmaps leave LDS
    n_s = next(n for n in range(1, 4097) if (3 * n * 4 + 15) // 16 * 16 > stars)       # ... whose star arrays leave LDS
    return [('registers_128', 70, 100), ('registers_384', 100, 129), ('bitmaps_in_lds', 100, 385),
            ('more_objects_than_hypotheses', 150, 60), ('rows_beyond_128', 129, 129),
            ('bitmaps_in_workspace', n_z, n_z), ('stars_in_workspace', n_s, n_s)]


@pytest.mark.parametrize('case', range(7), ids=['registers_128', 'registers_384', 'bitmaps_in_lds', 'more_objects_than_hypotheses',
                                                'rows_beyond_128', 'bitmaps_in_workspace', 'stars_in_workspace'])
def test_every_storage_path(case):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    name, n_gt, n_hyp = _storage_cases()[case]
    anns, rows = _crowd(40 + case, n_gt, n_hyp)
    ref = mot_id_ref.evaluate(anns, rows)
    r2, r1 = ref['table'][2][2], ref['table'][2][1]
    print(name, n_gt, n_hyp, r1, r2)
    assert 0 < r2['idtp'] < min(r2['gt'], r2['hyp']) and 0 < r1['idtp'] < r2['idtp'] and r1['hyp'] < r2['hyp']
    got = E.evaluate_identity(E.load_ground_truth(anns), [E.load_tracks(rows)], per_row=True)[0]
    assert_equals_reference(got, ref)
    assert_rows_consistent(anns, rows, got)


def test_capacity_and_workspace_errors(sequence):
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import evaluate as E
    limit = _limits()[0]
    assert limit == 4096
    anns = [{'image_id': 'seg/7/FRONT', 'bbox': [i % 100 * 3, i // 100 * 3, 2, 2], 'category_id': 1, 'object_id': 'o%d' % i}
            for i in range(limit + 1)]
    rows = [{'image_id': 'seg/7/FRONT', 'bbox': [0, 0, 2, 2], 'score': 1.0, 'category_id': 1, 'object_id': '1'}]
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY'):
        E.evaluate_identity(E.load_ground_truth(anns), [E.load_tracks(rows)])
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY'):
        E.DeviceIdentity(E.load_ground_truth(anns), [E.load_tracks(rows)])
    # 4096 is allowed: one pair reaches the threshold
    got = E.evaluate_identity(E.load_ground_truth(anns[:limit]), [E.load_tracks(rows)])[0]
    assert (got.table[1][2]['idtp'], got.table[1][2]['gt'], got.table[1][2]['hyp']) == (1, limit, 1)
    # a workspace smaller than the call needs: refused before anything is launched, by both forms
    gt_json, results, _ = sequence
    gt, tracks = E.load_ground_truth(gt_json), [E.load_tracks(results[0])]
    need = E.DeviceIdentity(gt, tracks).ws_bytes
    small = E.DeviceIdentity(gt, tracks, workspace_bytes=need - 1)
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_INVALID.*workspace too small'):
        small.launch()
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_INVALID.*workspace too small'):
        E.evaluate_identity(gt, tracks, workspace_limit_bytes=need - 1)
    # a trajectory twice in one frame: the library names the frame
    dup = rows + [dict(rows[0], bbox=[50, 50, 2, 2])]
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_INVALID'):
        E.evaluate_identity(E.load_ground_truth(anns[:10]), [E.load_tracks(dup)])


def test_cli_identity_tables_equal_the_api(tmp_path, capsys):
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.tracking import evaluate as E, track
    dets, gt_json = syn.make_tracking_json(21, n_segments=2, n_frames=12, n_objects=25, cameras=('FRONT', 'SIDE_LEFT'))
    (tmp_path / 'det.json').write_text(json.dumps(dets))
    gt_json = dict(gt_json, images=gt_json['images'][::2])           # ground truth for every other frame only
    (tmp_path / 'gt.json').write_text(json.dumps(gt_json))
    outs = []
    for i, flags in enumerate((['--max-age=2', '--min-hits=0', '--score-threshold=0.5,0.5,1.0,0.5'], ['--max-age=1', '--python-io'])):
        outs.append(str(tmp_path / ('tracks%d.json' % i)))
        assert track.main(['--input', str(tmp_path / 'det.json'), '--output', outs[-1]] + flags) == 0
    gt = E.load_ground_truth(str(tmp_path / 'gt.json'))
    tracks = [E.load_tracks(p) for p in outs]
    mot, ident = E.evaluate_tracks(gt, tracks), E.evaluate_identity(gt, tracks)
    capsys.readouterr()
    # without --identity: today's text and today's JSON
    assert E.main(['--annotations', str(tmp_path / 'gt.json'), '--json', str(tmp_path / 'mota.json')] + outs) == 0
    assert capsys.readouterr().out == ''.join(E.format_table(r, p) + '\n' for p, r in zip(outs, mot))
    assert (tmp_path / 'mota.json').read_text() == json.dumps(dict((p, r.as_json()) for p, r in zip(outs, mot)))
    # with it: the same tables, each followed by the identity table
    assert E.main(['--annotations', str(tmp_path / 'gt.json'), '--identity', '--json', str(tmp_path / 'id.json')] + outs) == 0
    assert capsys.readouterr().out == ''.join(E.format_table(r, p) + '\n' + E.format_identity_table(ir, p) + '\n'
                                              for p, r, ir in zip(outs, mot, ident))
    saved = json.loads((tmp_path / 'id.json').read_text())
    for p, ir in zip(outs, ident):
        ref = mot_id_ref.evaluate(gt_json, json.loads(open(p).read()))
        assert ref['ignored_rows'] == ir.ignored_rows > 0
        for c in (1, 2, 4, 'ALL'):
            for lv in (1, 2):
                for name, v in ref['table'][c][lv].items():
                    assert same_number(ir.table[c][lv][name], v) and same_number(saved[p]['identity'][str(c)]['LEVEL_%d' % lv][name], v)
        line = [ln for ln in E.format_identity_table(ir, p).split('\n') if ln.startswith('ALL    LEVEL_2')][0].split()
        assert [int(v) for v in line[2:5]] == [ref['table']['ALL'][2][k] for k in ('idtp', 'idfn', 'idfp')]


def test_sweep_ranked_by_idf1_picks_what_mot_id_ref_picks(tmp_path, capsys):
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.tracking import evaluate as E
    dets, gt_json = syn.make_tracking_json(31, n_segments=1, n_frames=16, n_objects=30, cameras=('FRONT', 'FRONT_LEFT'), clutter=0.3)
    (tmp_path / 'det.json').write_text(json.dumps(dets))
    (tmp_path / 'gt.json').write_text(json.dumps(gt_json))
    grid = {'score': [0.2, 0.7], 'iou': [0.01, 0.3], 'max_age': [2], 'min_hits': [0]}
    res = E.sweep(str(tmp_path / 'det.json'), E.load_ground_truth(gt_json), grid, rank_by='idf1')
    assert len(res['settings']) == 4 and len(res['id_results']) == 4
    refs = {}
    for score in grid['score']:
        for iou in grid['iou']:
            refs[score, iou] = mot_id_ref.evaluate(gt_json, _track(dets, 2, 0, [score] * 4, [iou] * 4))['table']
    assert len(set(json.dumps(t['ALL'], sort_keys=True) for t in refs.values())) > 1
    for lv in (1, 2):
        total = {'idtp': 0, 'gt': 0, 'hyp': 0}
        got = res['best'][lv]
        for c in (1, 2, 4):
            top = None
            for score in grid['score']:                               # grid order, the first of equals wins
                for iou in grid['iou']:
                    v = refs[score, iou][c][lv]['idf1']
                    v = v if v == v else -math.inf
                    if top is None or v > top[0]:
                        top = (v, score, iou)
            assert (got['score_threshold'][c - 1], got['iou_threshold'][c - 1]) == (top[1], top[2]), (lv, c)
            for f in total:
                total[f] += refs[top[1], top[2]][c][lv][f]
        assert got['id_counts'] == total and got['IDF1'] == mot_id_ref.finish(total)['idf1']
        assert got['score_threshold'][2] == 1.0 and got['iou_threshold'][2] == 1.0
    # --identity alone keeps the MOTA ranking and adds IDF1 to every ranked setting; the last line is the flag line of the best
    by_mota = E.sweep(str(tmp_path / 'det.json'), E.load_ground_truth(gt_json), grid, identity=True)
    plain = E.sweep(str(tmp_path / 'det.json'), E.load_ground_truth(gt_json), grid)
    for lv in (1, 2):
        assert [dict((k, v) for k, v in r.items() if k not in ('IDF1', 'id_counts')) for r in by_mota['ranked'][lv]] == plain['ranked'][lv]
        assert all('IDF1' in r for r in by_mota['ranked'][lv]) and not any('IDF1' in r for r in plain['ranked'][lv])
    capsys.readouterr()
    assert E.main(['--annotations', str(tmp_path / 'gt.json'), '--sweep', str(tmp_path / 'det.json'), '--score-grid', '0.2,0.7',
                   '--iou-grid', '0.01,0.3', '--max-age', '2', '--min-hits', '0', '--identity', '--rank-by', 'idf1']) == 0
    assert capsys.readouterr().out.rstrip('\n').split('\n')[-1] == E.flag_line(res['best'][2])
