"""HIP track refinement (csrc/track_refine.hip through tracking/refine.py) against the plain-Python restatement
tests/refine_ref.py: rows, their order, the trace column, job_row_offsets and frame_row_offsets must be EQUAL bit for bit -
the unfused interpolation and the order of the score sum are part of the definition."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mot_ref
import refine_cases
import refine_ref

pytestmark = pytest.mark.gpu

TRACKER = [(3, 0, [0.3, 0.2, 1.0, 0.1], [0.01, 0.01, 1.0, 0.0]), (2, 1, [0.5, 0.5, 1.0, 0.5], [0.1, 0.1, 1.0, 0.1])]
JOBS = [refine_cases.job(max_gap=1, min_len=2), refine_cases.job(max_gap=[2, 1, 0, 3], min_len=[1, 3, 1, 2], score_mode='mean'),
        refine_cases.job(max_gap=3), refine_cases.job(min_len=4, score_mode='mean')]


def packed_for(offsets):
    """the part of a packed detection set that refinement reads, for hand-made slots"""
    offsets = np.asarray(offsets, np.int64)
    n_streams = offsets.size - 1
    ids = np.concatenate([np.arange(offsets[s + 1] - offsets[s]) * 10 + 5 for s in range(n_streams)] + [np.zeros(0, np.int64)])
    return {'stream_frame_offsets': offsets, 'frame_ids': ids.astype(np.int64), 'stream_keys': [('seg%d' % s, 'FRONT') for s in range(n_streams)]}


def arrays(result):
    return {'frame': np.asarray(result['frame'], np.int64), 'category': np.asarray(result['category'], np.int32),
            'bbox': np.asarray(result['bbox'], np.float64).reshape(-1, 4), 'score': np.asarray(result['score'], np.float64),
            'object_id': np.asarray(result['object_id'], np.int64)}


def assert_same(got, ref):
    assert got['frame'].tolist() == ref['frame']
    assert got['source'].tolist() == ref['source']
    assert got['category'].tolist() == ref['category']
    assert [int(v) for v in got['object_id']] == ref['object_id']
    assert got['bbox'].dtype == np.float64 and got['score'].dtype == np.float64
    assert got['bbox'].tobytes() == np.asarray(ref['bbox'], np.float64).reshape(-1, 4).tobytes()
    assert got['score'].tobytes() == np.asarray(ref['score'], np.float64).tobytes()
    assert got['frame_row_offsets'].tolist() == ref['frame_row_offsets']


def lds_limit():
    from waymo_2d_tracking_amd import _lib
    n = C.c_int32(0)
    _lib.lib().wt_refine_tracks_limits(C.byref(n))
    return n.value


@pytest.fixture(scope='module')
def tracked():
    """A synthetic sequence with detection dropouts tracked under two settings, max_age 3 first: (packed, [out, out])."""
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.tracking import utils as T
    dets, _ = syn.make_tracking_json(31, n_segments=1, n_frames=16, n_objects=30, integer_boxes=False)
    predictions = {}
    for e in dets:
        seg, fr, cam = e['image_id'].split('/')
        predictions.setdefault(seg, {}).setdefault(cam, {}).setdefault(int(fr), []).append(
            {'bbox': e['bbox'], 'score': e['score'], 'category_id': e['category_id']})
    packed = T.pack_streams(predictions)
    outs = [T.track_packed(packed, iou, max_age, min_hits, score)[0] for max_age, min_hits, score, iou in TRACKER]
    return packed, outs


@pytest.fixture(scope='module')
def tracked_refs(tracked):
    packed, outs = tracked
    return [[refine_ref.refine(packed['stream_frame_offsets'], out, j) for j in JOBS] for out in outs]


def test_identity_setting_reproduces_the_tracked_sequence(tracked):
    from waymo_2d_tracking_amd.tracking import refine as R
    packed, outs = tracked
    got = R.refine_tracks(packed, outs, [{'result': 0}, {'result': 1, 'max_gap': 0, 'min_len': 1, 'score_mode': 'keep'}])
    for out, g in zip(outs, got):
        assert len(out['frame']) > 300
        for name in ('frame', 'category', 'bbox', 'score', 'object_id'):
            assert g[name].dtype == out[name].dtype and g[name].tobytes() == out[name].tobytes(), name
        assert g['source'].tolist() == list(range(len(out['frame'])))


def test_settings_on_the_tracked_sequence_equal_the_reference(tracked, tracked_refs):
    from waymo_2d_tracking_amd.tracking import refine as R
    packed, outs = tracked
    got = R.refine_tracks(packed, outs[:1], JOBS)
    n_in = len(outs[0]['frame'])
    fills = [sum(1 for s in ref['source'] if s < 0) for ref in tracked_refs[0]]
    assert fills[0] > 10 and fills[2] > fills[0] and fills[3] == 0 and len(tracked_refs[0][0]['frame']) - fills[0] < n_in      # max_age 3 left holes
    for g, ref in zip(got, tracked_refs[0]):
        assert_same(g, ref)


def test_jobs_over_results_in_one_call_equal_single_calls_and_dev_equals_host(tracked, tracked_refs):
    import torch
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import refine as R
    packed, outs = tracked
    pairs = [(1, 0), (0, 1), (1, 3), (0, 2), (1, 1)]                          # (result, job): results interleaved, one job twice
    jobs = [dict(JOBS[j], result=r) for r, j in pairs]
    together = R.refine_tracks(packed, outs, jobs)
    dev = R.DeviceRefine(packed, outs, jobs)
    dev.launch()
    from_dev = dev.results()
    rows = [0]
    for (r, j), a, b in zip(pairs, together, from_dev):
        alone = R.refine_tracks(packed, [outs[r]], [JOBS[j]])[0]
        for other in (alone, a, b):
            assert_same(other, tracked_refs[r][j])
        rows.append(rows[-1] + len(tracked_refs[r][j]['frame']))
    assert dev.job_row_offsets.cpu().tolist() == rows
    # a second plan + emit on the same buffers gives the same answer (the calls initialise everything they read)
    dev.launch()
    dev.emit()
    for a, b in zip(from_dev, dev.results()):
        assert all(np.array_equal(a[k], b[k]) for k in a)
    # an output that is too small: WT_ERR_CAPACITY, nothing launched
    dev.launch()
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY'):
        dev.emit(out_cap=rows[-1] - 1)
    p = R._prepare(packed, outs, jobs, 4)
    job_rows = np.zeros(len(jobs) + 1, np.int64)
    o = [np.zeros(rows[-1], np.int64), np.zeros(rows[-1], np.int32), np.zeros((rows[-1], 4)), np.zeros(rows[-1]), np.zeros(rows[-1], np.int32),
         np.zeros(rows[-1], np.int64), np.zeros((len(jobs), p['n_frames'] + 1), np.int64)]
    assert R._host_call(p, rows[-1] - 1, o, job_rows) == 4 and job_rows.tolist() == rows and not o[0].any()
    assert R._host_call(p, rows[-1], o, job_rows) == 0 and o[5][:rows[1]].tolist() == tracked_refs[1][0]['source']
    torch.cuda.synchronize()


def test_unsorted_input_equals_the_sorted_one(tracked, tracked_refs):
    from waymo_2d_tracking_amd.tracking import refine as R
    packed, outs = tracked
    perm = np.random.default_rng(4).permutation(len(outs[0]['frame']))
    shuffled = dict((k, v[perm]) for k, v in outs[0].items())
    got = R.refine_tracks(packed, [shuffled], JOBS[:2])
    for g, j, ref in zip(got, JOBS, tracked_refs[0]):
        assert_same(g, refine_ref.refine(packed['stream_frame_offsets'], shuffled, j))
        # the rows are those of the sorted input wherever the order inside a slot does not matter: the filled ones, as a set
        key = lambda r: sorted(zip(r['frame'], r['object_id'], [tuple(b) for b in r['bbox']], r['score']))
        assert key({k: (v.tolist() if k != 'object_id' else [int(x) for x in v]) for k, v in g.items()}) == key(ref)


@pytest.mark.parametrize('name', sorted(refine_cases.CASES))
def test_case_equals_reference(name):
    from waymo_2d_tracking_amd.tracking import refine as R
    offsets, result, jobs, claim = refine_cases.CASES[name]()
    refs = [refine_ref.refine(offsets, result, j) for j in jobs]
    claim(refs)
    got = R.refine_tracks(packed_for(offsets), [arrays(result)], jobs)
    assert len(got) == len(refs)
    for g, ref in zip(got, refs):
        assert_same(g, ref)


@pytest.mark.parametrize('above', [0, 1], ids=['tables_in_lds', 'tables_in_workspace'])
def test_trajectory_counts_on_either_side_of_the_lds_limit(above):
    from waymo_2d_tracking_amd.tracking import refine as R
    limit = lds_limit()
    assert 64 < limit <= 4096
    offsets, result, jobs, claim = refine_cases.many_trajectories(limit + above)
    refs = [refine_ref.refine(offsets, result, j) for j in jobs]
    claim(refs)
    p = R._prepare(packed_for(offsets), [arrays(result)], jobs, 4)
    assert p['n_traj'].tolist() == [[limit + above]]
    for g, ref in zip(R.refine_tracks(packed_for(offsets), [arrays(result)], jobs), refs):
        assert_same(g, ref)
    dev = R.DeviceRefine(packed_for(offsets), [arrays(result)], jobs)
    dev.launch()
    for g, ref in zip(dev.results(), refs):
        assert_same(g, ref)


def test_same_local_index_in_two_jobs_does_not_link():
    """two results whose trajectories have the same local indices, refined by two jobs in one call: each keeps its own links"""
    from waymo_2d_tracking_amd.tracking import refine as R
    a = refine_cases.result([(0, 1, refine_cases.box(0, 0), 0.5, 1), (2, 1, refine_cases.box(0, 2), 0.5, 1)])
    b = refine_cases.result([(1, 1, refine_cases.box(1, 1), 0.5, 1), (4, 1, refine_cases.box(1, 4), 0.5, 1)])
    jobs = [dict(refine_cases.job(max_gap=2), result=0), dict(refine_cases.job(max_gap=2), result=1), dict(refine_cases.job(max_gap=1), result=1)]
    got = R.refine_tracks(packed_for([0, 5]), [arrays(a), arrays(b)], jobs)
    refs = [refine_ref.refine([0, 5], r, j) for r, j in ((a, jobs[0]), (b, jobs[1]), (b, jobs[2]))]
    assert [r['frame'] for r in refs] == [[0, 1, 2], [1, 2, 3, 4], [1, 4]]
    for g, ref in zip(got, refs):
        assert_same(g, ref)


def test_duplicate_trajectory_in_a_slot_is_invalid_and_names_the_image():
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import refine as R
    rows = [(0, 1, [0, 0, 5, 5], 0.5, 1), (3, 1, [0, 0, 5, 5], 0.5, 2), (4, 1, [0, 0, 5, 5], 0.5, 3), (4, 1, [9, 9, 5, 5], 0.5, 2), (4, 1, [1, 1, 5, 5], 0.5, 3)]
    packed = packed_for([0, 3, 6])
    with pytest.raises(_lib.WaymoTrackError, match=r'WT_ERR_INVALID \(result 0: object_id 3 occurs twice in image seg1/15/FRONT\)'):
        R.refine_tracks(packed, [arrays(refine_cases.result(rows))], [refine_cases.job()])
    # the C entry point on its own: the same layout, the duplicate written into the trajectory indices
    p = R._prepare(packed, [arrays(refine_cases.result(rows[:4]))], [refine_cases.job()], 4)
    job_rows = np.zeros(2, np.int64)
    assert R._host_call(p, 0, [None] * 7, job_rows) == 0 and job_rows.tolist() == [0, 4]
    p['local'][3] = p['local'][2]
    assert R._host_call(p, 0, [None] * 7, job_rows) == 1
    assert b'occurs twice in frame 4' in _lib.lib().wt_last_error()
    p['local'][3] = 7
    assert R._host_call(p, 0, [None] * 7, job_rows) == 1 and b'trajectory index 7 outside' in _lib.lib().wt_last_error()


def test_filling_a_missed_frame_removes_the_false_negative():
    """Two objects on straight lines; the result misses one of them in one interior slot: fn = 1 before, 0 after, fp unchanged.
    The ground-truth boxes are linear in the frame with steps that halve exactly, so the filled box IS the ground-truth box."""
    from waymo_2d_tracking_amd.tracking import evaluate as E, refine as R
    gt_box = lambda o, f: [100.0 * o + 8.0 * f, 50.0 + 4.0 * f, 40.0 + 2.0 * f, 30.0]
    anns = [{'image_id': 'seg0/%d/FRONT' % (f * 10 + 5), 'bbox': gt_box(o, f), 'category_id': 1, 'object_id': 'g%d' % o}
            for f in range(4) for o in (1, 2)]
    rows = [(f, 1, gt_box(o, f), 0.9, 10 + o) for f in range(4) for o in (1, 2) if not (o == 2 and f == 2)]
    packed, out = packed_for([0, 4]), arrays(refine_cases.result(rows))
    refined = R.refine_tracks(packed, [out], [{'max_gap': 1}])[0]
    assert_same(refined, refine_ref.refine([0, 4], out, refine_cases.job(max_gap=1)))
    assert refined['source'].tolist() == [0, 1, 2, 3, 4, -7, 5, 6] and refined['bbox'][5].tolist() == gt_box(2, 2)
    gt = E.load_ground_truth(anns)
    before, after = E.evaluate_tracks(gt, [E.tracks_from_packed(packed, out), E.tracks_from_packed(packed, refined)])
    for lv in (1, 2):
        b, a = before.table[1][lv], after.table[1][lv]
        assert (b['gt'], b['tp'], b['fn'], b['fp'], b['idsw']) == (8, 7, 1, 0, 0)
        assert (a['gt'], a['tp'], a['fn'], a['fp'], a['idsw']) == (8, 8, 0, 0, 0)


def _expected_file(path, score_thr, iou_thr, max_age, job):
    """what track.py has to write: the tracker's rows through the reference refinement and format_tracks"""
    from waymo_2d_tracking_amd.tracking import utils as T
    packed = T.pack_streams(T.read_data_file(path, score_thr))
    out, _ = T.track_packed(packed, iou_thr, max_age, 0)
    ref = refine_ref.refine(packed['stream_frame_offsets'], out, job)
    return T.format_tracks(packed, arrays(ref)), len(out['frame']), ref


@pytest.mark.parametrize('fixture,max_age', [('sort_g5_input.json', 1), ('sort_g4_input.json', 3)])
def test_cli_writes_the_refined_file(golden_dir, tmp_path, fixture, max_age):
    from waymo_2d_tracking_amd.tracking import track, utils as T
    path = os.path.join(golden_dir, fixture)
    score = [0.95, 0.6, 1.0, 0.9] if 'g5' in fixture else [0.3, 0.3, 1.0, 0.2]
    expected, n_tracked, ref = _expected_file(path, score, [0.01, 0.01, 1.0, 0.0], max_age, refine_cases.job(max_gap=1, min_len=2))
    if 'g4' in fixture:
        assert any(s < 0 for s in ref['source']) and len([s for s in ref['source'] if s >= 0]) < n_tracked
    flags = ['--input', path, '--max-age=%d' % max_age, '--score-threshold=' + ','.join(map(str, score)), '--interpolate-gap', '1', '--min-track-len', '2']
    for name, extra in (('native.json', []), ('python.json', ['--python-io'])):
        T.reset_global_ids(0)
        assert track.main(flags + ['--output', str(tmp_path / name)] + extra) == 0
    assert (tmp_path / 'python.json').read_text() == json.dumps(expected)
    assert (tmp_path / 'native.json').read_bytes() == (tmp_path / 'python.json').read_bytes()


def test_cli_default_flags_write_what_they_wrote(golden_dir, tmp_path):
    from waymo_2d_tracking_amd.tracking import track, utils as T
    for fixture, score in (('sort_g5_input.json', '0.95,0.6,1.0,0.9'), ('sort_g4_input.json', '0.3,0.3,1.0,0.2')):
        path = os.path.join(golden_dir, fixture)
        flags = ['--input', path, '--max-age=2', '--score-threshold=' + score]
        T.reset_global_ids(0)
        unrefined = json.dumps(T.track_all(T.read_data_file(path, [float(v) for v in score.split(',')]), [0.01, 0.01, 1.0, 0.0], 2, 0))
        written = []
        for i, extra in enumerate(([], ['--python-io'], ['--interpolate-gap=0', '--min-track-len=1,1,1,1', '--track-score=keep'])):
            T.reset_global_ids(0)
            assert track.main(flags + ['--output', str(tmp_path / ('t%d.json' % i))] + extra) == 0
            written.append((tmp_path / ('t%d.json' % i)).read_text())
        assert written[1] == unrefined and written[0] == written[1] == written[2]
    exp = json.load(open(os.path.join(golden_dir, 'sort_g4_expected_a.json')))['tracks']
    assert [(r['image_id'], r['category_id'], r['object_id']) for r in json.loads(written[0])] == [(r['image_id'], r['category_id'], r['object_id']) for r in exp]


@pytest.fixture(scope='module')
def sweep_set(tmp_path_factory):
    from waymo_2d_tracking_amd import synthetic as syn
    dets, gt_json = syn.make_tracking_json(23, n_segments=1, n_frames=10, n_objects=12, cameras=('FRONT', 'SIDE_LEFT'))
    path = tmp_path_factory.mktemp('refine_sweep') / 'det.json'
    path.write_text(json.dumps(dets))
    return str(path), dets, gt_json


def test_sweep_with_refinement_grids_equals_the_references(sweep_set):
    from waymo_2d_tracking_amd.tracking import evaluate as E, utils as T
    path, dets, gt_json = sweep_set
    grid = {'score': [0.3, 0.6], 'iou': [0.01], 'max_age': [1, 3], 'min_hits': [0], 'gap': [0, 1], 'min_len': [1, 2]}
    res = E.sweep(path, E.load_ground_truth(gt_json), grid)
    assert len(res['settings']) == 16 and res['settings'][1] == {'max_age': 1, 'min_hits': 0, 'score': 0.3, 'iou': 0.01, 'interp_gap': 0, 'min_len': 2}
    predictions = {}
    for e in dets:
        seg, fr, cam = e['image_id'].split('/')
        predictions.setdefault(seg, {}).setdefault(cam, {}).setdefault(int(fr), []).append(
            {'bbox': e['bbox'], 'score': e['score'], 'category_id': e['category_id']})
    packed = T.pack_streams(predictions)
    cache = {}

    def reference(max_age, min_hits, score, iou, gap, length):
        key = (max_age, min_hits, score, iou, gap, length)
        if key not in cache:
            out, _ = T.track_packed(packed, [iou] * 4, max_age, min_hits, [score] * 4)
            ref = refine_ref.refine(packed['stream_frame_offsets'], out, refine_cases.job(max_gap=gap, min_len=length))
            cache[key] = mot_ref.evaluate(gt_json, json.loads(json.dumps(T.format_tracks(packed, arrays(ref)))))['table']
        return cache[key]
    picked = set()
    for lv in (1, 2):
        assert len(res['ranked'][lv]) == 2
        for row in res['ranked'][lv]:
            total = dict((f, 0) for f in mot_ref.FIELDS)
            for c in E.ALL_CLASSES:
                i = c - 1
                picked.add((row['interp_gap'][i], row['min_len'][i]))
                table = reference(row['max_age'], row['min_hits'], row['score_threshold'][i], row['iou_threshold'][i], row['interp_gap'][i], row['min_len'][i])
                for f in mot_ref.FIELDS:
                    total[f] += table[c][lv][f]
            assert row['counts'] == total, (lv, row)
            assert row['interp_gap'][2] == 0 and row['min_len'][2] == 1
            assert ' --interpolate-gap=%s --min-track-len=%s' % (','.join(map(str, row['interp_gap'])), ','.join(map(str, row['min_len']))) in E.flag_line(row)
    assert picked != {(0, 1)}                        # refinement won somewhere: the new axes are live
    # every setting's table, not only the picked ones, for one (max_age, min_hits)
    for k in range(8, 16):
        s = res['settings'][k]
        table = reference(s['max_age'], s['min_hits'], s['score'], s['iou'], s['interp_gap'], s['min_len'])
        for c in E.ALL_CLASSES:
            assert [res['results'][k].table[c][2][f] for f in mot_ref.FIELDS] == [table[c][2][f] for f in mot_ref.FIELDS]


def test_sweep_with_default_grids_is_the_unrefined_sweep(sweep_set):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    path, _, gt_json = sweep_set
    grid = {'score': [0.3, 0.6], 'iou': [0.01, 0.1], 'max_age': [1, 3], 'min_hits': [0, 1]}
    gt = E.load_ground_truth(gt_json)
    old = E.sweep(path, gt, grid)                                       # no refinement axes: the code path before them
    new = E.sweep(path, gt, dict(grid, gap=[0], min_len=[1]))
    for key in ('settings', 'ranked', 'best'):
        assert json.dumps(old[key], sort_keys=True) == json.dumps(new[key], sort_keys=True)
    assert sorted(old) == sorted(new) and sorted(old['settings'][0]) == ['iou', 'max_age', 'min_hits', 'score']
    assert sorted(old['best'][2]) == ['MOTA', 'counts', 'iou_threshold', 'max_age', 'min_hits', 'score_threshold']
    assert 'interpolate' not in E.flag_line(new['best'][2]) and E.flag_line(new['best'][2]) == E.flag_line(old['best'][2])
    args = E.build_parser().parse_args(['--annotations', 'x'])
    assert args.gap_grid == '0' and args.min_len_grid == '1'
