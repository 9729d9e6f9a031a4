"""HIP track deduplication (csrc/track_dedup.hip through tracking/dedup.py) against the plain-Python restatement
tests/dedup_ref.py: keep, by, match, the row mask, the counts and the surviving rows must be EQUAL bit for bit - no float is
produced, rows are only selected; the operation order of the IoU, the one multiplication of the fraction test and the strict
strength order are part of the definition.  The comparator and the bodies shared with the other
post-passes are in tests/track_stage_support.py."""
import json
import os

import numpy as np
import pytest

import dedup_cases
import dedup_ref
import mot_ref
import refine_cases
import refine_ref
import stitch_cases
import stitch_ref
import track_stage_support as H
from mot_support import assert_hota_equals_reference
from track_stage_support import COLUMNS, G4, G5, arrays, packed_for

pytestmark = pytest.mark.gpu

STAGE = H.STAGES['dedup']
assert_same = STAGE.assert_same
JOBS = [dedup_cases.job(min_frames=1, dup_iou=0.9, dup_frac=0.0),                             # the loosest: every injected copy is a duplicate
        dedup_cases.job(min_frames=[3, 2, 0, 1], dup_iou=[0.9, 0.5, 0.7, 0.8], dup_frac=[0.5, 1.0, 0.5, 0.25]),
        dedup_cases.job(min_frames=2, dup_iou=0.7, dup_frac=0.5),
        dedup_cases.job(min_frames=4, dup_iou=0.99, dup_frac=1.0)]                            # the strictest


def with_copies(packed, out):
    """Every third trajectory gets a copy on every second of its rows under a fresh object id: the box moved by 1 / 64 px - an IoU of
    at least (w - 1/64) / (w + 1/64) >= 0.969 with its original, boxes being at least one pixel wide - and half the score.  Returns
    the rows (copies appended: not sorted by frame) and the number of copies."""
    frame, oid = np.asarray(out['frame']), np.asarray(out['object_id'])
    stream = np.searchsorted(packed['stream_frame_offsets'], frame, side='right') - 1
    seen, picked = {}, []
    for i in np.argsort(frame, kind='stable'):
        seen.setdefault((int(stream[i]), int(oid[i])), []).append(int(i))
    fresh = int(oid.max()) + 1 if oid.size else 0
    new_ids = []
    for n, rows in enumerate(seen.values()):
        if n % 3 == 0:
            picked += rows[::2]
            new_ids += [fresh + n] * len(rows[::2])
    picked = np.asarray(picked, np.int64)
    bbox = np.asarray(out['bbox'])[picked].copy()
    bbox[:, 0] += 1.0 / 64.0
    copies = {'frame': frame[picked], 'category': np.asarray(out['category'])[picked], 'bbox': bbox,
              'score': np.asarray(out['score'])[picked] * 0.5, 'object_id': np.asarray(new_ids, oid.dtype)}
    return dict((k, np.concatenate([np.asarray(out[k]), copies[k]])) for k in COLUMNS), len(set(new_ids))


@pytest.fixture(scope='module')
def tracked(golden_dir):
    """The two tracking fixtures tracked with max_age 2, with injected copies: [(packed, out, copies, the tracker's own rows)], g4 first."""
    sets = []
    for packed, plain in H.tracked_fixtures(golden_dir):
        plain = dict((k, plain[k]) for k in COLUMNS)
        out, copies = with_copies(packed, plain)
        sets.append((packed, out, copies, plain))
    return sets


@pytest.fixture(scope='module')
def tracked_refs(tracked):
    return [[dedup_ref.dedup(packed['stream_frame_offsets'], out, j) for j in JOBS] for packed, out, _, _ in tracked]


@pytest.mark.parametrize('name', sorted(dedup_cases.CASES))
def test_case_equals_reference(name):
    H.check_case(STAGE, name)


def test_deep_chain_takes_one_round_per_link():
    from waymo_2d_tracking_amd.tracking import dedup as D
    offsets, result, jobs, claim = dedup_cases.deep_chain(40)
    dev = D.DeviceDedup(packed_for(offsets), [arrays(result)], jobs)
    dev.launch()
    assert dev.rounds().tolist() == [[40]]
    assert_same(dev.results()[0], dedup_ref.dedup(offsets, result, jobs[0]), arrays(result))


def test_all_zero_min_frames_reproduces_the_tracked_rows(tracked):
    from waymo_2d_tracking_amd.tracking import dedup as D
    for packed, out, _, plain in tracked:
        for rows in (out, plain):
            got = D.dedup_tracks(packed, [rows], [{}, {'min_frames': [0, 0, 0, 0], 'dup_iou': 0.0, 'dup_frac': 0.0}])
            for g in got:
                for name in COLUMNS:
                    assert g[name].dtype == rows[name].dtype and g[name].tobytes() == rows[name].tobytes(), name
                assert g['dropped'] == [] and not g['n_dropped'].any() and (g['keep'] == 1).all() and (g['by'] == -1).all() and (g['match'] == 0).all()
                assert g['row_keep'].dtype == np.int32 and (g['row_keep'] == 1).all() and g['n_dropped'].dtype == np.int64
        assert D.dedup_one(packed, plain, [0]) is plain
    assert len(tracked[0][3]['frame']) > 300


def test_settings_on_the_tracked_sequences_equal_the_reference(tracked, tracked_refs):
    from waymo_2d_tracking_amd.tracking import dedup as D
    for (packed, out, copies, _), refs in zip(tracked, tracked_refs):
        for g, ref in zip(D.dedup_tracks(packed, [out], JOBS), refs):
            assert_same(g, ref, out)
        dropped = [sum(ref['n_dropped']) for ref in refs]
        print('copies %d, dropped per job %s' % (copies, dropped))
        assert copies >= 1 and dropped[0] >= copies                      # of every injected pair at least one goes, by construction
    dropped = [sum(ref['n_dropped']) for ref in tracked_refs[0]]
    assert tracked[0][2] >= 5 and 0 <= dropped[3] < dropped[0] and dropped[3] <= dropped[2] <= dropped[0]


def test_jobs_over_results_in_one_call_equal_single_calls_and_dev_equals_host(tracked, tracked_refs):
    packed, out, _, plain = tracked[0]
    outs = [out, plain]                                                  # a second result over the same slots: without the copies
    plain_refs = [dedup_ref.dedup(packed['stream_frame_offsets'], plain, j) for j in JOBS]
    pairs = [(1, 0), (0, 1), (1, 3), (0, 2), (1, 1), (0, 0)]             # (result, job): results interleaved
    dev, jobs, from_dev = H.check_jobs_over_results(STAGE, packed, outs, [tracked_refs[0], plain_refs], JOBS, pairs)
    # the entries of the result a job does not name are -1
    p = dev.p
    grid = dict((k, dev.out[k].cpu().numpy().reshape(len(jobs), -1)) for k in ('keep', 'by', 'match', 'row_keep'))
    split, rows = int(p['traj_offsets'][p['n_streams']]), int(p['set_row_offsets'][1])
    for k in ('keep', 'by', 'match'):
        assert (grid[k][0, :split] == -1).all() and (grid[k][1, split:] == -1).all()
    assert (grid['keep'][0, split:] >= 0).all() and (grid['keep'][1, :split] >= 0).all()
    assert (grid['row_keep'][0, :rows] == -1).all() and (grid['row_keep'][0, rows:] >= 0).all() and (grid['row_keep'][1, rows:] == -1).all()
    H.check_relaunch_and_short_workspace(STAGE, dev, from_dev, packed, outs, jobs, lambda a, b: all(
        np.array_equal(a[k], b[k]) for k in ('object_id', 'keep', 'by', 'match', 'row_keep', 'n_dropped')) and a['dropped'] == b['dropped'])


def test_shuffled_input_gives_the_same_decision_per_row(tracked, tracked_refs):
    def per_row(g, ref, perm):
        # every row gets the decision it gets in the unshuffled input, in the caller's order
        assert g['row_keep'].tolist() == [ref['row_keep'][i] for i in perm]
    H.check_shuffled(STAGE, tracked[0][0], tracked[0][1], JOBS[1:3], tracked_refs[0][1:3], per_row)


@pytest.mark.parametrize('above', [0, 1], ids=['tables_in_lds', 'tables_in_workspace'])
def test_trajectory_counts_on_either_side_of_the_lds_limit(above):
    H.check_either_side_of_the_lds_limit(STAGE, above)


def test_same_local_index_in_two_jobs_does_not_interfere():
    """two results whose trajectories have the same local indices, deduplicated by three jobs in one call: each keeps its own state"""
    from waymo_2d_tracking_amd.tracking import dedup as D
    a = dedup_cases.result(dedup_cases.by_slot(dedup_cases.track(1, range(4), 0.0) + dedup_cases.track(2, range(4), 1.0)))
    b = dedup_cases.result(dedup_cases.by_slot(dedup_cases.track(1, range(4), 0.0) + dedup_cases.track(2, range(4), 5.0)))
    jobs = [dict(dedup_cases.job(min_frames=3), result=0), dict(dedup_cases.job(min_frames=3), result=1), dict(dedup_cases.job(min_frames=3, dup_iou=0.3), result=1)]
    got = D.dedup_tracks(packed_for([0, 5]), [arrays(a), arrays(b)], jobs)
    refs = [dedup_ref.dedup([0, 5], r, j) for r, j in ((a, jobs[0]), (b, jobs[1]), (b, jobs[2]))]
    assert [r['keep'] for r in refs] == [[1, 0], [1, 1], [1, 0]]
    for g, ref, out in zip(got, refs, (a, b, b)):
        assert_same(g, ref, arrays(out))


def test_invalid_input_is_refused():
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import dedup as D
    rows = [(0, 1, [0, 0, 5, 5], 0.5, 1), (3, 1, [0, 0, 5, 5], 0.5, 2), (4, 1, [0, 0, 5, 5], 0.5, 3), (4, 1, [9, 9, 5, 5], 0.5, 2), (4, 1, [1, 1, 5, 5], 0.5, 3)]
    packed = packed_for([0, 3, 6])
    with pytest.raises(_lib.WaymoTrackError, match=r'wt_dedup_tracks failed: WT_ERR_INVALID \(result 0: object_id 3 occurs twice in image seg1/15/FRONT\)'):
        D.dedup_tracks(packed, [arrays(dedup_cases.result(rows))], [dedup_cases.job(min_frames=1)])
    out = arrays(dedup_cases.result(rows[:4]))
    with pytest.raises(ValueError, match='dup_iou must not be NaN'):
        D.dedup_tracks(packed, [out], [{'min_frames': 1, 'dup_iou': float('nan')}])
    with pytest.raises(ValueError, match='min_frames must be >= 0'):
        D.dedup_tracks(packed, [out], [{'min_frames': [1, -1, 1, 1]}])
    with pytest.raises(ValueError, match=r'dup_frac must be in 0\.\.1'):
        D.dedup_tracks(packed, [out], [{'min_frames': 1, 'dup_frac': 1.25}])
    bad = dict(out, score=np.asarray([0.5, np.inf, 0.5, 0.5]))
    with pytest.raises(_lib.WaymoTrackError, match=r'WT_ERR_INVALID.*result 0, row 1: score is not finite'):
        D.dedup_tracks(packed, [bad], [dedup_cases.job(min_frames=1)])
    # the C entry point on its own: the same layout with the errors written into the arrays
    p = D._prepare(packed, [out], [dedup_cases.job(min_frames=1)], 4)
    o = [np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32), np.zeros((1, 4), np.int32), np.zeros((1, 2), np.int64)]
    last = lambda: _lib.lib().wt_last_error()
    # trajectories 0 and 1 of stream 1 meet in slot 4 only, apart: everything is kept
    assert D._host_call(p, o) == 0 and o[4].tolist() == [[0, 0]] and o[0].tolist() == [[1, 1, 1]] and o[1].tolist() == [[-1, -1, -1]] and o[3].tolist() == [[1, 1, 1, 1]]
    p['job_dup_iou'][0, 2] = np.nan
    assert D._host_call(p, o) == 1 and b'dup_iou of class 3 is NaN' in last()
    p['job_dup_iou'][0, 2] = 0.7
    p['job_min_frames'][0, 1] = -1
    assert D._host_call(p, o) == 1 and b'min_frames of class 2 is negative' in last()
    p['job_min_frames'][0, 1] = 1
    p['job_dup_frac'][0, 0] = 1.5
    assert D._host_call(p, o) == 1 and b'dup_frac of class 1 is outside 0..1' in last()
    p['job_dup_frac'][0, 0] = 0.5
    p['score'][2] = np.nan
    assert D._host_call(p, o) == 1 and b'result 0, row 2: score is not finite' in last()
    p['score'][2] = 0.5
    p['local'][3] = p['local'][2]
    assert D._host_call(p, o) == 1 and b'occurs twice in frame 4' in last()
    p['local'][3] = 0
    assert D._host_call(p, o) == 0


def gt_box(o, f):
    return [100.0 + 30.0 * (o - 1) + 8.0 * f, 50.0 + 4.0 * f, 70.0, 30.0]


def test_dedup_removes_the_false_positives_of_a_duplicate_track():
    """Object 1 over ten slots, track 11 on its boxes, track 12 on six of the slots with the box 5 px to the right (65 / 75 with track
    11); object 2 stands 30 px beside object 1 (40 / 100 = 0.4), track 21 on it.  Track 12 is six false positives; the pass drops it
    and nothing else."""
    from waymo_2d_tracking_amd.tracking import dedup as D, evaluate as E
    anns = [{'image_id': 'seg0/%d/FRONT' % (f * 10 + 5), 'bbox': gt_box(o, f), 'category_id': 1, 'object_id': 'g%d' % o} for f in range(10) for o in (1, 2)]
    rows = [(f, 1, gt_box(1, f), 0.9, 11) for f in range(10)] + [(f, 1, gt_box(2, f), 0.8, 21) for f in range(10)]
    shifted = lambda f: [gt_box(1, f)[0] + 5.0] + gt_box(1, f)[1:]
    rows += [(f, 1, shifted(f), 0.6, 12) for f in range(2, 8)]
    rows.sort(key=lambda r: r[0])
    packed, out = packed_for([0, 10]), arrays(dedup_cases.result(rows))
    assert dedup_ref.iou_dd([0.0, 0.0, 70.0, 30.0], [30.0, 0.0, 100.0, 30.0]) == 0.4
    job = dedup_cases.job(min_frames=3, dup_iou=0.7, dup_frac=0.5)
    got = D.dedup_tracks(packed, [out], [job])[0]
    assert_same(got, dedup_ref.dedup([0, 10], out, job), out)
    assert got['dropped'] == [(12, 11, 6)] and sorted(set(got['object_id'].tolist())) == [11, 21]
    gt = E.load_ground_truth(anns)
    tracks = [E.tracks_from_packed(packed, r) for r in (out, got)]
    mot = E.evaluate_tracks(gt, tracks)
    ident = E.evaluate_identity(gt, tracks)
    row = lambda k: tuple(mot[k].table[1][2][f] for f in ('gt', 'tp', 'fn', 'fp', 'idsw'))
    assert row(0) == (20, 20, 0, 6, 0) and row(1) == (20, 20, 0, 0, 0)
    assert ident[0].table[1][2]['idf1'] == 2 * 20 / (20 + 26) and ident[1].table[1][2]['idf1'] == 1.0
    neighbour = lambda r: [(int(f), b.tobytes()) for f, b, i in zip(r['frame'], r['bbox'], r['object_id']) if i == 21]
    assert neighbour(got) == neighbour(out) and len(neighbour(got)) == 10


def test_stitch_then_dedup_then_refine():
    """Track 30 sits on slots 2..7.  A second track on the same object is broken into 21 (slots 0..3) and 22 (slots 6..9).  Piece by
    piece it meets track 30 in two of four rows - no duplicate at dup_frac 0.6; stitched it has eight rows and meets the six of
    track 30 in four - 4 >= 0.6 * 6: a duplicate, and the longer one stays.  Refinement then fills the survivor's hole."""
    from waymo_2d_tracking_amd.tracking import dedup as D, refine as R, stitch as S
    box = lambda dx: [100.0 + dx, 50.0, 70.0, 30.0]
    rows = [(f, 1, box(0.0), 0.9, 30) for f in range(2, 8)] + [(f, 1, box(5.0), 0.8, 21) for f in range(4)] + [(f, 1, box(5.0), 0.8, 22) for f in range(6, 10)]
    rows.sort(key=lambda r: r[0])
    offsets, packed, out = [0, 10], packed_for([0, 10]), arrays(dedup_cases.result(rows))
    link, dup, fill = stitch_cases.job(max_link=3, link_iou=0.3), dedup_cases.job(min_frames=2, dup_iou=0.7, dup_frac=0.6), refine_cases.job(max_gap=2, min_len=1)
    alone = D.dedup_tracks(packed, [out], [dup])[0]
    assert_same(alone, dedup_ref.dedup(offsets, out, dup), out)
    assert alone['dropped'] == [] and len(alone['frame']) == 14
    stitched = S.stitch_tracks(packed, [out], [link])[0]                  # taken as it is, extras and all
    s_ref = stitch_ref.stitch(offsets, out, link)
    s_rows = dict(out, object_id=np.asarray(s_ref['object_id'], np.int64))
    assert [int(v) for v in stitched['object_id']] == s_ref['object_id'] and s_ref['links'] == [(21, 22, 3, 1.0)]
    deduped = D.dedup_tracks(packed, [stitched], [dup])[0]
    d_ref = dedup_ref.dedup(offsets, s_rows, dup)
    assert_same(deduped, d_ref, s_rows)
    assert deduped['dropped'] == [(30, 21, 4)] and deduped['object_id'].tolist() == [21] * 8
    refined = R.refine_tracks(packed, [deduped], [fill])[0]
    r_ref = refine_ref.refine(offsets, arrays(d_ref), fill)
    assert refined['frame'].tolist() == r_ref['frame'] == list(range(10)) and [int(v) for v in refined['object_id']] == r_ref['object_id']
    assert refined['bbox'].tobytes() == np.asarray(r_ref['bbox'], np.float64).tobytes()


def duplicated_detections(dets, every=2, shift=3.0, factor=0.9):
    """a second, lower-scored detection for every `every`-th wide enough box of classes 1 and 2, `shift` px to the right"""
    extra, n = [], 0
    for e in dets:
        if e['category_id'] in (1, 2) and e['bbox'][2] >= 20:
            n += 1
            if n % every == 0:
                extra.append(dict(e, bbox=[e['bbox'][0] + shift] + list(e['bbox'][1:]), score=e.get('score', 1.0) * factor))
    return list(dets) + extra


@pytest.mark.parametrize('fixture,cfg', [('sort_g5_input.json', G5), ('sort_g4_input.json', G4)])
def test_cli_writes_the_deduplicated_file(golden_dir, tmp_path, fixture, cfg):
    from waymo_2d_tracking_amd.tracking import track, utils as T
    raw = json.load(open(os.path.join(golden_dir, fixture)))
    raw = raw['annotations'] if 'annotations' in raw else raw
    path = str(tmp_path / 'det.json')
    with open(path, 'wt') as fp:
        json.dump(duplicated_detections(raw), fp)
    base = ['--input', path, '--max-age=2', '--score-threshold=' + ','.join(map(str, cfg['score']))]
    runs = [(['--dedup-frames', '3', '--dedup-iou', '0.5'], {'dedup': dedup_cases.job(min_frames=3, dup_iou=0.5)}),
            (['--link-gap=4', '--link-iou=0.2', '--dedup-frames=2,2,0,3', '--dedup-iou=0.6', '--dedup-frac=0.75,0.5,0.5,0.5', '--interpolate-gap=2',
              '--min-track-len=3'],
             {'stitch': stitch_cases.job(max_link=4, link_iou=0.2), 'dedup': dedup_cases.job(min_frames=[2, 2, 0, 3], dup_iou=0.6, dup_frac=[0.75, 0.5, 0.5, 0.5]),
              'refine': refine_cases.job(max_gap=2, min_len=3)})]
    for k, (flags, passes) in enumerate(runs):
        expected, refs, tracker_rows, _ = H._expected_file(path, cfg['score'], cfg['iou'], 2, passes)
        ref, n_tracked = refs['dedup'], len(tracker_rows['frame'])
        print('%s run %d: %d tracked rows, %d tracks dropped' % (fixture, k, n_tracked, sum(ref['n_dropped'])))
        if 'g4' in fixture:
            assert sum(ref['n_dropped']) >= 1 and len(ref['frame']) < n_tracked              # the flags are live on this input
        for name, extra in (('native%d.json' % k, []), ('python%d.json' % k, ['--python-io'])):
            T.reset_global_ids(0)
            assert track.main(base + flags + ['--output', str(tmp_path / name)] + extra) == 0
        assert (tmp_path / ('python%d.json' % k)).read_text() == json.dumps(expected)
        assert (tmp_path / ('native%d.json' % k)).read_bytes() == (tmp_path / ('python%d.json' % k)).read_bytes()


def test_cli_default_flags_write_what_they_wrote(golden_dir, tmp_path):
    from waymo_2d_tracking_amd.tracking import track
    H.check_cli_default_flags(golden_dir, tmp_path, (['--dedup-frames=0', '--dedup-iou=0.1', '--dedup-frac=0.0'], ['--dedup-frames=0,0,0,0', '--python-io']))
    args = track.build_parser().parse_args([])
    assert args.dedup_frames == [0] and args.dedup_iou == [0.7] and args.dedup_frac == [0.5] and not track.dedups(args)


@pytest.fixture(scope='module')
def sweep_set(tmp_path_factory):
    """synthetic detections with a second, lower-scored detection 3 px beside every second wide box of classes 1 and 2"""
    return H.sweep_set(tmp_path_factory, 'dedup_sweep', edit=lambda dets: duplicated_detections(dets, every=2, shift=3.0, factor=0.95))


def test_sweep_with_dedup_grids_equals_the_references(sweep_set):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    path, dets, gt_json = sweep_set
    grid = {'score': [0.3, 0.6], 'iou': [0.01], 'max_age': [1, 2], 'min_hits': [0], 'link_gap': [0, 3], 'link_iou': [0.3], 'dedup_frames': [0, 3],
            'dedup_iou': [0.5, 0.7], 'dedup_frac': 0.5, 'gap': [0, 2], 'min_len': [1]}
    res = E.sweep(path, E.load_ground_truth(gt_json), grid, identity=True, hota=True)
    assert len(res['settings']) == 64
    assert res['settings'][13] == {'max_age': 1, 'min_hits': 0, 'score': 0.3, 'iou': 0.01, 'link_gap': 3, 'link_iou': 0.3, 'dedup_frames': 3, 'dedup_iou': 0.5,
                                   'interp_gap': 2, 'min_len': 1}
    reference = H.sweep_reference(dets, gt_json, lambda s: {
        'stitch': stitch_cases.job(max_link=s['link_gap'], link_iou=s['link_iou']),
        'dedup': dedup_cases.job(min_frames=s['dedup_frames'], dup_iou=s['dedup_iou'], dup_frac=0.5),
        'refine': refine_cases.job(max_gap=s['interp_gap'], min_len=s['min_len'])})
    fps = {}
    same = lambda a, b: a == b or (a != a and b != b)
    for k, s in enumerate(res['settings']):
        mot, ident, hota = reference(s)
        # counts equal, sums and table within the bound of their addition order (the module text of mot_support.py)
        assert_hota_equals_reference(res['hota_results'][k], hota)
        for c in E.ALL_CLASSES:
            assert [res['results'][k].table[c][2][f] for f in mot_ref.FIELDS] == [mot[c][2][f] for f in mot_ref.FIELDS], (k, c)
            assert res['id_results'][k].table[c][2]['idtp'] == ident[c][2]['idtp'] and same(res['id_results'][k].table[c][2]['idf1'], ident[c][2]['idf1'])
        fps[(s['max_age'], s['score'], s['link_gap'], s['dedup_frames'], s['dedup_iou'], s['interp_gap'])] = mot['ALL'][2]['fp']
    print('ALL fp without / with the pass:', fps[(2, 0.3, 0, 0, 0.5, 0)], fps[(2, 0.3, 0, 3, 0.5, 0)])
    assert fps[(2, 0.3, 0, 3, 0.5, 0)] < fps[(2, 0.3, 0, 0, 0.5, 0)]                      # the loosest live setting drops false positives: the axes are live
    for lv in (1, 2):
        assert len(res['ranked'][lv]) == 2
        for row in res['ranked'][lv]:
            total = dict((f, 0) for f in mot_ref.FIELDS)
            for c in E.ALL_CLASSES:
                i = c - 1
                s = {'max_age': row['max_age'], 'min_hits': row['min_hits'], 'score': row['score_threshold'][i], 'iou': row['iou_threshold'][i],
                     'link_gap': row['link_gap'][i], 'link_iou': row['link_iou'][i], 'dedup_frames': row['dedup_frames'][i], 'dedup_iou': row['dedup_iou'][i],
                     'interp_gap': row['interp_gap'][i], 'min_len': row['min_len'][i]}
                for f in mot_ref.FIELDS:
                    total[f] += reference(s)[0][c][lv][f]
            assert row['counts'] == total, (lv, row)
            assert row['dedup_frames'][2] == 0 and row['dedup_frac'] == 0.5
            assert ' --dedup-frames=%s --dedup-iou=%s --dedup-frac=0.5 --interpolate-gap=' % (
                ','.join(map(str, row['dedup_frames'])), ','.join(repr(float(v)) for v in row['dedup_iou'])) in E.flag_line(row)


def test_sweep_with_default_dedup_grids_is_the_sweep_without_them(sweep_set):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    path, _, gt_json = sweep_set
    gt = E.load_ground_truth(gt_json)
    for grid in ({'score': [0.3, 0.6], 'iou': [0.01, 0.1], 'max_age': [1, 3], 'min_hits': [0, 1]},
                 {'score': [0.3], 'iou': [0.01], 'max_age': [1, 3], 'min_hits': [0], 'gap': [0, 1], 'min_len': [1, 2], 'link_gap': [0, 2]}):
        old = E.sweep(path, gt, grid)                                   # no dedup axes: the code path before them
        new = E.sweep(path, gt, dict(grid, dedup_frames=[0], dedup_iou=[0.3, 0.7], dedup_frac=0.9))
        for key in ('settings', 'ranked', 'best'):
            assert json.dumps(old[key], sort_keys=True) == json.dumps(new[key], sort_keys=True)
        assert sorted(old) == sorted(new) and 'dedup_frames' not in old['settings'][0] and 'dedup_frames' not in old['best'][2]
        assert 'dedup' not in E.flag_line(new['best'][2]) and E.flag_line(new['best'][2]) == E.flag_line(old['best'][2])
    args = E.build_parser().parse_args(['--annotations', 'x'])
    assert args.dedup_frames_grid == '0' and args.dedup_iou_grid == '0.7' and args.dedup_frac == 0.5
