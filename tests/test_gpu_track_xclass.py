"""HIP cross-class track suppression (csrc/track_xclass.hip through tracking/xclass.py) against the plain-Python restatement
tests/xclass_ref.py: keep, by, match, the row mask, the counts and the surviving rows must be EQUAL bit for bit - no float is
produced, rows are only selected; the operation order of the measures, the one multiplication of the fraction test and the strict
strength order are part of the definition.  The comparator and the bodies shared with the other
post-passes are in tests/track_stage_support.py."""
import json
import os

import numpy as np
import pytest

import dedup_cases
import dedup_ref
import refine_cases
import refine_ref
import stitch_cases
import stitch_ref
import track_stage_support as H
import xclass_cases
import xclass_ref
from track_stage_support import COLUMNS, G4, G5, arrays, packed_for

pytestmark = pytest.mark.gpu

STAGE = H.STAGES['xclass']
assert_same = STAGE.assert_same
NC = xclass_cases.N_CLASSES
EVERY = lambda v: dict(((a, b), v) for a in range(1, NC + 1) for b in range(a + 1, NC + 1))
JOBS = [xclass_cases.job(EVERY((1, 0.9, 0.0))),                                               # the loosest: every injected copy is the same object
        xclass_cases.job({(2, 4): (3, 0.9, 0.5), (1, 4): (2, 0.45, 1.0), (1, 2): (1, 0.5, 0.25), (1, 1): (2, 0.7, 0.5)}, prio=[0, 1, 0, 2], measure='iou'),
        xclass_cases.job(EVERY((2, 0.7, 0.5)), prio=[3, 2, 1, 0]),
        xclass_cases.job(EVERY((4, 0.99, 1.0)), measure='iou')]                               # the strictest: IoU of a copy is 0.5
KEYS = ('keep', 'by', 'match', 'row_keep', 'n_dropped', 'traj_offsets')


def with_other_class_copies(packed, out):
    """Every third trajectory gets a copy on every second of its rows under a fresh object id and ANOTHER class: the middle half of
    the box in x - wholly inside it, IoMin 1 and IoU 0.5 with its original - and half the score.  Returns the rows (copies
    appended: not sorted by frame) and the number of copies."""
    frame, oid = np.asarray(out['frame']), np.asarray(out['object_id'])
    stream = np.searchsorted(packed['stream_frame_offsets'], frame, side='right') - 1
    seen, picked = {}, []
    for i in np.argsort(frame, kind='stable'):
        seen.setdefault((int(stream[i]), int(oid[i])), []).append(int(i))
    fresh = int(oid.max()) + 1 if oid.size else 0
    new_ids, new_cat = [], []
    for n, rows in enumerate(seen.values()):
        if n % 3 == 0:
            first = int(np.asarray(out['category'])[rows[0]])
            picked += rows[::2]
            new_ids += [fresh + n] * len(rows[::2])
            new_cat += [2 if first == 4 else 4 if first == 2 else 2 + 2 * (n % 2)] * len(rows[::2])
    picked = np.asarray(picked, np.int64)
    bbox = np.asarray(out['bbox'])[picked].copy()
    bbox[:, 0] += bbox[:, 2] * 0.25
    bbox[:, 2] *= 0.5
    copies = {'frame': frame[picked], 'category': np.asarray(new_cat, np.asarray(out['category']).dtype), 'bbox': bbox,
              'score': np.asarray(out['score'])[picked] * 0.5, 'object_id': np.asarray(new_ids, oid.dtype)}
    return dict((k, np.concatenate([np.asarray(out[k]), copies[k]])) for k in COLUMNS), len(set(new_ids))


@pytest.fixture(scope='module')
def tracked(golden_dir):
    """The two tracking fixtures tracked with max_age 2, with injected other-class copies: [(packed, out, copies, the tracker's own rows)], g4 first."""
    sets = []
    for packed, plain in H.tracked_fixtures(golden_dir):
        plain = dict((k, plain[k]) for k in COLUMNS)
        out, copies = with_other_class_copies(packed, plain)
        sets.append((packed, out, copies, plain))
    return sets


@pytest.fixture(scope='module')
def tracked_refs(tracked):
    return [[xclass_ref.xclass(packed['stream_frame_offsets'], out, j, NC) for j in JOBS] for packed, out, _, _ in tracked]


def on_the_device(offsets, result, jobs):
    """a case whose categories the Python layer refuses: prepared with class 1 everywhere, the case's own categories written into
    the device form's column"""
    import torch
    from waymo_2d_tracking_amd.tracking import xclass as X
    out = arrays(result)
    dev = X.DeviceXClass(packed_for(offsets), [dict(out, category=np.ones_like(out['category']))], jobs)
    assert (np.diff(out['frame']) >= 0).all()                                                # the rows are in slot order: the column is the case's
    dev.t['category'].copy_(torch.from_numpy(out['category']).to(dev.device))
    dev.outs = [out]
    dev.launch()
    return dev.results()


@pytest.mark.parametrize('name', sorted(xclass_cases.CASES))
def test_case_equals_reference(name):
    H.check_case(STAGE, name, run=on_the_device if name in xclass_cases.DEVICE_ONLY else None)


def test_diagonal_jobs_are_the_deduplication_on_the_device():
    """the reduction: diagonal pairs, equal priorities and the IoU give what wt_dedup_tracks_host gives, on every dedup case"""
    from waymo_2d_tracking_amd.tracking import dedup as D, xclass as X
    n_jobs = dropped = 0
    for name in sorted(dedup_cases.CASES):
        offsets, result, jobs, _ = dedup_cases.CASES[name]()
        out, packed = arrays(result), packed_for(offsets)
        want = D.dedup_tracks(packed, [out], jobs)
        got = X.xclass_tracks(packed, [out], [xclass_ref.from_dedup_job(j, NC) for j in jobs])
        for a, b in zip(got, want):
            for k in KEYS + ('object_id',):
                assert a[k].tolist() == b[k].tolist(), (name, k)
            assert a['dropped'] == b['dropped']
            n_jobs += 1
            dropped += len(a['dropped'])
    assert n_jobs == 27 and dropped > 40


def test_deep_chain_takes_one_round_per_link():
    from waymo_2d_tracking_amd.tracking import xclass as X
    offsets, result, jobs, _ = dedup_cases.deep_chain(40)
    result = dict(result, category=[1 + (oid % 2) * 3 for oid in result['object_id']])      # neighbours of the chain: classes 1 and 4 in turn
    job = xclass_cases.job({(1, 4): (3, 0.6, 0.5)}, measure='iou')
    dev = X.DeviceXClass(packed_for(offsets), [arrays(result)], [job])
    dev.launch()
    assert dev.rounds().tolist() == [[40]]
    ref = xclass_ref.xclass(offsets, result, job, NC)
    assert ref['keep'] == [1 - k % 2 for k in range(40)]
    assert_same(dev.results()[0], ref, arrays(result))


def test_all_pairs_off_reproduces_the_tracked_rows(tracked):
    from waymo_2d_tracking_amd.tracking import xclass as X
    for packed, out, _, plain in tracked:
        for rows in (out, plain):
            got = X.xclass_tracks(packed, [rows], [{}, {'pairs': {(2, 4): {'frames': 0, 'overlap': 0.0, 'frac': 0.0}}, 'prio': [3, 2, 1, 0], 'measure': 'iou'}])
            for g in got:
                for name in COLUMNS:
                    assert g[name].dtype == rows[name].dtype and g[name].tobytes() == rows[name].tobytes(), name
                assert g['dropped'] == [] and not g['n_dropped'].any() and (g['keep'] == 1).all() and (g['by'] == -1).all() and (g['match'] == 0).all()
                assert g['row_keep'].dtype == np.int32 and (g['row_keep'] == 1).all() and g['n_dropped'].dtype == np.int64
        assert X.xclass_one(packed, plain, {}) is plain
    assert len(tracked[0][3]['frame']) > 300


def test_settings_on_the_tracked_sequences_equal_the_reference(tracked, tracked_refs):
    from waymo_2d_tracking_amd.tracking import xclass as X
    for (packed, out, copies, _), refs in zip(tracked, tracked_refs):
        for g, ref in zip(X.xclass_tracks(packed, [out], JOBS), refs):
            assert_same(g, ref, out)
        dropped = [sum(ref['n_dropped']) for ref in refs]
        print('copies %d, dropped per job %s' % (copies, dropped))
        assert copies >= 1 and dropped[0] >= copies                      # of every injected pair at least one goes, by construction
    dropped = [sum(ref['n_dropped']) for ref in tracked_refs[0]]
    assert tracked[0][2] >= 5 and 0 <= dropped[3] < dropped[0] and dropped[1] >= 1 and dropped[2] >= 1


def test_jobs_over_results_in_one_call_equal_single_calls_and_dev_equals_host(tracked, tracked_refs):
    packed, out, _, plain = tracked[0]
    outs = [out, plain, plain]                                           # a second result over the same slots, and a third no job names
    plain_refs = [xclass_ref.xclass(packed['stream_frame_offsets'], plain, j, NC) for j in JOBS]
    pairs = [(1, 0), (0, 1), (1, 3), (0, 2), (1, 1), (0, 0)]             # (result, job): results interleaved
    dev, jobs, from_dev = H.check_jobs_over_results(STAGE, packed, outs, [tracked_refs[0], plain_refs], JOBS, pairs)
    # the entries of the results a job does not name are -1
    p = dev.p
    S = p['n_streams']
    grid = dict((k, dev.out[k].cpu().numpy().reshape(len(jobs), -1)) for k in ('keep', 'by', 'match', 'row_keep'))
    split, third = int(p['traj_offsets'][S]), int(p['traj_offsets'][2 * S])
    rows, rows2 = int(p['set_row_offsets'][1]), int(p['set_row_offsets'][2])
    for k in ('keep', 'by', 'match'):
        assert (grid[k][0, :split] == -1).all() and (grid[k][1, split:] == -1).all() and (grid[k][:, third:] == -1).all()
    assert (grid['keep'][0, split:third] >= 0).all() and (grid['keep'][1, :split] >= 0).all()
    assert (grid['row_keep'][0, :rows] == -1).all() and (grid['row_keep'][0, rows:rows2] >= 0).all() and (grid['row_keep'][1, rows:] == -1).all()
    assert (grid['row_keep'][:, rows2:] == -1).all() and third < p['n_traj_total']
    small = H.check_relaunch_and_short_workspace(STAGE, dev, from_dev, packed, outs, jobs, lambda a, b: all(
        np.array_equal(a[k], b[k]) for k in ('object_id', 'keep', 'by', 'match', 'row_keep', 'n_dropped')) and a['dropped'] == b['dropped'])
    assert (small.out['keep'].cpu().numpy() == 0).all()                  # as allocated: no kernel ran


def test_shuffled_input_gives_the_same_decision_per_row(tracked, tracked_refs):
    def per_row(g, ref, perm):
        # every row gets the decision it gets in the unshuffled input, in the caller's order
        assert g['row_keep'].tolist() == [ref['row_keep'][i] for i in perm]
    H.check_shuffled(STAGE, tracked[0][0], tracked[0][1], JOBS[1:3], tracked_refs[0][1:3], per_row)


@pytest.mark.parametrize('above', [0, 1], ids=['tables_in_lds', 'tables_in_workspace'])
def test_trajectory_counts_on_either_side_of_the_lds_limit(above):
    assert H.lds_limit('xclass') == 1024
    H.check_either_side_of_the_lds_limit(STAGE, above)


def test_xclass_removes_the_false_positives_of_the_rider_track():
    """case 1 against a ground truth that holds the cyclist only: the pedestrian track on the rider is eight false positives of
    class 2; the pass removes them and the counts of class 4 do not change"""
    from waymo_2d_tracking_amd.tracking import evaluate as E, xclass as X
    offsets, result, jobs, _ = xclass_cases.rider_in_cyclist()
    packed, out = packed_for(offsets), arrays(result)
    anns = [{'image_id': 'seg0/%d/FRONT' % (f * 10 + 5), 'bbox': [0.0, 0.0, 10.0, 15.0], 'category_id': 4, 'object_id': 'g1'} for f in range(10)]
    got = X.xclass_tracks(packed, [out], jobs[:1])[0]
    assert_same(got, xclass_ref.xclass(offsets, result, jobs[0], NC), out)
    gt = E.load_ground_truth(anns)
    mot = E.evaluate_tracks(gt, [E.tracks_from_packed(packed, r) for r in (out, got)])
    row = lambda k, c: tuple(mot[k].table[c][2][f] for f in ('gt', 'tp', 'fn', 'fp', 'idsw'))
    assert row(0, 2) == (0, 0, 0, 8, 0) and row(1, 2) == (0, 0, 0, 0, 0)
    assert row(0, 4) == row(1, 4) == (10, 10, 0, 0, 0)
    assert row(0, 'ALL')[3] == 8 and row(1, 'ALL')[3] == 0


def test_stitch_then_dedup_then_xclass_then_refine():
    """A cyclist track 30 on slots 2..7.  A pedestrian track on its rider is broken into 21 (slots 0..3) and 22 (slots 6..9), and a
    second pedestrian track 23 lies on 21 in slots 0..2.  Piece by piece the pedestrian meets the cyclist in two slots - not the
    same object at frames 3; stitched it has eight rows and meets it in four, and the cyclist, the shorter, goes.  Deduplication
    removes 23 before the pass sees it; refinement then fills the survivor's hole.  track.refined runs the passes in that order."""
    from waymo_2d_tracking_amd.tracking import track, xclass as X
    cyc, ped = [100.0, 50.0, 70.0, 90.0], [110.0, 50.0, 40.0, 60.0]
    rows = [(f, 4, cyc, 0.9, 30) for f in range(2, 8)] + [(f, 2, ped, 0.8, 21) for f in range(4)] + [(f, 2, ped, 0.8, 22) for f in range(6, 10)]
    rows += [(f, 2, [ped[0] + 1.0] + ped[1:], 0.5, 23) for f in range(3)]
    rows.sort(key=lambda r: r[0])
    offsets, packed, out = [0, 10], packed_for([0, 10]), arrays(dedup_cases.result(rows))
    xjob = xclass_cases.job({(2, 4): (3, 0.9, 0.5)})
    alone = X.xclass_tracks(packed, [out], [xjob])[0]
    assert_same(alone, xclass_ref.xclass(offsets, out, xjob, NC), out)
    assert alone['dropped'] == []
    args = track.build_parser().parse_args(['--link-gap=3', '--link-iou=0.3', '--dedup-frames=2', '--dedup-iou=0.7', '--dedup-frac=0.6',
                                            '--xclass-pairs=2:4', '--xclass-overlap=0.9', '--interpolate-gap=2'])
    got = track.refined(args, packed, out)
    s_ref = stitch_ref.stitch(offsets, out, stitch_cases.job(max_link=3, link_iou=0.3))
    assert s_ref['links'] == [(21, 22, 3, 1.0)]
    d_ref = dedup_ref.dedup(offsets, dict(out, object_id=np.asarray(s_ref['object_id'], np.int64)), dedup_cases.job(min_frames=2, dup_iou=0.7, dup_frac=0.6))
    assert d_ref['dropped'] == [(23, 21, 3)]
    x_ref = xclass_ref.xclass(offsets, arrays(d_ref), xjob, NC)
    assert x_ref['dropped'] == [(30, 21, 4)]
    r_ref = refine_ref.refine(offsets, arrays(x_ref), refine_cases.job(max_gap=2, min_len=1))
    assert got['frame'].tolist() == r_ref['frame'] == list(range(10)) and [int(v) for v in got['object_id']] == r_ref['object_id'] == [21] * 10
    assert got['bbox'].tobytes() == np.asarray(r_ref['bbox'], np.float64).tobytes() and got['category'].tolist() == [2] * 10


def cross_class_detections(dets, every=2, factor=0.95):
    """a second, lower-scored detection of ANOTHER class inside every `every`-th wide enough box of classes 1 and 2: a cyclist box on
    a pedestrian, a pedestrian box on a vehicle"""
    extra, n = [], 0
    for e in dets:
        if e['category_id'] in (1, 2) and e['bbox'][2] >= 20:
            n += 1
            if n % every == 0:
                x, y, w, h = e['bbox']
                extra.append(dict(e, bbox=[x + w * 0.25, y, w * 0.5, h], category_id=4 if e['category_id'] == 2 else 2, score=e.get('score', 1.0) * factor))
    return list(dets) + extra


@pytest.mark.parametrize('fixture,cfg', [('sort_g5_input.json', G5), ('sort_g4_input.json', G4)])
def test_cli_writes_the_file_on_both_io_paths(golden_dir, tmp_path, fixture, cfg):
    from waymo_2d_tracking_amd.tracking import track, utils as T
    raw = json.load(open(os.path.join(golden_dir, fixture)))
    raw = raw['annotations'] if 'annotations' in raw else raw
    path = str(tmp_path / 'det.json')
    with open(path, 'wt') as fp:
        json.dump(cross_class_detections(raw), fp)
    base = ['--input', path, '--max-age=2', '--score-threshold=' + ','.join(map(str, cfg['score']))]
    runs = [(['--xclass-pairs', '2:4,1:2', '--xclass-frames', '2'], {'xclass': xclass_cases.job({(2, 4): (2, 0.7, 0.5), (1, 2): (2, 0.7, 0.5)})}),
            (['--link-gap=4', '--link-iou=0.2', '--dedup-frames=2,2,0,3', '--dedup-iou=0.6', '--xclass-pairs=1:2,2:4', '--xclass-frames=3,2',
              '--xclass-overlap=0.45,0.9', '--xclass-frac=0.25', '--xclass-measure=iou', '--xclass-prio=1,0,0,2', '--interpolate-gap=2', '--min-track-len=3'],
             {'stitch': stitch_cases.job(max_link=4, link_iou=0.2), 'dedup': dedup_cases.job(min_frames=[2, 2, 0, 3], dup_iou=0.6),
              'xclass': xclass_cases.job({(1, 2): (3, 0.45, 0.25), (2, 4): (2, 0.9, 0.25)}, prio=[1, 0, 0, 2], measure='iou'),
              'refine': refine_cases.job(max_gap=2, min_len=3)})]
    for k, (flags, passes) in enumerate(runs):
        expected, refs, tracker_rows, _ = H._expected_file(path, cfg['score'], cfg['iou'], 2, passes)
        ref = refs['xclass']
        print('%s run %d: %d tracked rows, %d tracks dropped' % (fixture, k, len(tracker_rows['frame']), sum(ref['n_dropped'])))
        if 'g4' in fixture:
            assert sum(ref['n_dropped']) >= 1                                                 # the flags are live on this input
        for name, extra in (('native%d.json' % k, []), ('python%d.json' % k, ['--python-io'])):
            T.reset_global_ids(0)
            assert track.main(base + flags + ['--output', str(tmp_path / name)] + extra) == 0
        assert (tmp_path / ('python%d.json' % k)).read_text() == json.dumps(expected)
        assert (tmp_path / ('native%d.json' % k)).read_bytes() == (tmp_path / ('python%d.json' % k)).read_bytes()


def test_cli_default_flags_write_what_they_wrote_without_the_module(golden_dir, tmp_path):
    H.check_cli_default_flags(golden_dir, tmp_path, (['--xclass-frames=5', '--xclass-overlap=0.1', '--xclass-prio=0,0,0,1'],
                                                     ['--xclass-pairs=2:4', '--xclass-frames=0', '--python-io']),
                              module='waymo_2d_tracking_amd.tracking.xclass')
