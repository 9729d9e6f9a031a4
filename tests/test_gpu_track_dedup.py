"""HIP track deduplication (csrc/track_dedup.hip through tracking/dedup.py) against the plain-Python restatement
tests/dedup_ref.py: keep, by, match, the row mask, the counts and the surviving rows must be EQUAL bit for bit - no float is
produced, rows are only selected; the operation order of the IoU, the one multiplication of the fraction test and the strict
strength order are part of the definition."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dedup_cases
import dedup_ref
import hota_ref
import mot_id_ref
import mot_ref
import refine_cases
import refine_ref
import stitch_cases
import stitch_ref
from test_gpu_mot_hota import assert_equals_reference as assert_hota_equals_reference

pytestmark = pytest.mark.gpu

JOBS = [dedup_cases.job(min_frames=1, dup_iou=0.9, dup_frac=0.0),                             # the loosest: every injected copy is a duplicate
        dedup_cases.job(min_frames=[3, 2, 0, 1], dup_iou=[0.9, 0.5, 0.7, 0.8], dup_frac=[0.5, 1.0, 0.5, 0.25]),
        dedup_cases.job(min_frames=2, dup_iou=0.7, dup_frac=0.5),
        dedup_cases.job(min_frames=4, dup_iou=0.99, dup_frac=1.0)]                            # the strictest
G4 = dict(score=[0.3, 0.3, 1.0, 0.2], iou=[0.01, 0.01, 1.0, 0.0])
G5 = dict(score=[0.95, 0.6, 1.0, 0.9], iou=[0.01, 0.01, 1.0, 0.0])
COLUMNS = ('frame', 'category', 'bbox', 'score', 'object_id')


def packed_for(offsets):
    """the part of a packed detection set that the pass reads, for hand-made slots"""
    offsets = np.asarray(offsets, np.int64)
    n_streams = offsets.size - 1
    ids = np.concatenate([np.arange(offsets[s + 1] - offsets[s]) * 10 + 5 for s in range(n_streams)] + [np.zeros(0, np.int64)])
    return {'stream_frame_offsets': offsets, 'frame_ids': ids.astype(np.int64), 'stream_keys': [('seg%d' % s, 'FRONT') for s in range(n_streams)]}


def arrays(result):
    return {'frame': np.asarray(result['frame'], np.int64), 'category': np.asarray(result['category'], np.int32),
            'bbox': np.asarray(result['bbox'], np.float64).reshape(-1, 4), 'score': np.asarray(result['score'], np.float64),
            'object_id': np.asarray(result['object_id'], np.int64)}


def assert_same(got, ref, out):
    """got: a dict of tracking/dedup.py; ref: dedup_ref.dedup() of `out`"""
    assert got['keep'].tolist() == ref['keep'] and got['by'].tolist() == ref['by'] and got['match'].tolist() == ref['match']
    assert got['row_keep'].tolist() == ref['row_keep']
    assert got['n_dropped'].tolist() == ref['n_dropped'] and got['traj_offsets'].tolist() == ref['traj_offsets']
    assert [(int(a), int(b), m) for a, b, m in got['dropped']] == ref['dropped']
    mask = np.asarray(ref['row_keep'], bool)
    for name in COLUMNS:                                                  # the surviving rows, in the caller's order, with their input bits
        want = np.asarray(out[name])[mask]
        assert got[name].dtype == want.dtype and got[name].shape == want.shape and got[name].tobytes() == want.tobytes(), name
    assert [int(v) for v in got['frame']] == ref['frame'] and [int(v) for v in got['object_id']] == ref['object_id']
    assert got['bbox'].tobytes() == np.asarray(ref['bbox'], np.float64).reshape(-1, 4).tobytes()
    assert got['score'].tobytes() == np.asarray(ref['score'], np.float64).tobytes()


def rows_of(ref):
    """the surviving rows of a reference as the arrays the next pass and the writers take"""
    return arrays(ref)


def lds_limit():
    from waymo_2d_tracking_amd import _lib
    n = C.c_int32(0)
    _lib.lib().wt_dedup_tracks_limits(C.byref(n))
    return n.value


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
    from waymo_2d_tracking_amd.tracking import utils as T
    sets = []
    for name, cfg in (('sort_g4_input.json', G4), ('sort_g5_input.json', G5)):
        packed = T.pack_streams(T.read_data_file(os.path.join(golden_dir, name), cfg['score']))
        plain = T.track_packed(packed, cfg['iou'], 2, 0)[0]
        plain = dict((k, plain[k]) for k in COLUMNS)
        out, copies = with_copies(packed, plain)
        sets.append((packed, out, copies, plain))
    return sets


@pytest.fixture(scope='module')
def tracked_refs(tracked):
    return [[dedup_ref.dedup(packed['stream_frame_offsets'], out, j) for j in JOBS] for packed, out, _, _ in tracked]


@pytest.mark.parametrize('name', sorted(dedup_cases.CASES))
def test_case_equals_reference(name):
    from waymo_2d_tracking_amd.tracking import dedup as D
    offsets, result, jobs, claim = dedup_cases.CASES[name]()
    refs = [dedup_ref.dedup(offsets, result, j) for j in jobs]
    claim(refs)
    out = arrays(result)
    got = D.dedup_tracks(packed_for(offsets), [out], jobs)
    assert len(got) == len(refs)
    for g, ref in zip(got, refs):
        assert_same(g, ref, out)


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
    import torch
    from waymo_2d_tracking_amd.tracking import dedup as D
    packed, out, _, plain = tracked[0]
    outs = [out, plain]                                                  # a second result over the same slots: without the copies
    plain_refs = [dedup_ref.dedup(packed['stream_frame_offsets'], plain, j) for j in JOBS]
    refs = [tracked_refs[0], plain_refs]
    pairs = [(1, 0), (0, 1), (1, 3), (0, 2), (1, 1), (0, 0)]             # (result, job): results interleaved
    jobs = [dict(JOBS[j], result=r) for r, j in pairs]
    together = D.dedup_tracks(packed, outs, jobs)
    dev = D.DeviceDedup(packed, outs, jobs)
    dev.launch()
    from_dev = dev.results()
    for (r, j), a, b in zip(pairs, together, from_dev):
        alone = D.dedup_tracks(packed, [outs[r]], [JOBS[j]])[0]
        for got in (alone, a, b):
            assert_same(got, refs[r][j], outs[r])
    # the entries of the result a job does not name are -1
    p = dev.p
    grid = dict((k, dev.out[k].cpu().numpy().reshape(len(jobs), -1)) for k in ('keep', 'by', 'match', 'row_keep'))
    split, rows = int(p['traj_offsets'][p['n_streams']]), int(p['set_row_offsets'][1])
    for k in ('keep', 'by', 'match'):
        assert (grid[k][0, :split] == -1).all() and (grid[k][1, split:] == -1).all()
    assert (grid['keep'][0, split:] >= 0).all() and (grid['keep'][1, :split] >= 0).all()
    assert (grid['row_keep'][0, :rows] == -1).all() and (grid['row_keep'][0, rows:] >= 0).all() and (grid['row_keep'][1, rows:] == -1).all()
    # a second launch on the same buffers gives the same answer (the call initialises everything it reads)
    dev.launch()
    for a, b in zip(from_dev, dev.results()):
        assert all(np.array_equal(a[k], b[k]) for k in ('object_id', 'keep', 'by', 'match', 'row_keep', 'n_dropped')) and a['dropped'] == b['dropped']
    # a workspace one byte too small: WT_ERR_CAPACITY, nothing launched
    from waymo_2d_tracking_amd import _lib
    small = D.DeviceDedup(packed, outs, jobs, workspace_bytes=dev.ws_bytes - 1)
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY'):
        small.launch()
    torch.cuda.synchronize()


def test_shuffled_input_gives_the_same_decision_per_row(tracked, tracked_refs):
    from waymo_2d_tracking_amd.tracking import dedup as D
    packed, out, _, _ = tracked[0]
    perm = np.random.default_rng(4).permutation(len(out['frame']))
    shuffled = dict((k, v[perm]) for k, v in out.items())
    got = D.dedup_tracks(packed, [shuffled], JOBS[1:3])
    for g, j, ref in zip(got, JOBS[1:3], tracked_refs[0][1:3]):
        assert_same(g, dedup_ref.dedup(packed['stream_frame_offsets'], shuffled, j), shuffled)
        # every row gets the decision it gets in the unshuffled input, in the caller's order
        assert g['row_keep'].tolist() == [ref['row_keep'][i] for i in perm]


@pytest.mark.parametrize('above', [0, 1], ids=['tables_in_lds', 'tables_in_workspace'])
def test_trajectory_counts_on_either_side_of_the_lds_limit(above):
    from waymo_2d_tracking_amd.tracking import dedup as D
    limit = lds_limit()
    assert 64 < limit <= 4096
    offsets, result, jobs, claim = dedup_cases.many_trajectories(limit + above)
    refs = [dedup_ref.dedup(offsets, result, j) for j in jobs]
    claim(refs)
    out = arrays(result)
    p = D._prepare(packed_for(offsets), [out], jobs, 4)
    assert p['n_traj'].tolist() == [[limit + above]]
    for g, ref in zip(D.dedup_tracks(packed_for(offsets), [out], jobs), refs):
        assert_same(g, ref, out)
    dev = D.DeviceDedup(packed_for(offsets), [out], jobs)
    dev.launch()
    for g, ref in zip(dev.results(), refs):
        assert_same(g, ref, out)


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
    r_ref = refine_ref.refine(offsets, rows_of(d_ref), fill)
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


def _expected_file(path, score_thr, iou_thr, max_age, link, dup, refine):
    """what track.py has to write: the tracker's rows through the reference stitching, deduplication and refinement - each where its
    flags are given - and format_tracks"""
    from waymo_2d_tracking_amd.tracking import utils as T
    packed = T.pack_streams(T.read_data_file(path, score_thr))
    out, _ = T.track_packed(packed, iou_thr, max_age, 0)
    rows = dict((k, out[k]) for k in COLUMNS)
    if link is not None:
        rows = dict(rows, object_id=np.asarray(stitch_ref.stitch(packed['stream_frame_offsets'], rows, link)['object_id'], dtype=np.asarray(out['object_id']).dtype))
    ref = dedup_ref.dedup(packed['stream_frame_offsets'], rows, dup)
    rows = rows_of(ref)
    if refine is not None:
        rows = rows_of(refine_ref.refine(packed['stream_frame_offsets'], rows, refine))
    return T.format_tracks(packed, rows), ref, len(out['frame'])


@pytest.mark.parametrize('fixture,cfg', [('sort_g5_input.json', G5), ('sort_g4_input.json', G4)])
def test_cli_writes_the_deduplicated_file(golden_dir, tmp_path, fixture, cfg):
    from waymo_2d_tracking_amd.tracking import track, utils as T
    raw = json.load(open(os.path.join(golden_dir, fixture)))
    raw = raw['annotations'] if 'annotations' in raw else raw
    path = str(tmp_path / 'det.json')
    with open(path, 'wt') as fp:
        json.dump(duplicated_detections(raw), fp)
    base = ['--input', path, '--max-age=2', '--score-threshold=' + ','.join(map(str, cfg['score']))]
    runs = [(['--dedup-frames', '3', '--dedup-iou', '0.5'], None, dedup_cases.job(min_frames=3, dup_iou=0.5), None),
            (['--link-gap=4', '--link-iou=0.2', '--dedup-frames=2,2,0,3', '--dedup-iou=0.6', '--dedup-frac=0.75,0.5,0.5,0.5', '--interpolate-gap=2',
              '--min-track-len=3'], stitch_cases.job(max_link=4, link_iou=0.2),
             dedup_cases.job(min_frames=[2, 2, 0, 3], dup_iou=0.6, dup_frac=[0.75, 0.5, 0.5, 0.5]), refine_cases.job(max_gap=2, min_len=3))]
    for k, (flags, link, dup, refine) in enumerate(runs):
        expected, ref, n_tracked = _expected_file(path, cfg['score'], cfg['iou'], 2, link, dup, refine)
        print('%s run %d: %d tracked rows, %d tracks dropped' % (fixture, k, n_tracked, sum(ref['n_dropped'])))
        if 'g4' in fixture:
            assert sum(ref['n_dropped']) >= 1 and len(ref['frame']) < n_tracked              # the flags are live on this input
        for name, extra in (('native%d.json' % k, []), ('python%d.json' % k, ['--python-io'])):
            T.reset_global_ids(0)
            assert track.main(base + flags + ['--output', str(tmp_path / name)] + extra) == 0
        assert (tmp_path / ('python%d.json' % k)).read_text() == json.dumps(expected)
        assert (tmp_path / ('native%d.json' % k)).read_bytes() == (tmp_path / ('python%d.json' % k)).read_bytes()


def test_cli_default_flags_write_what_they_wrote(golden_dir, tmp_path):
    from waymo_2d_tracking_amd.tracking import track, utils as T
    for fixture, score in (('sort_g5_input.json', '0.95,0.6,1.0,0.9'), ('sort_g4_input.json', '0.3,0.3,1.0,0.2')):
        path = os.path.join(golden_dir, fixture)
        flags = ['--input', path, '--max-age=2', '--score-threshold=' + score]
        T.reset_global_ids(0)
        untouched = json.dumps(T.track_all(T.read_data_file(path, [float(v) for v in score.split(',')]), [0.01, 0.01, 1.0, 0.0], 2, 0))
        written = []
        for i, extra in enumerate(([], ['--python-io'], ['--dedup-frames=0', '--dedup-iou=0.1', '--dedup-frac=0.0'], ['--dedup-frames=0,0,0,0', '--python-io'])):
            T.reset_global_ids(0)
            assert track.main(flags + ['--output', str(tmp_path / ('t%d.json' % i))] + extra) == 0
            written.append((tmp_path / ('t%d.json' % i)).read_text())
        assert written[1] == untouched and written[0] == written[1] == written[2] == written[3]
    exp = json.load(open(os.path.join(golden_dir, 'sort_g4_expected_a.json')))['tracks']
    assert [(r['image_id'], r['category_id'], r['object_id']) for r in json.loads(written[0])] == [(r['image_id'], r['category_id'], r['object_id']) for r in exp]
    args = track.build_parser().parse_args([])
    assert args.dedup_frames == [0] and args.dedup_iou == [0.7] and args.dedup_frac == [0.5] and not track.dedups(args)


@pytest.fixture(scope='module')
def sweep_set(tmp_path_factory):
    """synthetic detections with a second, lower-scored detection 3 px beside every second wide box of classes 1 and 2"""
    from waymo_2d_tracking_amd import synthetic as syn
    dets, gt_json = syn.make_tracking_json(23, n_segments=1, n_frames=12, n_objects=12, cameras=('FRONT', 'SIDE_LEFT'))
    dets = duplicated_detections(dets, every=2, shift=3.0, factor=0.95)
    path = tmp_path_factory.mktemp('dedup_sweep') / 'det.json'
    path.write_text(json.dumps(dets))
    return str(path), dets, gt_json


def test_sweep_with_dedup_grids_equals_the_references(sweep_set):
    from waymo_2d_tracking_amd.tracking import evaluate as E, utils as T
    path, dets, gt_json = sweep_set
    grid = {'score': [0.3, 0.6], 'iou': [0.01], 'max_age': [1, 2], 'min_hits': [0], 'link_gap': [0, 3], 'link_iou': [0.3], 'dedup_frames': [0, 3],
            'dedup_iou': [0.5, 0.7], 'dedup_frac': 0.5, 'gap': [0, 2], 'min_len': [1]}
    res = E.sweep(path, E.load_ground_truth(gt_json), grid, identity=True, hota=True)
    assert len(res['settings']) == 64
    assert res['settings'][13] == {'max_age': 1, 'min_hits': 0, 'score': 0.3, 'iou': 0.01, 'link_gap': 3, 'link_iou': 0.3, 'dedup_frames': 3, 'dedup_iou': 0.5,
                                   'interp_gap': 2, 'min_len': 1}
    predictions = {}
    for e in dets:
        seg, fr, cam = e['image_id'].split('/')
        predictions.setdefault(seg, {}).setdefault(cam, {}).setdefault(int(fr), []).append(
            {'bbox': e['bbox'], 'score': e['score'], 'category_id': e['category_id']})
    packed = T.pack_streams(predictions)
    cache, tracked_cache = {}, {}

    def reference(s):
        key = tuple(sorted(s.items()))
        if key not in cache:
            tkey = (s['iou'], s['max_age'], s['min_hits'], s['score'])
            if tkey not in tracked_cache:
                tracked_cache[tkey] = T.track_packed(packed, [s['iou']] * 4, s['max_age'], s['min_hits'], [s['score']] * 4)[0]
            out = dict((k, tracked_cache[tkey][k]) for k in COLUMNS)
            linked = dict(out, object_id=np.asarray(stitch_ref.stitch(packed['stream_frame_offsets'], out, stitch_cases.job(max_link=s['link_gap'], link_iou=s['link_iou']))['object_id'], np.int64))
            kept = rows_of(dedup_ref.dedup(packed['stream_frame_offsets'], linked, dedup_cases.job(min_frames=s['dedup_frames'], dup_iou=s['dedup_iou'], dup_frac=0.5)))
            rows = json.loads(json.dumps(T.format_tracks(packed, rows_of(refine_ref.refine(packed['stream_frame_offsets'], kept, refine_cases.job(max_gap=s['interp_gap'], min_len=s['min_len']))))))
            cache[key] = (mot_ref.evaluate(gt_json, rows)['table'], mot_id_ref.evaluate(gt_json, rows)['table'], hota_ref.evaluate(gt_json, rows))
        return cache[key]
    fps = {}
    same = lambda a, b: a == b or (a != a and b != b)
    for k, s in enumerate(res['settings']):
        mot, ident, hota = reference(s)
        # counts equal, sums and table within the bound of their addition order (the module text of test_gpu_mot_hota.py)
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
