"""HIP track splitting (csrc/track_split.hip through tracking/split.py) against the plain-Python restatement tests/split_ref.py:
object ids, pieces, piece numbers, the tests of every pair, the breaks and the new pieces per stream must be EQUAL bit for bit (a
NaN test equals a NaN test) - the unfused extrapolations and the operation order of the IoU are part of the definition (DESIGN.md
section 25)."""
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
import smooth_cases
import smooth_ref
import split_cases
import split_ref
import stitch_cases
import stitch_ref
from test_gpu_mot_hota import assert_equals_reference as assert_hota_equals_reference

pytestmark = pytest.mark.gpu

JOBS = [split_cases.job(0.3), split_cases.job([0.5, 0.2, 0.0, 0.3], [0, 1, 1, 0]), split_cases.job(0.3, 1, motion='hold'),
        split_cases.job(0.0, 1, first_new_id=100000)]
G4 = dict(score=[0.3, 0.3, 1.0, 0.2], iou=[0.01, 0.01, 1.0, 0.0])
G5 = dict(score=[0.95, 0.6, 1.0, 0.9], iou=[0.01, 0.01, 1.0, 0.0])


def packed_for(offsets):
    """the part of a packed detection set that splitting reads, for hand-made slots"""
    offsets = np.asarray(offsets, np.int64)
    n_streams = offsets.size - 1
    ids = np.concatenate([np.arange(offsets[s + 1] - offsets[s]) * 10 + 5 for s in range(n_streams)] + [np.zeros(0, np.int64)])
    return {'stream_frame_offsets': offsets, 'frame_ids': ids.astype(np.int64), 'stream_keys': [('seg%d' % s, 'FRONT') for s in range(n_streams)]}


def arrays(result):
    return {'frame': np.asarray(result['frame'], np.int64), 'category': np.asarray(result['category'], np.int32),
            'bbox': np.asarray(result['bbox'], np.float64).reshape(-1, 4), 'score': np.asarray(result['score'], np.float64),
            'object_id': np.asarray(result['object_id'], np.int64)}


def same_bits(got, ref):
    """float64 arrays equal bit for bit, any NaN equal to any NaN"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64).reshape(np.shape(got))
    nan = np.isnan(got) & np.isnan(ref)
    return got.dtype == np.float64 and bool((nan | (got.view(np.int64) == ref.view(np.int64))).all())


def assert_same(got, ref, out):
    """got: a dict of tracking/split.py; ref: split_ref.split() of `out`"""
    assert [int(v) for v in got['object_id']] == ref['object_id']
    assert got['piece'].dtype == np.int32 and got['piece'].tolist() == ref['piece']
    assert got['new'].dtype == np.int64 and got['new'].tolist() == ref['new']
    assert got['test'].shape == (len(ref['test']), 2) and same_bits(got['test'], ref['test'])
    assert got['breaks'].dtype == np.int32 and got['breaks'].tolist() == ref['breaks']
    assert got['n_new_pieces'].tolist() == ref['n_new_pieces'] and got['traj_offsets'].tolist() == ref['traj_offsets'] and got['n_new'] == ref['n_new']
    for name in ('frame', 'category', 'bbox', 'score'):                  # no row is added, removed, moved or changed
        assert got[name].dtype == np.asarray(out[name]).dtype and got[name].tobytes() == np.asarray(out[name]).tobytes(), name
    assert got['object_id'].dtype == np.asarray(out['object_id']).dtype


def with_ids(out, ref):
    """the input rows with the reference's object ids: what the later passes and the writers take"""
    return dict(out, object_id=np.asarray(ref['object_id'], dtype=np.asarray(out['object_id']).dtype))


def lds_limit():
    from waymo_2d_tracking_amd import _lib
    n = C.c_int32(0)
    _lib.lib().wt_split_tracks_limits(C.byref(n))
    return n.value


@pytest.fixture(scope='module')
def tracked(golden_dir):
    """The two tracking fixtures tracked with max_age 2: [(packed, out)], g4 first."""
    from waymo_2d_tracking_amd.tracking import utils as T
    sets = []
    for name, cfg in (('sort_g4_input.json', G4), ('sort_g5_input.json', G5)):
        packed = T.pack_streams(T.read_data_file(os.path.join(golden_dir, name), cfg['score']))
        sets.append((packed, T.track_packed(packed, cfg['iou'], 2, 0)[0]))
    return sets


@pytest.fixture(scope='module')
def tracked_refs(tracked):
    return [[split_ref.split(packed['stream_frame_offsets'], out, j) for j in JOBS] for packed, out in tracked]


@pytest.mark.parametrize('name', sorted(split_cases.CASES))
def test_case_equals_reference(name):
    from waymo_2d_tracking_amd.tracking import split as S
    offsets, result, jobs, claim = split_cases.CASES[name]()
    refs = [split_ref.split(offsets, result, j) for j in jobs]
    claim(refs)
    out = arrays(result)
    got = S.split_tracks(packed_for(offsets), [out], jobs)
    assert len(got) == len(refs)
    for g, ref in zip(got, refs):
        assert_same(g, ref, out)


@pytest.mark.parametrize('n,empty_stream', [(63, False), (64, False), (65, False), (65, True), (257, True)])
def test_many_trajectories_in_a_slot_and_scans_across_lanes_chunks_and_streams(n, empty_stream):
    from waymo_2d_tracking_amd.tracking import split as S
    offsets, result, jobs, claim = split_cases.many_in_a_slot(n, empty_stream=empty_stream)
    refs = [split_ref.split(offsets, result, j) for j in jobs]
    claim(refs)
    out = arrays(result)
    for g, ref in zip(S.split_tracks(packed_for(offsets), [out], jobs), refs):
        assert_same(g, ref, out)


@pytest.mark.parametrize('above', [0, 1], ids=['tables_in_lds', 'tables_in_workspace'])
def test_trajectory_counts_on_either_side_of_the_lds_limit(above):
    from waymo_2d_tracking_amd.tracking import split as S
    limit = lds_limit()
    assert 64 < limit <= 4096
    n = limit + above
    rows = []                                                            # four rows per trajectory; every third jumps after its second
    for f in range(4):
        rows += [(f, 1 + k % 4, [4.0 * f + (400.0 if (k % 3 == 0 and f >= 2) else 0.0), 60.0 * k, 50.0, 40.0], 0.9, k) for k in range(n)]
    result = split_cases.result(rows)
    jobs = [split_cases.job(0.3, motion='hold'), split_cases.job([0.3, 0.0, 0.3, 0.3], motion='hold')]
    refs = [split_ref.split([0, 4], result, j) for j in jobs]
    assert refs[0]['breaks'] == [1 if k % 3 == 0 else 0 for k in range(n)] and refs[0]['n_new'] == (n + 2) // 3
    out = arrays(result)
    p = S._prepare(packed_for([0, 4]), [out], jobs, 4)
    assert p['n_traj'].tolist() == [[n]]
    for g, ref in zip(S.split_tracks(packed_for([0, 4]), [out], jobs), refs):
        assert_same(g, ref, out)
    dev = S.DeviceSplit(packed_for([0, 4]), [out], jobs)
    dev.launch()
    for g, ref in zip(dev.results(), refs):
        assert_same(g, ref, out)


def test_all_off_reproduces_the_tracked_sequences(tracked):
    from waymo_2d_tracking_amd.tracking import split as S
    for packed, out in tracked:
        got = S.split_tracks(packed, [out], [{}, {'split_iou': [0.0, -1.0, 0.0, 0.0], 'split_gap': 0, 'motion': 'hold'}])
        for g in got:
            for name in ('frame', 'category', 'bbox', 'score', 'object_id'):
                assert g[name].dtype == out[name].dtype and g[name].tobytes() == out[name].tobytes(), name
            assert g['n_new'] == 0 and not g['breaks'].any() and not g['piece'].any() and (g['new'] == -1).all() and (g['test'] == -1.0).all()
        assert S.split_one(packed, out, 0.0) is out
    assert len(tracked[0][1]['frame']) > 300


def test_settings_on_the_tracked_sequences_equal_the_reference(tracked, tracked_refs):
    from waymo_2d_tracking_amd.tracking import split as S
    for (packed, out), refs in zip(tracked, tracked_refs):
        for g, ref in zip(S.split_tracks(packed, [out], JOBS), refs):
            assert_same(g, ref, out)
    made = [ref['n_new'] for ref in tracked_refs[0]]
    assert made[2] > 0 and made[3] > 0 and max(made) < len(tracked_refs[0][0]['piece'])      # max_age 2 left gaps of two slots: the rules are live
    assert min(v for v, n in zip(tracked_refs[0][3]['object_id'], tracked_refs[0][3]['new']) if n >= 0) == 100000


def test_jobs_over_results_in_one_call_equal_single_calls_and_dev_equals_host(tracked, tracked_refs):
    import torch
    from waymo_2d_tracking_amd.tracking import split as S, utils as T
    packed, out = tracked[0]
    other = T.track_packed(packed, G4['iou'], 3, 0)[0]                    # a second result over the same slots
    outs = [out, other]
    other_refs = [split_ref.split(packed['stream_frame_offsets'], other, j) for j in JOBS]
    refs = [tracked_refs[0], other_refs]
    pairs = [(1, 0), (0, 1), (1, 3), (0, 2), (1, 1), (0, 2)]             # (result, job): results interleaved, one job twice
    jobs = [dict(JOBS[j], result=r) for r, j in pairs]
    together = S.split_tracks(packed, outs, jobs)
    dev = S.DeviceSplit(packed, outs, jobs)
    dev.launch()
    from_dev = dev.results()
    for (r, j), a, b in zip(pairs, together, from_dev):
        alone = S.split_tracks(packed, [outs[r]], [JOBS[j]])[0]
        for got in (alone, a, b):
            assert_same(got, refs[r][j], outs[r])                         # the piece numbers restart with every job
    # the entries of the result a job does not name are -1 (-1.0)
    p = dev.p
    J = len(jobs)
    piece = dev.out['piece'].cpu().numpy().reshape(J, -1)
    new = dev.out['new'].cpu().numpy().reshape(J, -1)
    test = dev.out['test'].cpu().numpy().reshape(J, -1, 2)
    breaks = dev.out['breaks'].cpu().numpy().reshape(J, -1)
    cut, rows = int(p['traj_offsets'][p['n_streams']]), int(p['set_row_offsets'][1])
    assert (piece[0, :rows] == -1).all() and (piece[0, rows:] >= 0).all() and (new[0, :rows] == -1).all() and (test[0, :rows] == -1.0).all()
    assert (breaks[0, :cut] == -1).all() and (breaks[0, cut:] >= 0).all()
    assert (piece[1, rows:] == -1).all() and (piece[1, :rows] >= 0).all() and (breaks[1, cut:] == -1).all() and (test[1, rows:] == -1.0).all()
    # a second launch on the same buffers gives the same answer (the call initialises everything it reads)
    dev.launch()
    for a, b in zip(from_dev, dev.results()):
        assert all(np.array_equal(a[k], b[k]) for k in ('object_id', 'piece', 'new', 'breaks', 'n_new_pieces')) and same_bits(a['test'], b['test'])
    # a workspace that is one byte short: WT_ERR_CAPACITY, nothing launched
    from waymo_2d_tracking_amd import _lib
    small = S.DeviceSplit(packed, outs, jobs, workspace_bytes=dev.ws_bytes - 1)
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY'):
        small.launch()
    torch.cuda.synchronize()


def test_unsorted_input_equals_the_sorted_one(tracked, tracked_refs):
    from waymo_2d_tracking_amd.tracking import split as S
    packed, out = tracked[0]
    perm = np.random.default_rng(4).permutation(len(out['frame']))
    shuffled = dict((k, v[perm]) for k, v in out.items())
    got = S.split_tracks(packed, [shuffled], JOBS[1:3])
    for g, j, ref in zip(got, JOBS[1:3], tracked_refs[0][1:3]):
        assert_same(g, split_ref.split(packed['stream_frame_offsets'], shuffled, j), shuffled)
        # the rows keep the caller's order; the pieces are those of the sorted input
        assert g['piece'].tolist() == [ref['piece'][i] for i in perm]


def swap_chain():
    """two objects on parallel lines; the tracker's ids swap from slot 10 on"""
    rows, anns = [], []
    for f in range(20):
        a, b = (1, 2) if f < 10 else (2, 1)
        rows += [(f, 1, [10.0 * f, 0.0, 50.0, 40.0], 0.9, a), (f, 1, [10.0 * f, 200.0, 50.0, 40.0], 0.9, b)]
        anns += [{'image_id': 'seg0/%d/FRONT' % (f * 10 + 5), 'bbox': [10.0 * f, y, 50.0, 40.0], 'category_id': 1, 'object_id': 'g%d' % o}
                 for o, y in ((1, 0.0), (2, 200.0))]
    return rows, anns


def test_split_then_stitch_removes_the_identity_swap():
    from waymo_2d_tracking_amd.tracking import split as S, stitch as ST, utils as T
    rows, anns = swap_chain()
    packed, out = packed_for([0, 20]), arrays(split_cases.result(rows))
    cut = S.split_tracks(packed, [out], [split_cases.job(0.3)])[0]
    ref = split_ref.split([0, 20], out, split_cases.job(0.3))
    assert_same(cut, ref, out)
    assert cut['n_new'] == 2 and sorted(set(cut['object_id'].tolist())) == [1, 2, 3, 4]
    link = stitch_cases.job(max_link=1, link_iou=0.3)
    linked = ST.stitch_tracks(packed, [cut], [link])[0]
    assert [int(v) for v in linked['object_id']] == stitch_ref.stitch([0, 20], with_ids(out, ref), link)['object_id']
    plain = lambda r: json.loads(json.dumps(T.format_tracks(packed, {k: r[k] for k in ('frame', 'category', 'bbox', 'score', 'object_id')})))
    scores = []
    for result in (out, cut, linked):
        tracks = plain(result)
        scores.append((mot_ref.evaluate(anns, tracks)['table']['ALL'][2]['idsw'], mot_id_ref.evaluate(anns, tracks)['table']['ALL'][2]['idf1']))
    assert scores[0][0] == 2 and scores[0][1] == 0.5                      # before: both objects switch, each identity keeps half
    assert scores[1][0] == 2 and scores[1][1] == 0.5                      # split alone: the same switches under new names
    assert scores[2] == (0, 1.0)                                         # split + stitch: no switch, every identity whole


def as_rows(r):
    return {'frame': np.asarray(r['frame'], np.int64), 'category': np.asarray(r['category'], np.int32), 'bbox': np.asarray(r['bbox'], np.float64).reshape(-1, 4),
            'score': np.asarray(r['score'], np.float64), 'object_id': np.asarray(r['object_id'], np.int64)}


def _expected_file(path, score_thr, iou_thr, max_age, split, link=None, dedup=None, refine=None, smooth=None):
    """what track.py has to write: the tracker's rows through the reference splitting, stitching, deduplication, refinement and
    smoothing - in this order - and format_tracks; new ids from the id counter"""
    from waymo_2d_tracking_amd.tracking import utils as T
    packed = T.pack_streams(T.read_data_file(path, score_thr))
    out, births = T.track_packed(packed, iou_thr, max_age, 0)
    ref = split_ref.split(packed['stream_frame_offsets'], out, dict(split, first_new_id=births + 1))     # a birth is written as the counter + 1
    rows = with_ids(out, ref)
    if link is not None:
        rows = with_ids(rows, stitch_ref.stitch(packed['stream_frame_offsets'], rows, link))
    if dedup is not None:
        rows = as_rows(dedup_ref.dedup(packed['stream_frame_offsets'], rows, dedup))
    if refine is not None:
        rows = as_rows(refine_ref.refine(packed['stream_frame_offsets'], rows, refine))
    if smooth is not None:
        rows = dict(rows, bbox=np.asarray(smooth_ref.smooth(packed['stream_frame_offsets'], rows, smooth)['bbox'], np.float64).reshape(-1, 4))
    return T.format_tracks(packed, rows), ref, int(np.asarray(out['object_id']).max()) + 1, births


@pytest.mark.parametrize('fixture,cfg', [('sort_g5_input.json', G5), ('sort_g4_input.json', G4)])
def test_cli_writes_the_split_file(golden_dir, tmp_path, fixture, cfg):
    from waymo_2d_tracking_amd.tracking import track, utils as T
    path = os.path.join(golden_dir, fixture)
    base = ['--input', path, '--max-age=2', '--score-threshold=' + ','.join(map(str, cfg['score']))]
    runs = [(['--split-iou', '0.3'], split_cases.job(0.3), None, None, None, None),
            (['--split-iou=0.3,0.3,0,0.5', '--split-gap=1', '--split-motion=hold', '--link-gap=3', '--link-iou=0.3', '--link-motion=linear',
              '--dedup-frames=3', '--dedup-iou=0.5', '--interpolate-gap=2', '--min-track-len=2', '--smooth-window=1', '--smooth-kernel=box'],
             split_cases.job([0.3, 0.3, 0.0, 0.5], 1, motion='hold'), stitch_cases.job(max_link=3, link_iou=0.3, motion='linear'),
             dedup_cases.job(min_frames=3, dup_iou=0.5), refine_cases.job(max_gap=2, min_len=2), smooth_cases.job(window=1, kernel='box'))]
    for k, (flags, split, link, dedup, refine, smooth) in enumerate(runs):     # the second run: all five passes, in their order
        expected, ref, next_id, births = _expected_file(path, cfg['score'], cfg['iou'], 2, split, link, dedup, refine, smooth)
        assert next_id <= births + 1                                         # no tracked id lies above the id counter
        if 'g4' in fixture and k == 1:
            assert ref['n_new'] > 0                                          # the flags are live on this input
        for name, extra in (('native%d.json' % k, []), ('python%d.json' % k, ['--python-io'])):
            T.reset_global_ids(0)
            assert track.main(base + flags + ['--output', str(tmp_path / name)] + extra) == 0
            assert T._GLOBAL_IDS['next'] == births + ref['n_new']            # the new pieces moved the counter on, as births do
        assert (tmp_path / ('python%d.json' % k)).read_text() == json.dumps(expected)
        assert (tmp_path / ('native%d.json' % k)).read_bytes() == (tmp_path / ('python%d.json' % k)).read_bytes()


def test_cli_default_flags_write_what_they_wrote(golden_dir, tmp_path):
    import sys
    from waymo_2d_tracking_amd.tracking import track, utils as T
    for fixture, score in (('sort_g5_input.json', '0.95,0.6,1.0,0.9'), ('sort_g4_input.json', '0.3,0.3,1.0,0.2')):
        path = os.path.join(golden_dir, fixture)
        flags = ['--input', path, '--max-age=2', '--score-threshold=' + score]
        T.reset_global_ids(0)
        unsplit = json.dumps(T.track_all(T.read_data_file(path, [float(v) for v in score.split(',')]), [0.01, 0.01, 1.0, 0.0], 2, 0))
        written = []
        sys.modules.pop('waymo_2d_tracking_amd.tracking.split', None)
        for i, extra in enumerate(([], ['--python-io'], ['--split-iou=0', '--split-gap=0', '--split-motion=hold'], ['--split-iou=0,0,0,0', '--python-io'])):
            T.reset_global_ids(0)
            assert track.main(flags + ['--output', str(tmp_path / ('t%d.json' % i))] + extra) == 0
            written.append((tmp_path / ('t%d.json' % i)).read_text())
        assert 'waymo_2d_tracking_amd.tracking.split' not in sys.modules        # with the flags off the pass is not even imported
        assert written[1] == unsplit and written[0] == written[1] == written[2] == written[3]
    args = track.build_parser().parse_args([])
    assert args.split_iou == [0.0] and args.split_gap == [0] and args.split_motion == 'linear' and not track.splits(args)


@pytest.fixture(scope='module')
def sweep_set(tmp_path_factory):
    """synthetic detections of one segment and two cameras"""
    from waymo_2d_tracking_amd import synthetic as syn
    dets, gt_json = syn.make_tracking_json(23, n_segments=1, n_frames=12, n_objects=12, cameras=('FRONT', 'SIDE_LEFT'))
    path = tmp_path_factory.mktemp('split_sweep') / 'det.json'
    path.write_text(json.dumps(dets))
    return str(path), dets, gt_json


def test_sweep_with_a_split_grid_equals_the_references(sweep_set):
    from waymo_2d_tracking_amd.tracking import evaluate as E, utils as T
    path, dets, gt_json = sweep_set
    grid = {'score': [0.3, 0.6], 'iou': [0.01], 'max_age': [1, 2], 'min_hits': [0], 'split_iou': [0.0, 0.3, 0.9], 'split_gap': 2,
            'link_gap': [0, 2], 'link_iou': [0.3], 'gap': [0, 1], 'min_len': [1]}
    res = E.sweep(path, E.load_ground_truth(gt_json), grid, identity=True, hota=True)
    assert len(res['settings']) == 48
    assert res['settings'][5] == {'max_age': 1, 'min_hits': 0, 'score': 0.3, 'iou': 0.01, 'split_iou': 0.3, 'link_gap': 0, 'link_iou': 0.3,
                                  'interp_gap': 1, 'min_len': 1}
    predictions = {}
    for e in dets:
        seg, fr, cam = e['image_id'].split('/')
        predictions.setdefault(seg, {}).setdefault(cam, {}).setdefault(int(fr), []).append(
            {'bbox': e['bbox'], 'score': e['score'], 'category_id': e['category_id']})
    packed = T.pack_streams(predictions)
    cache = {}

    def reference(s):
        key = tuple(sorted(s.items()))
        if key not in cache:
            out, _ = T.track_packed(packed, [s['iou']] * 4, s['max_age'], s['min_hits'], [s['score']] * 4)
            cut = with_ids(out, split_ref.split(packed['stream_frame_offsets'], out, split_cases.job(s['split_iou'], 2)))
            linked = with_ids(cut, stitch_ref.stitch(packed['stream_frame_offsets'], cut, stitch_cases.job(max_link=s['link_gap'], link_iou=s['link_iou'])))
            ref = refine_ref.refine(packed['stream_frame_offsets'], linked, refine_cases.job(max_gap=s['interp_gap'], min_len=s['min_len']))
            rows = json.loads(json.dumps(T.format_tracks(packed, {
                'frame': np.asarray(ref['frame'], np.int64), 'category': np.asarray(ref['category'], np.int32),
                'bbox': np.asarray(ref['bbox'], np.float64).reshape(-1, 4), 'score': np.asarray(ref['score'], np.float64),
                'object_id': np.asarray(ref['object_id'], np.int64)})))
            cache[key] = (mot_ref.evaluate(gt_json, rows)['table'], mot_id_ref.evaluate(gt_json, rows)['table'], hota_ref.evaluate(gt_json, rows))
        return cache[key]
    same = lambda a, b: a == b or (a != a and b != b)
    hyp_ids = {}
    for k, s in enumerate(res['settings']):
        mot, ident, hota = reference(s)
        assert_hota_equals_reference(res['hota_results'][k], hota)
        for c in E.ALL_CLASSES:
            assert [res['results'][k].table[c][2][f] for f in mot_ref.FIELDS] == [mot[c][2][f] for f in mot_ref.FIELDS], (k, c)
            assert res['id_results'][k].table[c][2]['idtp'] == ident[c][2]['idtp'] and same(res['id_results'][k].table[c][2]['idf1'], ident[c][2]['idf1'])
        hyp_ids[(s['max_age'], s['score'], s['split_iou'], s['link_gap'], s['interp_gap'])] = mot['ALL'][2]['idsw']
    assert len(set(hyp_ids.values())) > 1
    # the axis is live: splitting at 0.9 changes the switches somewhere
    assert any(hyp_ids[(a, sc, 0.9, g, i)] != hyp_ids[(a, sc, 0.0, g, i)] for a in (1, 2) for sc in (0.3, 0.6) for g in (0, 2) for i in (0, 1))
    for lv in (1, 2):
        assert len(res['ranked'][lv]) == 2
        for row in res['ranked'][lv]:
            total = dict((f, 0) for f in mot_ref.FIELDS)
            for c in E.ALL_CLASSES:
                i = c - 1
                s = {'max_age': row['max_age'], 'min_hits': row['min_hits'], 'score': row['score_threshold'][i], 'iou': row['iou_threshold'][i],
                     'split_iou': row['split_iou'][i], 'link_gap': row['link_gap'][i], 'link_iou': row['link_iou'][i],
                     'interp_gap': row['interp_gap'][i], 'min_len': row['min_len'][i]}
                for f in mot_ref.FIELDS:
                    total[f] += reference(s)[0][c][lv][f]
            assert row['counts'] == total, (lv, row)
            assert row['split_iou'][2] == 0.0 and row['split_gap'] == 2 and row['split_motion'] == 'linear'
            assert ' --split-iou=%s --split-gap=2 --link-gap=' % ','.join(repr(float(v)) for v in row['split_iou']) in E.flag_line(row)


def test_sweep_with_the_default_split_grid_is_the_sweep_without_it(sweep_set):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    path, _, gt_json = sweep_set
    gt = E.load_ground_truth(gt_json)
    for grid in ({'score': [0.3, 0.6], 'iou': [0.01, 0.1], 'max_age': [1, 3], 'min_hits': [0, 1]},
                 {'score': [0.3], 'iou': [0.01], 'max_age': [1, 3], 'min_hits': [0], 'link_gap': [0, 2], 'gap': [0, 1], 'min_len': [1, 2]}):
        old = E.sweep(path, gt, grid)                                   # no split axis: the code path before it
        new = E.sweep(path, gt, dict(grid, split_iou=[0.0], split_gap=3, split_motion='hold'))
        for key in ('settings', 'ranked', 'best'):
            assert json.dumps(old[key], sort_keys=True) == json.dumps(new[key], sort_keys=True)
        assert sorted(old) == sorted(new) and 'split_iou' not in old['settings'][0] and 'split_iou' not in old['best'][2]
        assert 'split' not in E.flag_line(new['best'][2]) and E.flag_line(new['best'][2]) == E.flag_line(old['best'][2])
    args = E.build_parser().parse_args(['--annotations', 'x'])
    assert args.split_iou_grid == '0' and args.split_gap == 0 and args.split_motion == 'linear'
