"""HIP track splitting (csrc/track_split.hip through tracking/split.py) against the plain-Python restatement tests/split_ref.py:
object ids, pieces, piece numbers, the tests of every pair, the breaks and the new pieces per stream must be EQUAL bit for bit (a
NaN test equals a NaN test) - the unfused extrapolations and the operation order of the IoU are part of the definition (DESIGN.md
section 25).  The comparator and the bodies shared with the other post-passes are in tests/track_stage_support.py."""
import json
import os

import numpy as np
import pytest

import dedup_cases
import mot_id_ref
import mot_ref
import refine_cases
import smooth_cases
import split_cases
import split_ref
import stitch_cases
import stitch_ref
import track_stage_support as H
from mot_support import assert_hota_equals_reference
from track_stage_support import G4, G5, arrays, packed_for, same_bits, with_ids

pytestmark = pytest.mark.gpu

STAGE = H.STAGES['split']
assert_same = STAGE.assert_same
JOBS = [split_cases.job(0.3), split_cases.job([0.5, 0.2, 0.0, 0.3], [0, 1, 1, 0]), split_cases.job(0.3, 1, motion='hold'),
        split_cases.job(0.0, 1, first_new_id=100000)]


@pytest.fixture(scope='module')
def tracked(golden_dir):
    """The two tracking fixtures tracked with max_age 2: [(packed, out)], g4 first."""
    return H.tracked_fixtures(golden_dir)


@pytest.fixture(scope='module')
def tracked_refs(tracked):
    return [[split_ref.split(packed['stream_frame_offsets'], out, j) for j in JOBS] for packed, out in tracked]


@pytest.mark.parametrize('name', sorted(split_cases.CASES))
def test_case_equals_reference(name):
    H.check_case(STAGE, name)


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
    def jumping_trajectories(n):
        rows = []                                                        # four rows per trajectory; every third jumps after its second
        for f in range(4):
            rows += [(f, 1 + k % 4, [4.0 * f + (400.0 if (k % 3 == 0 and f >= 2) else 0.0), 60.0 * k, 50.0, 40.0], 0.9, k) for k in range(n)]

        def claim(refs):
            assert refs[0]['breaks'] == [1 if k % 3 == 0 else 0 for k in range(n)] and refs[0]['n_new'] == (n + 2) // 3
        return [0, 4], split_cases.result(rows), [split_cases.job(0.3, motion='hold'), split_cases.job([0.3, 0.0, 0.3, 0.3], motion='hold')], claim
    H.check_either_side_of_the_lds_limit(STAGE, above, make_case=jumping_trajectories)


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
    from waymo_2d_tracking_amd.tracking import utils as T
    packed, out = tracked[0]
    other = T.track_packed(packed, G4['iou'], 3, 0)[0]                    # a second result over the same slots
    outs = [out, other]
    other_refs = [split_ref.split(packed['stream_frame_offsets'], other, j) for j in JOBS]
    pairs = [(1, 0), (0, 1), (1, 3), (0, 2), (1, 1), (0, 2)]             # (result, job): results interleaved, one job twice
    # every job equals its reference: the piece numbers restart with every job
    dev, jobs, from_dev = H.check_jobs_over_results(STAGE, packed, outs, [tracked_refs[0], other_refs], JOBS, pairs)
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
    H.check_relaunch_and_short_workspace(STAGE, dev, from_dev, packed, outs, jobs, lambda a, b: all(
        np.array_equal(a[k], b[k]) for k in ('object_id', 'piece', 'new', 'breaks', 'n_new_pieces')) and same_bits(a['test'], b['test']))


def test_unsorted_input_equals_the_sorted_one(tracked, tracked_refs):
    def per_row(g, ref, perm):
        # the rows keep the caller's order; the pieces are those of the sorted input
        assert g['piece'].tolist() == [ref['piece'][i] for i in perm]
    H.check_shuffled(STAGE, *tracked[0], JOBS[1:3], tracked_refs[0][1:3], per_row)


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


@pytest.mark.parametrize('fixture,cfg', [('sort_g5_input.json', G5), ('sort_g4_input.json', G4)])
def test_cli_writes_the_split_file(golden_dir, tmp_path, fixture, cfg):
    from waymo_2d_tracking_amd.tracking import track, utils as T
    path = os.path.join(golden_dir, fixture)
    base = ['--input', path, '--max-age=2', '--score-threshold=' + ','.join(map(str, cfg['score']))]
    runs = [(['--split-iou', '0.3'], {'split': split_cases.job(0.3)}),
            (['--split-iou=0.3,0.3,0,0.5', '--split-gap=1', '--split-motion=hold', '--link-gap=3', '--link-iou=0.3', '--link-motion=linear',
              '--dedup-frames=3', '--dedup-iou=0.5', '--interpolate-gap=2', '--min-track-len=2', '--smooth-window=1', '--smooth-kernel=box'],
             {'split': split_cases.job([0.3, 0.3, 0.0, 0.5], 1, motion='hold'), 'stitch': stitch_cases.job(max_link=3, link_iou=0.3, motion='linear'),
              'dedup': dedup_cases.job(min_frames=3, dup_iou=0.5), 'refine': refine_cases.job(max_gap=2, min_len=2),
              'smooth': smooth_cases.job(window=1, kernel='box')})]
    for k, (flags, passes) in enumerate(runs):                               # the second run: all five passes, in their order; new ids from the id counter
        expected, refs, out, births = H._expected_file(path, cfg['score'], cfg['iou'], 2, passes)
        ref, next_id = refs['split'], int(np.asarray(out['object_id']).max()) + 1
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
    from waymo_2d_tracking_amd.tracking import track
    H.check_cli_default_flags(golden_dir, tmp_path, (['--split-iou=0', '--split-gap=0', '--split-motion=hold'], ['--split-iou=0,0,0,0', '--python-io']),
                              module='waymo_2d_tracking_amd.tracking.split')       # with the flags off the pass is not even imported
    args = track.build_parser().parse_args([])
    assert args.split_iou == [0.0] and args.split_gap == [0] and args.split_motion == 'linear' and not track.splits(args)


@pytest.fixture(scope='module')
def sweep_set(tmp_path_factory):
    """synthetic detections of one segment and two cameras"""
    return H.sweep_set(tmp_path_factory, 'split_sweep')


def test_sweep_with_a_split_grid_equals_the_references(sweep_set):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    path, dets, gt_json = sweep_set
    grid = {'score': [0.3, 0.6], 'iou': [0.01], 'max_age': [1, 2], 'min_hits': [0], 'split_iou': [0.0, 0.3, 0.9], 'split_gap': 2,
            'link_gap': [0, 2], 'link_iou': [0.3], 'gap': [0, 1], 'min_len': [1]}
    res = E.sweep(path, E.load_ground_truth(gt_json), grid, identity=True, hota=True)
    assert len(res['settings']) == 48
    assert res['settings'][5] == {'max_age': 1, 'min_hits': 0, 'score': 0.3, 'iou': 0.01, 'split_iou': 0.3, 'link_gap': 0, 'link_iou': 0.3,
                                  'interp_gap': 1, 'min_len': 1}
    reference = H.sweep_reference(dets, gt_json, lambda s: {'split': split_cases.job(s['split_iou'], 2),
                                                            'stitch': stitch_cases.job(max_link=s['link_gap'], link_iou=s['link_iou']),
                                                            'refine': refine_cases.job(max_gap=s['interp_gap'], min_len=s['min_len'])})
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
