"""HIP track smoothing (csrc/track_smooth.hip through tracking/smooth.py) against the plain-Python restatement
tests/smooth_ref.py: every smoothed value and every pair count must be EQUAL bit for bit (two NaNs count as equal) - the order of
the distances, the sum of the pair before the product and the unfused accumulation are part of the definition (DESIGN.md
section 22)."""
import json
import os

import numpy as np
import pytest

import mot_ref
import refine_cases
import refine_ref
import smooth_cases
import smooth_ref
import stitch_cases
import track_stage_support as H
from mot_support import assert_hota_equals_reference
from track_stage_support import G4, G5, arrays, gt_box, packed_for, same_bits, with_boxes

pytestmark = pytest.mark.gpu

STAGE = H.STAGES['smooth']
assert_same = STAGE.assert_same
JOBS = [smooth_cases.job(window=2, sigma=1.0), smooth_cases.job(window=[3, 1, 0, 2], sigma=1.5, n_weights=6), smooth_cases.job(window=1, kernel='box'),
        smooth_cases.job(window=3, weights=[1.0, 0.5, 0.25, 0.125])]


@pytest.fixture(scope='module')
def tracked(golden_dir):
    """The two tracking fixtures tracked with max_age 2: [(packed, out)], g4 first."""
    return H.tracked_fixtures(golden_dir)


@pytest.fixture(scope='module')
def tracked_refs(tracked):
    return [[smooth_ref.smooth(packed['stream_frame_offsets'], out, j) for j in JOBS] for packed, out in tracked]


@pytest.mark.parametrize('name', sorted(smooth_cases.CASES))
def test_case_equals_reference(name):
    H.check_case(STAGE, name)


def test_all_zero_windows_reproduce_the_tracked_sequences(tracked):
    from waymo_2d_tracking_amd.tracking import smooth as S
    for packed, out in tracked:
        got = S.smooth_tracks(packed, [out], [{}, {'window': [0, 0, 0, 0], 'sigma': 3.0}, {'window': 0, 'kernel': 'box'}])
        assert len(got) == 3
        for g in got:
            for name in ('frame', 'category', 'bbox', 'score', 'object_id'):
                assert g[name].dtype == out[name].dtype and g[name].tobytes() == out[name].tobytes(), name
            assert not g['pairs'].any()
    assert len(tracked[0][1]['frame']) > 300


def test_settings_on_the_tracked_sequences_equal_the_reference(tracked, tracked_refs):
    from waymo_2d_tracking_amd.tracking import smooth as S
    for (packed, out), refs in zip(tracked, tracked_refs):
        for g, ref in zip(S.smooth_tracks(packed, [out], JOBS), refs):
            assert_same(g, ref, out)
    moved = [sum(1 for n in ref['pairs'] if n) for ref in tracked_refs[0]]
    assert min(moved) > 0 and max(tracked_refs[0][1]['pairs']) >= 2                  # the settings are live on this input
    # the kernel / sigma form of a job gives the weights of the definition
    packed, out = tracked[0]
    named = S.smooth_tracks(packed, [out], [{'window': 2, 'sigma': 1.0}, {'window': [3, 1, 0, 2], 'kernel': 'gaussian', 'sigma': [1.5] * 4}, {'window': 1, 'kernel': 'box'}])
    for g, ref in zip(named, tracked_refs[0][:3]):
        assert_same(g, ref, out)
    one = S.smooth_one(packed, out, [3, 1, 0, 2], 1.5)
    assert_same(one, tracked_refs[0][1], out)


def test_jobs_over_results_in_one_call_equal_single_calls_and_dev_equals_host(tracked, tracked_refs):
    from waymo_2d_tracking_amd.tracking import utils as T
    packed, out = tracked[0]
    other = T.track_packed(packed, G4['iou'], 3, 0)[0]                    # a second result over the same slots
    outs = [out, other]
    other_refs = [smooth_ref.smooth(packed['stream_frame_offsets'], other, j) for j in JOBS]
    pairs = [(1, 0), (0, 1), (1, 3), (0, 2), (1, 1), (0, 2)]             # (result, job): results interleaved, one job twice
    dev, jobs, from_dev = H.check_jobs_over_results(STAGE, packed, outs, [tracked_refs[0], other_refs], JOBS, pairs)
    assert dev.n_out == 3 * len(out['frame']) + 3 * len(other['frame'])
    H.check_relaunch_and_short_workspace(STAGE, dev, from_dev, packed, outs, jobs,
                                         lambda a, b: same_bits(a['bbox'], b['bbox']) and np.array_equal(a['pairs'], b['pairs']))


def test_unsorted_input_equals_the_sorted_one(tracked, tracked_refs):
    def per_row(g, ref, perm):
        # the rows keep the caller's order, and every row gets the box it gets in the sorted input
        assert same_bits(g['bbox'], np.asarray(ref['bbox'], np.float64)[perm]) and g['pairs'].tolist() == [ref['pairs'][i] for i in perm]
    H.check_shuffled(STAGE, *tracked[0], JOBS[1:3], tracked_refs[0][1:3], per_row)


@pytest.mark.parametrize('above', [0, 1], ids=['table_in_lds', 'table_in_workspace'])
def test_trajectory_counts_on_either_side_of_the_lds_limit(above):
    H.check_either_side_of_the_lds_limit(STAGE, above)


def test_two_jobs_on_one_result_do_not_interfere():
    """two results whose trajectories have the same local indices, smoothed by three jobs in one call: each keeps its own boxes"""
    from waymo_2d_tracking_amd.tracking import smooth as S
    a = smooth_cases.result([(f, 1, smooth_cases.box_of(0, f * f), 0.5, 1) for f in range(5)])
    b = smooth_cases.result([(f, 1, smooth_cases.box_of(1, f * f * f), 0.5, 1) for f in (0, 1, 2, 4)])
    jobs = [dict(smooth_cases.job(window=1, kernel='box'), result=0), dict(smooth_cases.job(window=2, sigma=1.0), result=1),
            dict(smooth_cases.job(window=2, kernel='box'), result=0), dict(smooth_cases.job(window=0), result=1)]
    got = S.smooth_tracks(packed_for([0, 5]), [arrays(a), arrays(b)], jobs)
    refs = [smooth_ref.smooth([0, 5], r, j) for r, j in ((a, jobs[0]), (b, jobs[1]), (a, jobs[2]), (b, jobs[3]))]
    assert [r['pairs'] for r in refs] == [[0, 1, 1, 1, 0], [0, 1, 1, 0], [0, 1, 2, 1, 0], [0, 0, 0, 0]]
    for g, ref, out in zip(got, refs, (a, b, a, b)):
        assert_same(g, ref, arrays(out))
    assert not same_bits(got[0]['bbox'], got[2]['bbox'])


def test_results_of_the_other_passes_are_taken_as_they_are(tracked):
    """the dicts refine_tracks and stitch_tracks return go in unchanged, and filled rows are smoothed like observed ones"""
    from waymo_2d_tracking_amd.tracking import refine as R, smooth as S, stitch as St
    packed, out = tracked[0]
    linked = St.stitch_tracks(packed, [out], [{'max_link': 4, 'link_iou': 0.2}])[0]
    filled = R.refine_tracks(packed, [linked], [{'max_gap': 2, 'min_len': 2}])[0]
    assert (filled['source'] < 0).any()
    for rows in (linked, filled):
        got = S.smooth_tracks(packed, [rows], [JOBS[0]])[0]
        assert_same(got, smooth_ref.smooth(packed['stream_frame_offsets'], rows, JOBS[0]), rows)
    assert S.smooth_tracks(packed, [filled], [JOBS[0]])[0]['pairs'][filled['source'] < 0].any()


def test_invalid_input_is_refused():
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import smooth as S
    rows = [(0, 1, [0, 0, 5, 5], 0.5, 1), (3, 1, [0, 0, 5, 5], 0.5, 2), (4, 1, [0, 0, 5, 5], 0.5, 3), (4, 1, [9, 9, 5, 5], 0.5, 2), (4, 1, [1, 1, 5, 5], 0.5, 3)]
    packed = packed_for([0, 3, 6])
    with pytest.raises(_lib.WaymoTrackError, match=r'WT_ERR_INVALID \(result 0: object_id 3 occurs twice in image seg1/15/FRONT\)'):
        S.smooth_tracks(packed, [arrays(smooth_cases.result(rows))], [smooth_cases.job(window=1)])
    out = arrays(smooth_cases.result(rows[:4]))
    with pytest.raises(ValueError, match='window must be in 0..32'):
        S.smooth_tracks(packed, [out], [{'window': 33}])
    # the C entry point on its own: the same layout with the errors written into the arrays
    p = S._prepare(packed, [out], [smooth_cases.job(window=1, kernel='box')], 4)
    o = [np.zeros((4, 4)), np.zeros(4, np.int32)]
    last = lambda: _lib.lib().wt_last_error()
    assert S._host_call(p, o) == 0 and o[1].tolist() == [0, 0, 0, 0] and o[0].tobytes() == out['bbox'].tobytes()
    p['job_window'][0, 1] = 33
    assert S._host_call(p, o) == 1 and b'window 33 of class 2 outside 0..32' in last()
    p['job_window'][0, 1] = 2
    assert S._host_call(p, o) == 1 and b'needs 3 weights, 2 given' in last()
    p['job_window'][0, 1] = 1
    p['job_weights'][0, 0, 0] = 0.0
    assert S._host_call(p, o) == 1 and b'weight 0 of class 1 must be above 0' in last()
    p['job_weights'][0, 0, 0] = 1.0
    p['local'][3] = p['local'][2]
    assert S._host_call(p, o) == 1 and b'occurs twice in frame 4' in last()
    p['local'][3] = 0
    assert S._host_call(p, o) == 0


def test_smoothing_improves_the_localisation_and_nothing_else():
    """Two objects moving on a line; the hypotheses are the truth with x shifted by +3, -3, +3, ...  Under the box of width 1 the
    interior shifts become -1, +1, ... - a third: every IoU but the ends' rises, so MOTP and LocA rise; matches and ids stay."""
    from waymo_2d_tracking_amd.tracking import evaluate as E, smooth as S
    n = 10
    anns = [{'image_id': 'seg0/%d/FRONT' % (f * 10 + 5), 'bbox': gt_box(o, f), 'category_id': o, 'object_id': 'g%d' % o} for f in range(n) for o in (1, 2)]
    noisy = lambda o, f: [gt_box(o, f)[0] + (3.0 if f % 2 == 0 else -3.0)] + gt_box(o, f)[1:]
    rows = [(f, o, noisy(o, f), 0.9, 10 + o) for f in range(n) for o in (1, 2)]
    packed, out = packed_for([0, n]), arrays(smooth_cases.result(rows))
    j = smooth_cases.job(window=1, kernel='box')
    got = S.smooth_tracks(packed, [out], [j])[0]
    assert_same(got, smooth_ref.smooth([0, n], out, j), out)
    shift = got['bbox'][:, 0] - np.asarray([gt_box(o, f)[0] for f in range(n) for o in (1, 2)])
    assert np.abs(shift[2:-2]).max() < 1.0 + 1e-9 and np.abs(shift[:2]).tolist() == [3.0, 3.0] and np.abs(shift[-2:]).tolist() == [3.0, 3.0]
    gt = E.load_ground_truth(anns)
    tracks = [E.tracks_from_packed(packed, r) for r in (out, got)]
    mot = E.evaluate_tracks(gt, tracks)
    hota = E.evaluate_hota(gt, tracks)
    for c in (1, 2, 'ALL'):
        before, after = mot[0].table[c][2], mot[1].table[c][2]
        print(c, 'MOTP', before['MOTP'], '->', after['MOTP'], ' LocA', hota[0].table[c][2]['LocA'], '->', hota[1].table[c][2]['LocA'])
        assert after['MOTP'] > before['MOTP'] and hota[1].table[c][2]['LocA'] > hota[0].table[c][2]['LocA']
        for f in ('gt', 'tp', 'fn', 'fp', 'idsw'):
            assert after[f] == before[f], (c, f)
        assert before['tp'] == (2 * n if c == 'ALL' else n) and before['fp'] == 0 and before['idsw'] == 0
    assert got['object_id'].tobytes() == out['object_id'].tobytes()


@pytest.mark.parametrize('fixture,cfg', [('sort_g5_input.json', G5), ('sort_g4_input.json', G4)])
def test_cli_writes_the_smoothed_file(golden_dir, tmp_path, fixture, cfg):
    from waymo_2d_tracking_amd.tracking import track, utils as T
    path = os.path.join(golden_dir, fixture)
    base = ['--input', path, '--max-age=2', '--score-threshold=' + ','.join(map(str, cfg['score']))]
    runs = [(['--smooth-window', '2'], {'smooth': smooth_cases.job(window=2, sigma=1.0)}),
            (['--smooth-window=3,1,0,2', '--smooth-sigma=1.5,1.0,1.0,0.7', '--link-gap=6,6,0,6', '--link-iou=0.1', '--link-motion=linear', '--interpolate-gap=2',
              '--min-track-len=3'],
             {'smooth': {'window': [3, 1, 0, 2], 'weights': [smooth_ref.gaussian(s, 4) for s in (1.5, 1.0, 1.0, 0.7)]},
              'stitch': stitch_cases.job(max_link=[6, 6, 0, 6], link_iou=0.1, motion='linear'), 'refine': refine_cases.job(max_gap=2, min_len=3)}),
            (['--smooth-window=1', '--smooth-kernel=box', '--smooth-sigma=7', '--interpolate-gap=2'],
             {'smooth': smooth_cases.job(window=1, kernel='box'), 'refine': refine_cases.job(max_gap=2)})]
    for k, (flags, passes) in enumerate(runs):               # the reference passes run in the order of the command line's, not in the one given here
        expected, refs, out, _ = H._expected_file(path, cfg['score'], cfg['iou'], 2, passes)
        ref, n_tracked, n_rows = refs['smooth'], len(out['frame']), len(refs['smooth']['bbox'])
        if 'g4' in fixture:                                                              # the flags are live on this input
            assert sum(1 for n in ref['pairs'] if n) > 0 and (k != 1 or n_rows != n_tracked)
        for name, extra in (('native%d.json' % k, []), ('python%d.json' % k, ['--python-io'])):
            T.reset_global_ids(0)
            assert track.main(base + flags + ['--output', str(tmp_path / name)] + extra) == 0
        assert (tmp_path / ('python%d.json' % k)).read_text() == json.dumps(expected)
        assert (tmp_path / ('native%d.json' % k)).read_bytes() == (tmp_path / ('python%d.json' % k)).read_bytes()


def test_the_order_of_the_passes_matters_on_the_fixture(golden_dir):
    """stitch -> refine -> smooth is not refine -> smooth -> ... on the g4 input: the CLI test above can tell the orders apart"""
    from waymo_2d_tracking_amd.tracking import utils as T
    path = os.path.join(golden_dir, 'sort_g4_input.json')
    packed = T.pack_streams(T.read_data_file(path, G4['score']))
    rows, _ = T.track_packed(packed, G4['iou'], 2, 0)
    offsets = packed['stream_frame_offsets']
    smooth, refine = smooth_cases.job(window=1, kernel='box'), refine_cases.job(max_gap=2)
    a = smooth_ref.smooth(offsets, arrays(refine_ref.refine(offsets, rows, refine)), smooth)
    b = refine_ref.refine(offsets, with_boxes(rows, smooth_ref.smooth(offsets, rows, smooth)), refine)
    assert len(a['bbox']) == len(b['bbox']) and a['bbox'] != [list(r) for r in b['bbox']]


def test_cli_default_flags_write_what_they_wrote(golden_dir, tmp_path):
    from waymo_2d_tracking_amd.tracking import track
    H.check_cli_default_flags(golden_dir, tmp_path, (['--smooth-window=0', '--smooth-sigma=2.5', '--smooth-kernel=box'], ['--smooth-window=0,0,0,0', '--python-io']),
                              module='waymo_2d_tracking_amd.tracking.smooth')      # with the defaults the module is not even imported
    args = track.build_parser().parse_args([])
    assert args.smooth_window == [0] and args.smooth_sigma == [1.0] and args.smooth_kernel == 'gaussian' and not track.smooths(args)


@pytest.fixture(scope='module')
def sweep_set(tmp_path_factory):
    """detections without classes 1 and 2 in two frames: tracks with holes under max_age 2, so that the refinement axis adds rows"""
    return H.sweep_set(tmp_path_factory, 'smooth_sweep', edit=lambda dets: H.without_frames(dets, (4, 8)))


def test_sweep_with_smooth_grids_equals_the_references(sweep_set):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    path, dets, gt_json = sweep_set
    grid = {'score': [0.3, 0.6], 'iou': [0.01], 'max_age': [2], 'min_hits': [0], 'gap': [0, 2], 'min_len': [1],
            'smooth_window': [0, 1, 2], 'smooth_sigma': [1.0, 2.0]}
    res = E.sweep(path, E.load_ground_truth(gt_json), grid, hota=True)
    assert len(res['settings']) == 24
    assert res['settings'][9] == {'max_age': 2, 'min_hits': 0, 'score': 0.3, 'iou': 0.01, 'interp_gap': 2, 'min_len': 1, 'smooth_window': 1, 'smooth_sigma': 2.0}
    reference = H.sweep_reference(dets, gt_json, lambda s: {'refine': refine_cases.job(max_gap=s['interp_gap'], min_len=s['min_len']),
                                                            'smooth': smooth_cases.job(window=s['smooth_window'], sigma=s['smooth_sigma'])},
                                  metrics=('mot', 'hota'))
    loca = {}
    for k, s in enumerate(res['settings']):
        mot, hota = reference(s)
        # counts equal, sums and table within the bound of their addition order (the module text of mot_support.py)
        assert_hota_equals_reference(res['hota_results'][k], hota)
        for c in E.ALL_CLASSES:
            assert [res['results'][k].table[c][2][f] for f in mot_ref.FIELDS] == [mot[c][2][f] for f in mot_ref.FIELDS], (k, c)
        loca[(s['score'], s['interp_gap'], s['smooth_window'], s['smooth_sigma'])] = hota['table']['ALL'][2]['LocA']
    assert loca[(0.3, 2, 0, 1.0)] == loca[(0.3, 2, 0, 2.0)]                              # window 0: sigma is not read
    assert len(set(loca[(0.3, 2, w, v)] for w in (0, 1, 2) for v in (1.0, 2.0))) >= 3    # the axes are live
    for lv in (1, 2):
        assert len(res['ranked'][lv]) == 1
        for row in res['ranked'][lv]:
            total = dict((f, 0) for f in mot_ref.FIELDS)
            for c in E.ALL_CLASSES:
                i = c - 1
                s = {'max_age': row['max_age'], 'min_hits': row['min_hits'], 'score': row['score_threshold'][i], 'iou': row['iou_threshold'][i],
                     'interp_gap': row['interp_gap'][i], 'min_len': row['min_len'][i], 'smooth_window': row['smooth_window'][i],
                     'smooth_sigma': row['smooth_sigma'][i]}
                for f in mot_ref.FIELDS:
                    total[f] += reference(s)[0][c][lv][f]
            assert row['counts'] == total, (lv, row)
            assert row['smooth_window'][2] == 0 and row['smooth_kernel'] == 'gaussian'
            assert E.flag_line(row).endswith(' --smooth-window=%s --smooth-sigma=%s' % (','.join(map(str, row['smooth_window'])),
                                                                                        ','.join(repr(float(v)) for v in row['smooth_sigma'])))


def test_sweep_with_default_smooth_grids_is_the_sweep_without_them(sweep_set):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    path, _, gt_json = sweep_set
    gt = E.load_ground_truth(gt_json)
    for grid in ({'score': [0.3, 0.6], 'iou': [0.01, 0.1], 'max_age': [1, 3], 'min_hits': [0, 1]},
                 {'score': [0.3], 'iou': [0.01], 'max_age': [1, 3], 'min_hits': [0], 'gap': [0, 1], 'min_len': [1, 2], 'link_gap': [0, 2], 'link_iou': [0.3]}):
        old = E.sweep(path, gt, grid)                                   # no smooth axes: the code path before them
        new = E.sweep(path, gt, dict(grid, smooth_window=[0], smooth_sigma=[1.0, 2.5], smooth_kernel='box'))
        for key in ('settings', 'ranked', 'best'):
            assert json.dumps(old[key], sort_keys=True) == json.dumps(new[key], sort_keys=True)
        assert sorted(old) == sorted(new) and 'smooth_window' not in old['settings'][0] and 'smooth_window' not in old['best'][2]
        assert 'smooth' not in E.flag_line(new['best'][2]) and E.flag_line(new['best'][2]) == E.flag_line(old['best'][2])
    args = E.build_parser().parse_args(['--annotations', 'x'])
    assert args.smooth_window_grid == '0' and args.smooth_sigma_grid == '1.0' and args.smooth_kernel == 'gaussian'
