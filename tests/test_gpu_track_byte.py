"""The tracker's second association with low-score detections on the GPU (wt_track_streams_byte_host through
utils.track_packed_byte) against the CPU reference tests/byte_ref.py, which shares no code with it: frames, categories, ids,
boxes and births are equal, the confidence within the libm-vs-ocml exp() difference test_gpu_sort.py allows (rtol 4e-16).
tests/test_byte_cases.py proves on the CPU that every input reaches the path it is named for."""
import json
import os

import numpy as np
import pytest

import byte_cases as BC
import byte_ref
from waymo_2d_tracking_amd.tracking import utils as T

pytestmark = pytest.mark.gpu


def _gpu(c, id_base=0):
    return T.track_packed_byte(c['packed'], c['iou'], c['max_age'], c['min_hits'], c['score'], c['low_score'], c['low_iou'], id_base)


def _ref(c, id_base=0):
    return byte_ref.track_streams(c['packed'], c['max_age'], c['min_hits'], c['score'], c['iou'], c['low_score'], c['low_iou'], id_base)


def _equal(out, births, ref):
    assert births == ref['n_births']
    for k in ('frame', 'category', 'object_id'):
        assert np.array_equal(out[k], ref[k]), k
    assert np.array_equal(out['bbox'], ref['bbox'], equal_nan=True)
    np.testing.assert_allclose(out['score'], ref['score'], rtol=4e-16, atol=0)


def _check(c, id_base=0):
    ref = _ref(c, id_base)
    for name, least in c['reach'].items():
        assert ref['stats'][name] >= least, (name, ref['stats'])
    out, births = _gpu(c, id_base)
    _equal(out, births, ref)
    return out, births, ref


# ---- 1: nothing low ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fourteen():
    """14 streams x 4 classes, seeded (class 3 given a reachable threshold so that all four classes track)."""
    c = BC.random_streams(11, 3, 10, 25, 2, 0, streams=14)
    c['packed']['category'][::7] = 3
    c['score'], c['iou'], c['low_score'], c['low_iou'] = [0.6, 0.6, 0.5, 0.6], [0.2, 0.1, 0.1, 0.05], [0.3, 0.3, 0.2, 0.3], [0.4, 0.3, 0.3, 0.2]
    return c


@pytest.mark.parametrize('id_base', [0, 1000])
def test_low_equal_to_high_is_track_packed(fourteen, id_base):
    c = fourteen
    want, want_births = T.track_packed(c['packed'], c['iou'], c['max_age'], c['min_hits'], c['score'], id_base)
    got, births = T.track_packed_byte(c['packed'], c['iou'], c['max_age'], c['min_hits'], c['score'], c['score'], c['low_iou'], id_base)
    assert births == want_births > 0 and len(want['frame']) > 200 and set(want['category'].tolist()) == {1, 2, 3, 4}
    assert all(np.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize('id_base', [0, 1000])
def test_no_score_between_low_and_high_is_track_packed(fourteen, id_base):
    c = fourteen
    p = dict(c['packed'])
    high = np.asarray(c['score'])[p['category'] - 1]
    p['score'] = np.where(p['score'] < high, 0.01, p['score'])          # below every low threshold
    want, want_births = T.track_packed(p, c['iou'], c['max_age'], c['min_hits'], c['score'], id_base)
    got, births = T.track_packed_byte(p, c['iou'], c['max_age'], c['min_hits'], c['score'], c['low_score'], c['low_iou'], id_base)
    assert births == want_births > 0
    assert all(np.array_equal(got[k], want[k]) for k in want)


# ---- 2: hand-worked ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(BC.HAND))
def test_hand_worked_cases(name):
    c = BC.HAND[name]()
    out, births, _ = _check(c)
    assert list(zip(out['frame'].tolist(), out['category'].tolist(), out['object_id'].tolist())) == c['rows']
    assert births == c['births']


# ---- 3: threshold edges of the second pass -------------------------------------------------------------------------
@pytest.mark.parametrize('where', ['equal', 'iou_just_below', 'iou_above'])
def test_second_pass_threshold_edges(where):
    v = byte_ref.low_pair_iou(BC.EDGE_TRACK, BC.EDGE_DET)
    thr = {'equal': v, 'iou_just_below': np.nextafter(v, np.float32(1)), 'iou_above': np.nextafter(v, np.float32(0))}[where]
    out, births, ref = _check(BC.edge(float(thr)))
    kept = where != 'iou_just_below'
    assert ref['stats']['second_match'] == int(kept) and ref['stats']['second_reject'] == int(not kept)
    # a rejected pair updates nothing (the track's next box is the reference's) and bears nothing
    assert out['frame'].tolist() == ([0, 1, 2] if kept else [0, 2]) and out['object_id'].tolist() == [1] * (2 + kept) and births == 1


# ---- 4: contested low detections -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['contested_two_tracks', 'contested_two_dets'])
def test_contested_low_detections_break_ties_like_linear_assignment(name):
    out, births, ref = _check(BC.PATHS[name]())
    assert len(out['frame']) == len(ref['frame']) and ref['stats']['second_match'] == 1


# ---- 5: one of the two passes skipped ------------------------------------------------------------------------------
def test_first_pass_skipped_second_runs():
    c = BC.dip()
    _, _, ref = _check(c)
    assert ref['stats']['first_skipped'] == 2


def test_low_detections_with_no_track_left_or_no_track_at_all():
    _, _, ref = _check(BC.high_keeps_track())
    assert ref['stats']['second_run'] == 0 and ref['stats']['second_no_track'] == 1
    _, births, ref = _check(BC.lone_low())
    assert ref['stats']['second_run'] == 0 and births == 1


# ---- 6: wave-width edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_low,n_left', BC.WAVE_EDGES)
def test_wave_width_edges(n_low, n_left):
    _, _, ref = _check(BC.wave_edges(n_low, n_left))
    assert ref['stats']['second_match'] + ref['stats']['second_reject'] == min(n_low, n_left)


# ---- 7: the second cost matrix in global memory --------------------------------------------------------------------
def test_second_cost_matrix_off_lds():
    c = BC.off_lds()
    p = c['packed']
    cap_n = int(np.diff(p['frame_det_offsets']).max())
    assert (len(p['stream_frame_offsets']) - 1) * BC.C4 > 256 and cap_n * ((cap_n * (c['max_age'] + 2)) | 1) > 8192
    assert 100 * (100 | 1) > 8192                                  # n * ld of the second pass against kLdsCostFloats
    _, _, ref = _check(c)
    assert ref['stats']['second_match'] + ref['stats']['second_reject'] == 100


# ---- 8: a class created by a low detection -------------------------------------------------------------------------
def test_class_created_by_a_low_detection_fixes_the_id_order():
    c = BC.low_creates_class()
    out, births, _ = _check(c)
    assert list(zip(out['frame'].tolist(), out['category'].tolist(), out['object_id'].tolist())) == c['rows'] and births == 2


# ---- 9: a non-finite predicted box in a frame with a second pass ---------------------------------------------------
def test_nonfinite_predicted_box_in_a_frame_with_a_second_pass():
    _, _, ref = _check(BC.nonfinite())
    assert ref['stats']['nonfinite_second'] >= 1


# ---- 10: seeded random streams -------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_age,min_hits', BC.AGE_HITS)
def test_random_streams_three(max_age, min_hits):
    c = BC.random_streams(5, 1, 12, 40, max_age, min_hits, streams=3)
    out, births, _ = _check(c, id_base=17)
    again, births2 = _gpu(c, id_base=17)
    assert births2 == births and all(np.array_equal(out[k], again[k], equal_nan=True) for k in out)      # deterministic


@pytest.mark.parametrize('max_age,min_hits', BC.AGE_HITS)
def test_random_streams_three_hundred(max_age, min_hits):
    """300 streams x 4 classes: far past the 256 trackers up to which the plain tracker would take helper waves and the large
    LDS budget."""
    c = BC.random_streams(6, 60, 6, 12, max_age, min_hits)
    assert len(c['packed']['stream_frame_offsets']) - 1 == 300
    c['reach'] = {'second_run': 10, 'second_match': 10}
    out, births, _ = _check(c)
    again, births2 = _gpu(c)
    assert births2 == births and all(np.array_equal(out[k], again[k], equal_nan=True) for k in out)


def test_device_form_equals_host_form():
    """wt_track_streams_byte_dev on tensors in HBM (devpath.DeviceTrackerByte), run twice on one workspace."""
    from waymo_2d_tracking_amd.devpath import DeviceTrackerByte
    c = BC.random_streams(5, 1, 12, 40, 2, 0, streams=3)
    want, want_births = _gpu(c, id_base=5)
    dev = DeviceTrackerByte(c['packed'], c['iou'], c['max_age'], c['min_hits'], c['score'], c['low_score'], c['low_iou'])
    for _ in range(2):
        dev.run(id_base=5)
        got, births = dev.results()
        assert births == want_births and all(np.array_equal(got[k], want[k], equal_nan=True) for k in want)


# ---- 11: the command line ------------------------------------------------------------------------------------------
def _rows(tracks):
    return [(t['image_id'], t['category_id'], t['object_id']) for t in tracks]


def test_cli_with_and_without_the_flag(golden_dir, tmp_path, capsys):
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.tracking import track
    dets = syn.make_sequence_json(9, n_segments=1, n_frames=8, n_objects=12)
    src = tmp_path / 'dets.json'
    src.write_text(json.dumps(dets))
    high, low, iou, low_iou = [0.6, 0.6, 1.0, 0.6], [0.3, 0.3, 1.0, 0.3], [0.2, 0.1, 1.0, 0.05], [0.4] * 4
    packed = T.pack_streams(T.read_data_file(str(src), low))
    out, births = T.track_packed_byte(packed, iou, 2, 0, high, low, low_iou)
    plain, _ = T.track_packed(T.pack_streams(T.read_data_file(str(src), high)), iou, 2, 0, None)
    assert births > 0 and len(out['frame']) > len(plain['frame'])               # the flag changes the result
    want = T.format_tracks(packed, out)
    for extra in ([], ['--python-io']):
        T.reset_global_ids(0)
        dst = tmp_path / ('tracks%d.json' % len(extra))
        assert track.main(['--input', str(src), '--output', str(dst), '--max-age=2', '--min-hits=0', '--score-threshold=0.6,0.6,1.0,0.6',
                           '--iou-threshold=0.2,0.1,1.0,0.05', '--low-score-threshold=0.3,0.3,1.0,0.3', '--low-iou-threshold=0.4'] + extra) == 0
        assert json.load(open(dst)) == want
    # flags absent: today's golden
    exp = json.load(open(os.path.join(golden_dir, 'sort_g4_expected_a.json')))
    T.reset_global_ids(0)
    dst = tmp_path / 'golden.json'
    assert track.main(['--input', os.path.join(golden_dir, 'sort_g4_input.json'), '--output', str(dst), '--max-age=2', '--min-hits=0',
                       '--score-threshold=0.3,0.3,1.0,0.2', '--iou-threshold=0.01,0.01,1.0,0.0']) == 0
    assert _rows(json.load(open(dst))) == _rows(exp['tracks'])
    capsys.readouterr()


# ---- 12: the sweep -------------------------------------------------------------------------------------------------
def test_sweep_low_score_grid(tmp_path):
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.tracking import evaluate as E
    dets, gt = syn.make_tracking_json(4, n_segments=1, n_frames=10, n_objects=12)
    src, ann = tmp_path / 'dets.json', tmp_path / 'gt.json'
    src.write_text(json.dumps(dets))
    ann.write_text(json.dumps(gt))
    gt = E.load_ground_truth(str(ann))
    grid = {'score': [0.3, 0.7], 'iou': [0.1], 'max_age': [1], 'min_hits': [0]}
    plain = E.sweep(str(src), gt, grid)
    both = E.sweep(str(src), gt, dict(grid, low_score=[0.3], low_iou=[0.5]))
    assert [(s['score'], s['low_score'], s['low_iou']) for s in both['settings']] == [(0.3, 0.3, 0.5), (0.7, 0.3, 0.5)]
    assert 'low_score' not in plain['settings'][0]
    # low clamped to its high: the plain row's counts
    assert both['results'][0].as_json() == plain['results'][0].as_json()
    assert both['results'][1].as_json() != plain['results'][1].as_json()
    best = both['best'][2]
    assert len(best['low_score_threshold']) == 4 and all(lo <= hi for lo, hi in zip(best['low_score_threshold'], best['score_threshold']))
    assert '--low-score-threshold=' in E.flag_line(best) and '--low-iou-threshold=' in E.flag_line(best)
    assert '--low-score-threshold' not in E.flag_line(plain['best'][2])
