"""What wt_dedup_tracks_host refuses before it touches a device (no GPU): the status code and the wt_last_error() text of the
layout and job checks of csrc/dedup_host.h, reached through tracking/dedup.py's own argument marshalling; and what
tracking/dedup.py refuses before it calls the library."""
import numpy as np
import pytest

import dedup_cases
from track_stage_support import arrays, packed_for

INVALID = 1


def _modules():
    from waymo_2d_tracking_amd import build
    build.build(verbose=False)
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import dedup
    return _lib, dedup


ROWS = [(0, 1, [0, 0, 5, 5], 0.5, 1), (3, 1, [0, 0, 5, 5], 0.5, 2), (4, 1, [0, 0, 5, 5], 0.5, 3), (4, 1, [9, 9, 5, 5], 0.5, 2)]


def prepared(dedup):
    """two streams of three slots; stream 1 holds trajectory 0 at slots 3 and 4 and trajectory 1 at slot 4: local = [0, 0, 1, 0]"""
    p = dedup._prepare(packed_for([0, 3, 6]), [arrays(dedup_cases.result(ROWS))], [dedup_cases.job(min_frames=1)], 4)
    assert p['local'].tolist() == [0, 0, 1, 0] and p['n_traj'].tolist() == [[1, 2]] and p['n_traj_total'] == 3
    assert p['traj_ids'][0].tolist() == [1, 2, 3] and p['job_dup_iou'].tolist() == [[0.7] * 4] and p['job_dup_frac'].tolist() == [[0.5] * 4]
    outputs = [np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32), np.zeros((1, 4), np.int32), np.zeros((1, 2), np.int64)]
    return p, outputs


def refused(_lib, dedup, p, outputs, text):
    assert dedup._host_call(p, outputs) == INVALID
    message = _lib.lib().wt_last_error().decode()
    assert text in message, message


def test_job_parameters_are_checked_by_the_entry_point():
    _lib, dedup = _modules()
    for name, index, value, text in (('job_dup_iou', (0, 2), np.nan, 'job 0: dup_iou of class 3 is NaN'),
                                     ('job_min_frames', (0, 1), -1, 'job 0: min_frames of class 2 is negative'),
                                     ('job_dup_frac', (0, 0), 1.5, 'job 0: dup_frac of class 1 is outside 0..1'),
                                     ('job_dup_frac', (0, 3), -0.25, 'job 0: dup_frac of class 4 is outside 0..1'),
                                     ('job_dup_frac', (0, 1), np.nan, 'job 0: dup_frac of class 2 is outside 0..1'),
                                     ('job_result', 0, 1, 'job 0: result 1 outside 0..0')):
        p, outputs = prepared(dedup)
        p[name][index] = value
        refused(_lib, dedup, p, outputs, text)


def test_layout_is_checked_by_the_entry_point():
    _lib, dedup = _modules()
    p, outputs = prepared(dedup)
    p['local'][3] = 1
    refused(_lib, dedup, p, outputs, 'result 0: trajectory 1 occurs twice in frame 4')
    p, outputs = prepared(dedup)
    p['local'][1:] = [1, 0, 1]
    refused(_lib, dedup, p, outputs, 'result 0, row 1: trajectory index 1 before 0 appeared (indices number the trajectories by first appearance)')
    p, outputs = prepared(dedup)
    p['n_traj'][0, 0] = 2
    refused(_lib, dedup, p, outputs, 'result 0, stream 0: 2 trajectories declared, 1 occur')
    p, outputs = prepared(dedup)
    p['category'][2] = 5
    refused(_lib, dedup, p, outputs, 'category 5 outside 1..4')
    for bad in (np.nan, np.inf, -np.inf):
        p, outputs = prepared(dedup)
        p['score'][2] = bad
        refused(_lib, dedup, p, outputs, 'result 0, row 2: score is not finite')
    p, outputs = prepared(dedup)
    p['stream_frame_offsets'][2] = 5
    refused(_lib, dedup, p, outputs, 'wt_dedup_tracks_host: CSR offsets do not cover the rows')
    p, outputs = prepared(dedup)
    outputs[3] = None
    refused(_lib, dedup, p, outputs, 'wt_dedup_tracks_host: bad argument')


def test_python_layer_refuses_before_it_calls():
    _lib, dedup = _modules()
    packed, out = packed_for([0, 3, 6]), arrays(dedup_cases.result(ROWS))
    with pytest.raises(ValueError, match='dup_iou must not be NaN'):
        dedup.dedup_tracks(packed, [out], [{'min_frames': 1, 'dup_iou': float('nan')}])
    with pytest.raises(ValueError, match='min_frames must be >= 0'):
        dedup.dedup_tracks(packed, [out], [{'min_frames': [1, -1, 1, 1]}])
    for frac in (1.5, -0.1, float('nan')):
        with pytest.raises(ValueError, match=r'dup_frac must be in 0\.\.1'):
            dedup.dedup_tracks(packed, [out], [{'min_frames': 1, 'dup_frac': frac}])
    with pytest.raises(ValueError, match='one value, or one per class'):
        dedup.dedup_tracks(packed, [out], [{'min_frames': [1, 1]}])
    with pytest.raises(ValueError, match='names a result outside'):
        dedup.dedup_tracks(packed, [out], [{'min_frames': 1, 'result': 1}])
    twice = arrays(dedup_cases.result(ROWS + [(4, 1, [1, 1, 5, 5], 0.5, 3)]))
    with pytest.raises(_lib.WaymoTrackError, match=r'wt_dedup_tracks failed: WT_ERR_INVALID \(result 0: object_id 3 occurs twice in image seg1/15/FRONT\)'):
        dedup.dedup_tracks(packed, [twice], [dedup_cases.job(min_frames=1)])
    # a setting that drops nothing is the input itself, and nothing is called
    assert dedup.dedup_one(packed, out, [0, 0, 0, 0]) is out


def test_track_flags_default_to_off():
    from waymo_2d_tracking_amd.tracking import track
    args = track.build_parser().parse_args([])
    assert args.dedup_frames == [0] and args.dedup_iou == [0.7] and args.dedup_frac == [0.5]
    assert not track.dedups(args) and track.dedups(track.build_parser().parse_args(['--dedup-frames', '0,3,0,0']))
    assert track.post_passes(args, None, 'the rows') == 'the rows'                          # nothing is imported or called


def test_workspace_depends_on_the_five_sizes_only():
    _lib, dedup = _modules()
    import ctypes as C
    ws = lambda J, nt, mt, S=40, nr=300000: int(_lib.lib().wt_dedup_tracks_workspace(C.c_int32(J), C.c_int32(S), C.c_int64(nr), C.c_int64(nt), C.c_int64(mt)))
    small = ws(64, 40000, 1000)
    assert 0 < small <= 4 * 64 * 40 + 24 * 40001 + 12 * 300001 + 8192                       # up to the LDS limit: the summary, shared by all jobs
    big = ws(64, 40000, 2000)
    assert small < big <= small + 64 * 40000 * 12 + 4096                                    # beyond it: 12 bytes per (job, trajectory)
    assert ws(-1, 1, 1) == 0
    limit = C.c_int32(0)
    _lib.lib().wt_dedup_tracks_limits(C.byref(limit))
    assert 64 < limit.value <= 4096
