"""What wt_stitch_tracks_host refuses before it touches a device (no GPU): the status code and the wt_last_error() text of the
layout and job checks of csrc/stitch_host.h, reached through tracking/stitch.py's own argument marshalling; and what
tracking/stitch.py refuses before it calls the library."""
import numpy as np
import pytest

import stitch_cases
from track_stage_support import arrays, packed_for

INVALID = 1


def _modules():
    from waymo_2d_tracking_amd import build
    build.build(verbose=False)
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import stitch
    return _lib, stitch


ROWS = [(0, 1, [0, 0, 5, 5], 0.5, 1), (3, 1, [0, 0, 5, 5], 0.5, 2), (4, 1, [0, 0, 5, 5], 0.5, 3), (4, 1, [9, 9, 5, 5], 0.5, 2)]


def prepared(stitch):
    """two streams of three slots; stream 1 holds trajectory 0 at slots 3 and 4 and trajectory 1 at slot 4: local = [0, 0, 1, 0]"""
    p = stitch._prepare(packed_for([0, 3, 6]), [arrays(stitch_cases.result(ROWS))], [stitch_cases.job(max_link=1)], 4)
    assert p['local'].tolist() == [0, 0, 1, 0] and p['n_traj'].tolist() == [[1, 2]] and p['n_traj_total'] == 3
    outputs = [np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32), np.zeros((1, 3)), np.zeros((1, 4), np.int32), np.zeros((1, 2), np.int64)]
    return p, outputs


def refused(_lib, stitch, p, outputs, text):
    assert stitch._host_call(p, outputs) == INVALID
    message = _lib.lib().wt_last_error().decode()
    assert text in message, message


def test_job_parameters_are_checked_by_the_entry_point():
    _lib, stitch = _modules()
    for name, index, value, text in (('job_link_iou', (0, 2), np.nan, 'job 0: link_iou of class 3 is NaN'),
                                     ('job_max_link', (0, 1), -1, 'job 0: max_link of class 2 is negative'),
                                     ('job_motion', 0, 2, 'job 0: motion must be 0 (hold) or 1 (linear)'),
                                     ('job_result', 0, 1, 'job 0: result 1 outside 0..0')):
        p, outputs = prepared(stitch)
        p[name][index] = value
        refused(_lib, stitch, p, outputs, text)


def test_layout_is_checked_by_the_entry_point():
    _lib, stitch = _modules()
    p, outputs = prepared(stitch)
    p['local'][3] = 1
    refused(_lib, stitch, p, outputs, 'result 0: trajectory 1 occurs twice in frame 4')
    p, outputs = prepared(stitch)
    p['local'][1:] = [1, 0, 1]
    refused(_lib, stitch, p, outputs, 'result 0, row 1: trajectory index 1 before 0 appeared (indices number the trajectories by first appearance)')
    p, outputs = prepared(stitch)
    p['n_traj'][0, 0] = 2
    refused(_lib, stitch, p, outputs, 'result 0, stream 0: 2 trajectories declared, 1 occur')
    p, outputs = prepared(stitch)
    p['category'][2] = 5
    refused(_lib, stitch, p, outputs, 'category 5 outside 1..4')
    p, outputs = prepared(stitch)
    p['stream_frame_offsets'][2] = 5
    refused(_lib, stitch, p, outputs, 'wt_stitch_tracks_host: CSR offsets do not cover the rows')
    p, outputs = prepared(stitch)
    outputs[3] = None
    refused(_lib, stitch, p, outputs, 'wt_stitch_tracks_host: bad argument')


def test_python_layer_refuses_before_it_calls():
    _lib, stitch = _modules()
    packed, out = packed_for([0, 3, 6]), arrays(stitch_cases.result(ROWS))
    with pytest.raises(ValueError, match='link_iou must not be NaN'):
        stitch.stitch_tracks(packed, [out], [{'max_link': 1, 'link_iou': float('nan')}])
    with pytest.raises(ValueError, match='max_link must be >= 0'):
        stitch.stitch_tracks(packed, [out], [{'max_link': [1, -1, 1, 1]}])
    with pytest.raises(ValueError, match='one value, or one per class'):
        stitch.stitch_tracks(packed, [out], [{'max_link': [1, 1]}])
    with pytest.raises(KeyError):
        stitch.stitch_tracks(packed, [out], [{'max_link': 1, 'motion': 'quadratic'}])
    with pytest.raises(ValueError, match='names a result outside'):
        stitch.stitch_tracks(packed, [out], [{'max_link': 1, 'result': 1}])
    twice = arrays(stitch_cases.result(ROWS + [(4, 1, [1, 1, 5, 5], 0.5, 3)]))
    with pytest.raises(_lib.WaymoTrackError, match=r'wt_stitch_tracks failed: WT_ERR_INVALID \(result 0: object_id 3 occurs twice in image seg1/15/FRONT\)'):
        stitch.stitch_tracks(packed, [twice], [stitch_cases.job(max_link=1)])
    # a setting that links nothing is the input itself, and nothing is called
    assert stitch.stitch_one(packed, out, [0, 0, 0, 0]) is out


def test_workspace_is_linear_in_jobs_times_trajectories():
    _lib, stitch = _modules()
    import ctypes as C
    ws = lambda J, nt, mt: int(_lib.lib().wt_stitch_tracks_workspace(C.c_int32(J), C.c_int32(40), C.c_int64(300000), C.c_int64(nt), C.c_int64(mt)))
    small = ws(64, 40000, 1000)
    assert 0 < small <= 7 * 4 * 40001 + 4096                                   # up to the LDS limit: the summary alone, shared by all jobs
    assert ws(1, 40000, 1000) == small
    big = ws(64, 40000, 2000)
    assert small < big <= small + 64 * 40000 * 36 + 4096                       # beyond it: 36 bytes per (job, trajectory)
    assert ws(-1, 1, 1) == 0
    limit = C.c_int32(0)
    _lib.lib().wt_stitch_tracks_limits(C.byref(limit))
    assert 64 < limit.value <= 4096
