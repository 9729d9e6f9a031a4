"""What wt_smooth_tracks_host refuses before it touches a device (no GPU): the status code and the wt_last_error() text of the
layout and job checks of csrc/smooth_host.h, reached through tracking/smooth.py's own argument marshalling; and what
tracking/smooth.py refuses before it calls the library."""
import ctypes as C

import numpy as np
import pytest

import smooth_cases
from track_stage_support import arrays, packed_for

INVALID = 1


def _modules():
    from waymo_2d_tracking_amd import build
    build.build(verbose=False)
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import smooth
    return _lib, smooth


ROWS = [(0, 1, [0, 0, 5, 5], 0.5, 1), (3, 1, [0, 0, 5, 5], 0.5, 2), (4, 1, [0, 0, 5, 5], 0.5, 3), (4, 1, [9, 9, 5, 5], 0.5, 2)]


def prepared(smooth):
    """two streams of three slots; stream 1 holds trajectory 0 at slots 3 and 4 and trajectory 1 at slot 4: local = [0, 0, 1, 0]"""
    p = smooth._prepare(packed_for([0, 3, 6]), [arrays(smooth_cases.result(ROWS))], [smooth_cases.job(window=2)], 4)
    assert p['local'].tolist() == [0, 0, 1, 0] and p['n_traj'].tolist() == [[1, 2]] and p['n_weights'] == 3
    assert p['job_row_offsets'].tolist() == [0, 4] and p['job_weights'].shape == (1, 4, 3)
    return p, [np.zeros((4, 4), np.float64), np.zeros(4, np.int32)]


def refused(_lib, smooth, p, outputs, text):
    assert smooth._host_call(p, outputs) == INVALID
    message = _lib.lib().wt_last_error().decode()
    assert text in message, message


def test_job_parameters_are_checked_by_the_entry_point():
    _lib, smooth = _modules()
    for name, index, value, text in (('job_window', (0, 1), -1, 'job 0: window -1 of class 2 outside 0..32'),
                                     ('job_window', (0, 3), 33, 'job 0: window 33 of class 4 outside 0..32'),
                                     ('job_window', (0, 2), 3, 'job 0: window 3 of class 3 needs 4 weights, 3 given'),
                                     ('job_weights', (0, 2, 1), np.nan, 'job 0: weight 1 of class 3 is not finite'),
                                     ('job_weights', (0, 0, 2), np.inf, 'job 0: weight 2 of class 1 is not finite'),
                                     ('job_weights', (0, 1, 1), -0.5, 'job 0: weight 1 of class 2 is negative'),
                                     ('job_weights', (0, 3, 0), 0.0, 'job 0: weight 0 of class 4 must be above 0'),
                                     ('job_result', 0, 1, 'job 0: result 1 outside 0..0')):
        p, outputs = prepared(smooth)
        p[name][index] = value
        refused(_lib, smooth, p, outputs, text)


def test_layout_is_checked_by_the_entry_point():
    _lib, smooth = _modules()
    p, outputs = prepared(smooth)
    p['local'][3] = 1
    refused(_lib, smooth, p, outputs, 'result 0: trajectory 1 occurs twice in frame 4')
    p, outputs = prepared(smooth)
    p['local'][2] = 2
    refused(_lib, smooth, p, outputs, 'result 0, row 2: trajectory index 2 outside 0..1')
    p, outputs = prepared(smooth)
    p['n_traj'][0, 1] = -1
    refused(_lib, smooth, p, outputs, 'result 0, stream 1: negative trajectory count')
    p, outputs = prepared(smooth)
    p['category'][2] = 5
    refused(_lib, smooth, p, outputs, 'result 0, row 2: category 5 outside 1..4')
    p, outputs = prepared(smooth)
    p['frame_row_offsets'][0, 4] = 0
    refused(_lib, smooth, p, outputs, 'result 0: frame_row_offsets must be non-decreasing')
    p, outputs = prepared(smooth)
    p['stream_frame_offsets'][2] = 5
    refused(_lib, smooth, p, outputs, 'wt_smooth_tracks_host: CSR offsets do not cover the rows')
    p, outputs = prepared(smooth)
    p['n_weights'] = 0
    refused(_lib, smooth, p, outputs, 'wt_smooth_tracks_host: bad argument')
    p, outputs = prepared(smooth)
    outputs[1] = None
    refused(_lib, smooth, p, outputs, 'wt_smooth_tracks_host: bad argument')


def test_python_layer_refuses_before_it_calls():
    _lib, smooth = _modules()
    packed, out = packed_for([0, 3, 6]), arrays(smooth_cases.result(ROWS))
    with pytest.raises(ValueError, match='window must be in 0..32'):
        smooth.smooth_tracks(packed, [out], [{'window': 33}])
    with pytest.raises(ValueError, match='window must be in 0..32'):
        smooth.smooth_tracks(packed, [out], [{'window': [1, -1, 1, 1]}])
    with pytest.raises(ValueError, match='one value, or one per class'):
        smooth.smooth_tracks(packed, [out], [{'window': [1, 1]}])
    with pytest.raises(ValueError, match='a window of 3 needs 4 weights, 3 given'):
        smooth.smooth_tracks(packed, [out], [{'window': 3, 'weights': [1.0, 0.5, 0.25]}])
    with pytest.raises(ValueError, match='weights must be finite'):
        smooth.smooth_tracks(packed, [out], [{'window': 1, 'weights': [1.0, float('nan')]}])
    with pytest.raises(ValueError, match='the first one > 0'):
        smooth.smooth_tracks(packed, [out], [{'window': 1, 'weights': [0.0, 1.0]}])
    with pytest.raises(ValueError, match="kernel must be 'gaussian' or 'box'"):
        smooth.smooth_tracks(packed, [out], [{'window': 1, 'kernel': 'triangle'}])
    with pytest.raises(ValueError, match='sigma must be a positive number'):
        smooth.smooth_tracks(packed, [out], [{'window': 1, 'sigma': 0.0}])
    with pytest.raises(ValueError, match='names a result outside'):
        smooth.smooth_tracks(packed, [out], [{'window': 1, 'result': 1}])
    twice = arrays(smooth_cases.result(ROWS + [(4, 1, [1, 1, 5, 5], 0.5, 3)]))
    with pytest.raises(_lib.WaymoTrackError, match=r'wt_smooth_tracks failed: WT_ERR_INVALID \(result 0: object_id 3 occurs twice in image seg1/15/FRONT\)'):
        smooth.smooth_tracks(packed, [twice], [smooth_cases.job(window=1)])
    # a setting that smooths nothing is the input itself, and nothing is called
    assert smooth.smooth_one(packed, out, [0, 0, 0, 0]) is out and smooth.smooth_one(packed, out, 0, sigma=2.0, kernel='box') is out


def test_weights_are_computed_on_the_host_as_the_definition_says():
    import math
    _lib, smooth = _modules()
    packed, out = packed_for([0, 3, 6]), arrays(smooth_cases.result(ROWS))
    p = smooth._prepare(packed, [out], [{'window': [3, 1, 0, 2], 'sigma': [1.5, 1.0, 1.0, 0.5]}, {'window': 1, 'kernel': 'box'},
                                         {'window': 2, 'weights': [1.0, 0.5, 0.25, 0.125, 0.0625]}], 4)
    assert p['n_weights'] == 5 and p['job_weights'].shape == (3, 4, 5)
    assert p['job_weights'][0, 0].tolist() == [math.exp(-(d * d) / (2.0 * 1.5 * 1.5)) for d in range(4)] + [0.0]
    assert p['job_weights'][0, 3].tolist() == [math.exp(-(d * d) / (2.0 * 0.5 * 0.5)) for d in range(4)] + [0.0]
    assert p['job_weights'][1].tolist() == [[1.0, 1.0, 0.0, 0.0, 0.0]] * 4
    assert p['job_weights'][2, 2].tolist() == [1.0, 0.5, 0.25, 0.125, 0.0625]
    assert p['job_window'].tolist() == [[3, 1, 0, 2], [1, 1, 1, 1], [2, 2, 2, 2]] and p['job_row_offsets'].tolist() == [0, 4, 8, 12]


def test_workspace_does_not_grow_with_the_jobs():
    _lib, smooth = _modules()
    ws = lambda J, nr, nt, mt: int(_lib.lib().wt_smooth_tracks_workspace(C.c_int32(J), C.c_int32(40), C.c_int64(nr), C.c_int64(nt), C.c_int64(mt)))
    small = ws(64, 300000, 40000, 1000)
    assert 0 < small <= 4 * 4 * 300001 + 4096                                  # four int32 per row, shared by all jobs
    assert ws(1, 300000, 40000, 1000) == small
    big = ws(64, 300000, 40000, 2000)
    assert small < big <= small + 2 * 4 * 40000 + 4096                         # beyond the LDS limit: the link table, 8 bytes per trajectory
    assert ws(-1, 1, 1, 1) == 0
    limit = C.c_int32(0)
    _lib.lib().wt_smooth_tracks_limits(C.byref(limit))
    assert 64 < limit.value <= 4096
