"""What wt_split_tracks_host refuses before it touches a device (no GPU): the status code and the wt_last_error() text of the
layout and job checks of csrc/split_host.h, reached through tracking/split.py's own argument marshalling; and what
tracking/split.py refuses before it calls the library."""
import numpy as np
import pytest

import split_cases
from track_stage_support import arrays, packed_for

INVALID = 1


def _modules():
    from waymo_2d_tracking_amd import build
    build.build(verbose=False)
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import split
    return _lib, split


ROWS = [(0, 1, [0, 0, 5, 5], 0.5, 1), (3, 1, [0, 0, 5, 5], 0.5, 2), (4, 1, [0, 0, 5, 5], 0.5, 3), (4, 1, [9, 9, 5, 5], 0.5, 2)]


def prepared(split):
    """two streams of three slots; stream 1 holds trajectory 0 at slots 3 and 4 and trajectory 1 at slot 4: local = [0, 0, 1, 0]"""
    p = split._prepare(packed_for([0, 3, 6]), [arrays(split_cases.result(ROWS))], [split_cases.job(0.3, 2)], 4)
    assert p['local'].tolist() == [0, 0, 1, 0] and p['n_traj'].tolist() == [[1, 2]] and p['n_traj_total'] == 3 and p['first_new_id'] == [4]
    outputs = [np.zeros((1, 4), np.int32), np.zeros((1, 4), np.int64), np.zeros((1, 4, 2)), np.zeros((1, 3), np.int32), np.zeros((1, 2), np.int64)]
    return p, outputs


def refused(_lib, split, p, outputs, text):
    assert split._host_call(p, outputs) == INVALID
    message = _lib.lib().wt_last_error().decode()
    assert text in message, message


def test_job_parameters_are_checked_by_the_entry_point():
    _lib, split = _modules()
    for name, index, value, text in (('job_split_iou', (0, 2), np.nan, 'job 0: split_iou of class 3 is NaN'),
                                     ('job_split_gap', (0, 1), -1, 'job 0: split_gap of class 2 is negative'),
                                     ('job_motion', 0, 2, 'job 0: motion must be 0 (hold) or 1 (linear)'),
                                     ('job_motion', 0, -1, 'job 0: motion must be 0 (hold) or 1 (linear)'),
                                     ('job_result', 0, 1, 'job 0: result 1 outside 0..0'),
                                     ('job_result', 0, -1, 'job 0: result -1 outside 0..0')):
        p, outputs = prepared(split)
        p[name][index] = value
        refused(_lib, split, p, outputs, text)


def test_layout_is_checked_by_the_entry_point():
    _lib, split = _modules()
    p, outputs = prepared(split)
    p['local'][3] = 1
    refused(_lib, split, p, outputs, 'result 0: trajectory 1 occurs twice in frame 4')
    p, outputs = prepared(split)
    p['local'][3] = 2
    refused(_lib, split, p, outputs, 'result 0, row 3: trajectory index 2 outside 0..1')
    p, outputs = prepared(split)
    p['n_traj'][0, 1] = -1
    refused(_lib, split, p, outputs, 'result 0, stream 1: negative trajectory count')
    p, outputs = prepared(split)
    p['category'][2] = 5
    refused(_lib, split, p, outputs, 'category 5 outside 1..4')
    p, outputs = prepared(split)
    p['stream_frame_offsets'][2] = 5
    refused(_lib, split, p, outputs, 'wt_split_tracks_host: CSR offsets do not cover the rows')
    p, outputs = prepared(split)
    p['frame_row_offsets'][0, 2] = 0
    refused(_lib, split, p, outputs, 'result 0: frame_row_offsets must be non-decreasing')
    for missing in range(5):
        p, outputs = prepared(split)
        outputs[missing] = None
        refused(_lib, split, p, outputs, 'wt_split_tracks_host: bad argument')


def test_python_layer_refuses_before_it_calls():
    _lib, split = _modules()
    packed, out = packed_for([0, 3, 6]), arrays(split_cases.result(ROWS))
    with pytest.raises(ValueError, match='split_iou must not be NaN'):
        split.split_tracks(packed, [out], [{'split_iou': float('nan')}])
    with pytest.raises(ValueError, match='split_gap must be >= 0'):
        split.split_tracks(packed, [out], [{'split_gap': [1, -1, 1, 1]}])
    with pytest.raises(ValueError, match='one value, or one per class'):
        split.split_tracks(packed, [out], [{'split_iou': [0.3, 0.3]}])
    with pytest.raises(KeyError):
        split.split_tracks(packed, [out], [{'split_iou': 0.3, 'motion': 'quadratic'}])
    with pytest.raises(ValueError, match='names a result outside'):
        split.split_tracks(packed, [out], [{'split_iou': 0.3, 'result': 1}])
    with pytest.raises(ValueError, match='at least one result'):
        split.split_tracks(packed, [], [{'split_iou': 0.3}])
    with pytest.raises(ValueError, match='result 0: object ids must be integers'):
        split.split_tracks(packed, [arrays(split_cases.result(ROWS), np.float64)], [{'split_iou': 0.3}])
    with pytest.raises(ValueError, match='result 0: object ids must be integers'):
        split.split_tracks(packed, [dict(out, object_id=np.asarray(['a', 'b', 'c', 'b']))], [{'split_iou': 0.3}])
    twice = arrays(split_cases.result(ROWS + [(4, 1, [1, 1, 5, 5], 0.5, 3)]))
    with pytest.raises(_lib.WaymoTrackError, match=r'wt_split_tracks failed: WT_ERR_INVALID \(result 0: object_id 3 occurs twice in image seg1/15/FRONT\)'):
        split.split_tracks(packed, [twice], [split_cases.job(0.3)])
    # a setting that splits nothing is the input itself, and nothing is called
    assert split.split_one(packed, out, 0.0) is out and split.split_one(packed, out, [0.0, -1.0, 0.0, 0.0], [0, 0, 0, 0], 'hold') is out


def test_new_ids_must_fit_the_id_dtype():
    """_job_dicts on outputs as the library would write them: a row of a new piece gets first_new_id + its number"""
    _lib, split = _modules()
    packed = packed_for([0, 3, 6])
    for dtype, first, fits in ((np.int8, 126, True), (np.int8, 127, False), (np.int64, None, True), (np.uint8, 254, True), (np.uint8, 255, False),
                               (np.uint8, -1, False)):
        out = arrays(split_cases.result(ROWS), dtype)
        job = dict(split_cases.job(0.3), **({} if first is None else {'first_new_id': first}))
        p = split._prepare(packed, [out], [job], 4)
        piece = np.asarray([[0, 0, 1, 1]], np.int32)
        new = np.asarray([[-1, -1, 0, 1]], np.int64)
        args = (p, [out], piece, new, np.full((1, 4, 2), -1.0), np.asarray([[0, 1, 1]], np.int32), np.asarray([[0, 2]], np.int64))
        if fits:
            got = split._job_dicts(*args)[0]
            start = 4 if first is None else first
            assert got['object_id'].dtype == dtype and got['object_id'].tolist() == [1, 2, start, start + 1] and got['n_new'] == 2
        else:
            with pytest.raises(ValueError, match='do not fit the object ids'):
                split._job_dicts(*args)


def test_workspace_is_linear_in_rows_and_in_jobs_times_trajectories():
    _lib, split = _modules()
    import ctypes as C
    ws = lambda J, nr, nt, mt: int(_lib.lib().wt_split_tracks_workspace(C.c_int32(J), C.c_int32(40), C.c_int64(nr), C.c_int64(nt), C.c_int64(mt)))
    limit = C.c_int32(0)
    _lib.lib().wt_split_tracks_limits(C.byref(limit))
    assert 64 < limit.value <= 4096
    small = ws(64, 300000, 40000, limit.value)
    assert 0 < small <= 4 * 4 * 300001 + 64 * 40000 * 4 + 4096                # four link columns per row, one int32 per (job, trajectory)
    assert ws(1, 300000, 40000, limit.value) < small
    big = ws(64, 300000, 40000, limit.value + 1)
    assert small < big <= small + 2 * 4 * 40000 + 4096                         # beyond the limit: the link table of every trajectory
    assert ws(-1, 1, 1, 1) == 0 and ws(1, -1, 1, 1) == 0
