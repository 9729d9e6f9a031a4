"""What wt_xclass_tracks_host refuses before it touches a device (no GPU): the status code and the wt_last_error() text of the
layout and job checks of csrc/xclass_host.h, reached through tracking/xclass.py's own argument marshalling; and what
tracking/xclass.py and the flags of tracking/track.py refuse or leave alone before anything is called."""
import numpy as np
import pytest

import dedup_cases
import xclass_cases
from track_stage_support import arrays, packed_for

INVALID = 1


def _modules():
    from waymo_2d_tracking_amd import build
    build.build(verbose=False)
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import xclass
    return _lib, xclass


ROWS = [(0, 2, [0, 0, 5, 5], 0.5, 1), (3, 2, [0, 0, 5, 5], 0.5, 2), (4, 4, [0, 0, 5, 5], 0.5, 3), (4, 2, [9, 9, 5, 5], 0.5, 2)]
JOB = xclass_cases.job({(2, 4): (3, 0.9, 0.5), (1, 1): (2, 0.6, 0.25)}, prio=[0, 0, 0, 1])


def prepared(xclass):
    """two streams of three slots; stream 1 holds trajectory 0 at slots 3 and 4 and trajectory 1 at slot 4: local = [0, 0, 1, 0]"""
    p = xclass._prepare(packed_for([0, 3, 6]), [arrays(dedup_cases.result(ROWS))], [JOB], 4)
    assert p['local'].tolist() == [0, 0, 1, 0] and p['n_traj'].tolist() == [[1, 2]] and p['n_traj_total'] == 3
    outputs = [np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32), np.zeros((1, 4), np.int32), np.zeros((1, 2), np.int64)]
    return p, outputs


def refused(_lib, xclass, p, outputs, text):
    assert xclass._host_call(p, outputs) == INVALID
    message = _lib.lib().wt_last_error().decode()
    assert text in message, message


def test_python_layer_builds_symmetric_tables():
    _lib, xclass = _modules()
    p, _ = prepared(xclass)
    frames, overlap, frac = p['job_pair_frames'][0], p['job_pair_overlap'][0], p['job_pair_frac'][0]
    assert frames.dtype == np.int32 and overlap.dtype == np.float64 and frames.shape == (4, 4)
    assert frames.tolist() == [[2, 0, 0, 0], [0, 0, 0, 3], [0, 0, 0, 0], [0, 3, 0, 0]]
    assert (frames == frames.T).all() and overlap.tobytes() == overlap.T.copy().tobytes() and frac.tobytes() == frac.T.copy().tobytes()
    assert overlap[1, 3] == 0.9 and overlap[0, 0] == 0.6 and frac[3, 1] == 0.5 and frac[0, 0] == 0.25 and overlap[2, 2] == 0.7
    assert p['job_class_prio'].tolist() == [[0, 0, 0, 1]] and p['job_measure'].tolist() == [1] and p['traj_ids'][0].tolist() == [1, 2, 3]
    q = xclass._prepare(packed_for([0, 3, 6]), [arrays(dedup_cases.result(ROWS))], [{'pairs': {(4, 2): {}}, 'measure': 'iou'}], 4)
    assert q['job_pair_frames'][0, 1, 3] == q['job_pair_frames'][0, 3, 1] == 3 and q['job_measure'].tolist() == [0] and q['job_class_prio'].tolist() == [[0] * 4]


def test_job_parameters_are_checked_by_the_entry_point():
    _lib, xclass = _modules()
    for name, cells, value, text in (
            ('job_pair_frames', [(0, 1, 3)], 4, 'job 0: pair (2, 4) and pair (4, 2) differ (the tables must be symmetric)'),
            ('job_pair_overlap', [(0, 3, 1)], np.nextafter(0.9, 1.0), 'job 0: pair (2, 4) and pair (4, 2) differ'),
            ('job_pair_frac', [(0, 0, 2)], 0.25, 'job 0: pair (1, 3) and pair (3, 1) differ'),
            ('job_pair_overlap', [(0, 1, 3), (0, 3, 1)], np.nan, 'job 0: overlap of pair (2, 4) is NaN'),
            ('job_pair_overlap', [(0, 2, 2)], np.nan, 'job 0: overlap of pair (3, 3) is NaN'),
            ('job_pair_frac', [(0, 1, 3), (0, 3, 1)], 1.5, 'job 0: frac of pair (2, 4) is outside 0..1'),
            ('job_pair_frac', [(0, 3, 3)], -0.25, 'job 0: frac of pair (4, 4) is outside 0..1'),
            ('job_pair_frac', [(0, 0, 0)], np.nan, 'job 0: frac of pair (1, 1) is outside 0..1'),
            ('job_pair_frames', [(0, 1, 3), (0, 3, 1)], -1, 'job 0: frames of pair (2, 4) is negative'),
            ('job_measure', [0], 2, 'job 0: measure 2 is neither 0 (IoU) nor 1 (IoMin)'),
            ('job_measure', [0], -1, 'job 0: measure -1 is neither'),
            ('job_result', [0], 1, 'job 0: result 1 outside 0..0')):
        p, outputs = prepared(xclass)
        for cell in cells:
            p[name][cell] = value
        refused(_lib, xclass, p, outputs, text)
    # the doubles are compared as bits: 0.0 and -0.0 are equal and differ
    p, outputs = prepared(xclass)
    p['job_pair_overlap'][0, 0, 2], p['job_pair_overlap'][0, 2, 0] = 0.0, -0.0
    refused(_lib, xclass, p, outputs, 'job 0: pair (1, 3) and pair (3, 1) differ')


def test_layout_is_checked_by_the_entry_point():
    _lib, xclass = _modules()
    p, outputs = prepared(xclass)
    p['local'][3] = 1
    refused(_lib, xclass, p, outputs, 'result 0: trajectory 1 occurs twice in frame 4')
    p, outputs = prepared(xclass)
    p['local'][1:] = [1, 0, 1]
    refused(_lib, xclass, p, outputs, 'result 0, row 1: trajectory index 1 before 0 appeared (indices number the trajectories by first appearance)')
    for bad in (0, 5):
        p, outputs = prepared(xclass)
        p['category'][2] = bad
        refused(_lib, xclass, p, outputs, 'category %d outside 1..4' % bad)
    for bad in (np.nan, np.inf, -np.inf):
        p, outputs = prepared(xclass)
        p['score'][2] = bad
        refused(_lib, xclass, p, outputs, 'result 0, row 2: score is not finite')
    p, outputs = prepared(xclass)
    p['stream_frame_offsets'][2] = 5
    refused(_lib, xclass, p, outputs, 'wt_xclass_tracks_host: CSR offsets do not cover the rows')
    p, outputs = prepared(xclass)
    outputs[3] = None
    refused(_lib, xclass, p, outputs, 'wt_xclass_tracks_host: bad argument')


def test_python_layer_refuses_before_it_calls():
    _lib, xclass = _modules()
    packed, out = packed_for([0, 3, 6]), arrays(dedup_cases.result(ROWS))
    pair = lambda **kw: [{'pairs': {(2, 4): kw}}]
    with pytest.raises(ValueError, match='overlap must not be NaN'):
        xclass.xclass_tracks(packed, [out], pair(overlap=float('nan')))
    with pytest.raises(ValueError, match='frames must be >= 0'):
        xclass.xclass_tracks(packed, [out], pair(frames=-1))
    for frac in (1.5, -0.1, float('nan')):
        with pytest.raises(ValueError, match=r'frac must be in 0\.\.1'):
            xclass.xclass_tracks(packed, [out], pair(frac=frac))
    with pytest.raises(ValueError, match="measure must be 'iou' or 'iomin'"):
        xclass.xclass_tracks(packed, [out], [{'pairs': {(2, 4): {}}, 'measure': 'giou'}])
    with pytest.raises(ValueError, match=r'pair \(2, 5\): classes are 1\.\.4'):
        xclass.xclass_tracks(packed, [out], [{'pairs': {(2, 5): {}}}])
    with pytest.raises(ValueError, match=r'pair \(4, 2\) is given twice'):
        xclass.xclass_tracks(packed, [out], [{'pairs': {(2, 4): {}, (4, 2): {'frames': 5}}}])
    with pytest.raises(ValueError, match='one value, or one per class'):
        xclass.xclass_tracks(packed, [out], [{'pairs': {(2, 4): {}}, 'prio': [1, 1]}])
    with pytest.raises(ValueError, match='names a result outside'):
        xclass.xclass_tracks(packed, [out], [{'pairs': {(2, 4): {}}, 'result': 1}])
    twice = arrays(dedup_cases.result(ROWS + [(4, 2, [1, 1, 5, 5], 0.5, 3)]))
    with pytest.raises(_lib.WaymoTrackError, match=r'wt_xclass_tracks failed: WT_ERR_INVALID \(result 0: object_id 3 occurs twice in image seg1/15/FRONT\)'):
        xclass.xclass_tracks(packed, [twice], [JOB])
    # a setting with no pair on is the input itself, and nothing is called
    assert xclass.xclass_one(packed, out, {}) is out and xclass.xclass_one(packed, out, {(2, 4): {'frames': 0}}, prio=[0, 0, 0, 1]) is out


def test_track_flags_default_to_off():
    from waymo_2d_tracking_amd.tracking import track
    parse = track.build_parser().parse_args
    args = parse([])
    assert args.xclass_pairs is None and args.xclass_frames == [3] and args.xclass_overlap == [0.7] and args.xclass_frac == [0.5]
    assert args.xclass_measure == 'iomin' and args.xclass_prio == [0]
    assert not track.xclasses(args) and track.xclass_pairs(args) == {}
    assert track.post_passes(args, None, 'the rows') == 'the rows'                          # nothing is imported or called
    args = parse(['--xclass-pairs', '2:4,1:4', '--xclass-frames', '3,0', '--xclass-overlap=0.9', '--xclass-prio=0,0,0,1', '--xclass-measure=iou'])
    assert args.xclass_pairs == [(2, 4), (1, 4)] and track.xclasses(args)
    assert track.xclass_pairs(args) == {(2, 4): {'frames': 3, 'overlap': 0.9, 'frac': 0.5}}                  # frames 0: the pair is off
    assert not track.xclasses(parse(['--xclass-pairs', '2:4', '--xclass-frames', '0']))
    with pytest.raises(SystemExit, match='one value, or one per listed pair'):
        track.xclass_pairs(parse(['--xclass-pairs', '2:4,1:4', '--xclass-frac', '0.5,0.5,0.5']))
    with pytest.raises(SystemExit, match='pairs of classes'):
        track.xclass_pairs(parse(['--xclass-pairs', '2:4:1']))


def test_workspace_depends_on_the_five_sizes_only():
    _lib, xclass = _modules()
    import ctypes as C
    ws = lambda name, J, nt, mt, S=40, nr=300000: int(getattr(_lib.lib(), name)(C.c_int32(J), C.c_int32(S), C.c_int64(nr), C.c_int64(nt), C.c_int64(mt)))
    small = ws('wt_xclass_tracks_workspace', 64, 40000, 1000)
    assert 0 < small <= 4 * 64 * 40 + 24 * 40001 + 12 * 300001 + 8192                       # up to the LDS limit: the summary, shared by all jobs
    big = ws('wt_xclass_tracks_workspace', 64, 40000, 2000)
    assert small < big <= small + 64 * 40000 * 12 + 4096                                    # beyond it: 12 bytes per (job, trajectory)
    assert ws('wt_xclass_tracks_workspace', -1, 1, 1) == 0
    assert (small, big) == (ws('wt_dedup_tracks_workspace', 64, 40000, 1000), ws('wt_dedup_tracks_workspace', 64, 40000, 2000))   # one carve for both passes
    limit = C.c_int32(0)
    _lib.lib().wt_xclass_tracks_limits(C.byref(limit))
    assert limit.value == 1024
