"""What wt_xlink_tracks_host refuses before it touches a device (no GPU): the status code and the wt_last_error() text of the
layout and job checks of csrc/xlink_host.h, reached through tracking/xlink.py's own argument marshalling; and what
tracking/xlink.py and the flags of tracking/track.py refuse or leave alone before anything is called."""
import numpy as np
import pytest

import xlink_cases
from track_cases import result
from track_stage_support import arrays, packed_for

INVALID = 1

ROWS = [(0, 2, [0, 0, 5, 5], 0.5, 1), (3, 2, [0, 0, 5, 5], 0.5, 2), (4, 4, [0, 0, 5, 5], 0.5, 3), (4, 2, [9, 9, 5, 5], 0.5, 2)]
JOB = xlink_cases.job({(2, 4): xlink_cases.pair(3, 0.9), (1, 1): xlink_cases.pair(2, 0.6)}, prio=[0, 0, 0, 1], motion='linear')


def _modules():
    from waymo_2d_tracking_amd import build
    build.build(verbose=False)
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import xlink
    return _lib, xlink


def prepared(xlink):
    """two streams of three slots; stream 1 holds trajectory 0 at slots 3 and 4 and trajectory 1 at slot 4: local = [0, 0, 1, 0]"""
    p = xlink._prepare(packed_for([0, 3, 6]), [arrays(result(ROWS))], [JOB], 4)
    assert p['local'].tolist() == [0, 0, 1, 0] and p['n_traj'].tolist() == [[1, 2]] and p['n_traj_total'] == 3
    outputs = [np.zeros(*xlink._outputs(p)[k]) for k in xlink._OUT]
    return p, outputs


def refused(_lib, xlink, p, outputs, text):
    assert xlink._host_call(p, outputs) == INVALID
    message = _lib.lib().wt_last_error().decode()
    assert text in message, message


def test_python_layer_builds_symmetric_tables():
    _lib, xlink = _modules()
    p, outputs = prepared(xlink)
    gap, thr = p['job_pair_max_link'][0], p['job_pair_link_iou'][0]
    assert gap.dtype == np.int32 and thr.dtype == np.float64 and gap.shape == (4, 4)
    assert gap.tolist() == [[2, 0, 0, 0], [0, 0, 0, 3], [0, 0, 0, 0], [0, 3, 0, 0]]
    assert (gap == gap.T).all() and thr.tobytes() == thr.T.copy().tobytes() and thr[1, 3] == 0.9 and thr[0, 0] == 0.6 and thr[2, 2] == 0.3
    assert p['job_class_prio'].tolist() == [[0, 0, 0, 1]] and p['job_motion'].tolist() == [1] and p['traj_ids'][0].tolist() == [1, 2, 3]
    assert [o.shape for o in outputs] == [(1, 3)] * 4 + [(1, 4)] * 2 + [(1, 2)] * 2 and outputs[2].dtype == np.float64 and outputs[7].dtype == np.int64
    q = xlink._prepare(packed_for([0, 3, 6]), [arrays(result(ROWS))], [{'pairs': {(4, 2): {}}}], 4)
    assert q['job_pair_max_link'][0, 1, 3] == q['job_pair_max_link'][0, 3, 1] == 1 and q['job_motion'].tolist() == [0] and q['job_class_prio'].tolist() == [[0] * 4]
    assert xlink.pair_tables({}, 4)[0].tolist() == [[0] * 4] * 4


def test_job_parameters_are_checked_by_the_entry_point():
    _lib, xlink = _modules()
    for name, cells, value, text in (
            ('job_pair_max_link', [(0, 1, 3)], 4, 'job 0: pair (2, 4) and pair (4, 2) differ (the tables must be symmetric)'),
            ('job_pair_link_iou', [(0, 3, 1)], np.nextafter(0.9, 1.0), 'job 0: pair (2, 4) and pair (4, 2) differ'),
            ('job_pair_link_iou', [(0, 0, 2)], 0.25, 'job 0: pair (1, 3) and pair (3, 1) differ'),
            ('job_pair_link_iou', [(0, 1, 3), (0, 3, 1)], np.nan, 'job 0: link_iou of pair (2, 4) is NaN'),
            ('job_pair_link_iou', [(0, 2, 2)], np.nan, 'job 0: link_iou of pair (3, 3) is NaN'),
            ('job_pair_max_link', [(0, 1, 3), (0, 3, 1)], -1, 'job 0: max_link of pair (2, 4) is negative'),
            ('job_motion', [0], 2, 'job 0: motion must be 0 (hold) or 1 (linear)'),
            ('job_motion', [0], -1, 'job 0: motion must be'),
            ('job_result', [0], 1, 'job 0: result 1 outside 0..0')):
        p, outputs = prepared(xlink)
        for cell in cells:
            p[name][cell] = value
        refused(_lib, xlink, p, outputs, text)
    # the doubles are compared as bits: 0.0 and -0.0 are equal and differ
    p, outputs = prepared(xlink)
    p['job_pair_link_iou'][0, 0, 2], p['job_pair_link_iou'][0, 2, 0] = 0.0, -0.0
    refused(_lib, xlink, p, outputs, 'job 0: pair (1, 3) and pair (3, 1) differ')


def test_layout_is_checked_by_the_entry_point():
    _lib, xlink = _modules()
    p, outputs = prepared(xlink)
    p['local'][3] = 1
    refused(_lib, xlink, p, outputs, 'result 0: trajectory 1 occurs twice in frame 4')
    p, outputs = prepared(xlink)
    p['local'][1:] = [1, 0, 1]
    refused(_lib, xlink, p, outputs, 'result 0, row 1: trajectory index 1 before 0 appeared (indices number the trajectories by first appearance)')
    for bad in (0, 5):
        p, outputs = prepared(xlink)
        p['category'][2] = bad
        refused(_lib, xlink, p, outputs, 'category %d outside 1..4' % bad)
    p, outputs = prepared(xlink)
    p['stream_frame_offsets'][2] = 5
    refused(_lib, xlink, p, outputs, 'wt_xlink_tracks_host: CSR offsets do not cover the rows')
    for k in (3, 5, 7):
        p, outputs = prepared(xlink)
        outputs[k] = None
        refused(_lib, xlink, p, outputs, 'wt_xlink_tracks_host: bad argument')
    p, outputs = prepared(xlink)
    p['n_classes'] = 17
    refused(_lib, xlink, p, outputs, 'wt_xlink_tracks_host: 17 classes, at most 16')          # before any table is read as 17 x 17


def test_python_layer_refuses_before_it_calls():
    _lib, xlink = _modules()
    packed, out = packed_for([0, 3, 6]), arrays(result(ROWS))
    pair = lambda **kw: [{'pairs': {(2, 4): kw}}]
    with pytest.raises(ValueError, match='link_iou must not be NaN'):
        xlink.xlink_tracks(packed, [out], pair(link_iou=float('nan')))
    with pytest.raises(ValueError, match='max_link must be >= 0'):
        xlink.xlink_tracks(packed, [out], pair(max_link=-1))
    with pytest.raises(ValueError, match="motion must be 'hold' or 'linear'"):
        xlink.xlink_tracks(packed, [out], [{'pairs': {(2, 4): {}}, 'motion': 'kalman'}])
    with pytest.raises(ValueError, match=r'pair \(2, 5\): classes are 1\.\.4'):
        xlink.xlink_tracks(packed, [out], [{'pairs': {(2, 5): {}}}])
    with pytest.raises(ValueError, match=r'pair \(4, 2\) is given twice'):
        xlink.xlink_tracks(packed, [out], [{'pairs': {(2, 4): {}, (4, 2): {'max_link': 5}}}])
    with pytest.raises(ValueError, match='one value, or one per class'):
        xlink.xlink_tracks(packed, [out], [{'pairs': {(2, 4): {}}, 'prio': [1, 1]}])
    with pytest.raises(ValueError, match='names a result outside'):
        xlink.xlink_tracks(packed, [out], [{'pairs': {(2, 4): {}}, 'result': 1}])
    with pytest.raises(ValueError, match='at most 16 classes'):
        xlink.xlink_tracks(packed, [out], [JOB], n_classes=17)
    twice = arrays(result(ROWS + [(4, 2, [1, 1, 5, 5], 0.5, 3)]))
    with pytest.raises(_lib.WaymoTrackError, match=r'wt_xlink_tracks failed: WT_ERR_INVALID \(result 0: object_id 3 occurs twice in image seg1/15/FRONT\)'):
        xlink.xlink_tracks(packed, [twice], [JOB])
    # a setting with no pair on is the input itself, and nothing is called
    assert xlink.xlink_one(packed, out, {}) is out and xlink.xlink_one(packed, out, {(2, 4): {'max_link': 0}}, prio=[0, 0, 0, 1]) is out


def test_track_flags_default_to_off():
    from waymo_2d_tracking_amd.tracking import track
    parse = track.build_parser().parse_args
    args = parse([])
    assert args.xlink_pairs is None and args.xlink_gap == [1] and args.xlink_iou == [0.3] and args.xlink_motion == 'hold' and args.xlink_prio == [0]
    assert not track.xlinks(args) and track.xlink_pairs(args) == {}
    assert track.post_passes(args, None, 'the rows') == 'the rows'                          # nothing is imported or called
    args = parse(['--xlink-pairs', '2:4,1:2', '--xlink-gap', '2,0', '--xlink-iou=0.5', '--xlink-prio=0,0,0,1', '--xlink-motion=linear'])
    assert args.xlink_pairs == [(2, 4), (1, 2)] and track.xlinks(args) and args.xlink_motion == 'linear' and args.xlink_prio == [0, 0, 0, 1]
    assert track.xlink_pairs(args) == {(2, 4): {'max_link': 2, 'link_iou': 0.5}}                     # gap 0: the pair is off
    assert track.xlink_pairs(parse(['--xlink-pairs', '2:4,2:2', '--xlink-gap', '2,1', '--xlink-iou', '0.5,0.25'])) == {
        (2, 4): {'max_link': 2, 'link_iou': 0.5}, (2, 2): {'max_link': 1, 'link_iou': 0.25}}
    assert not track.xlinks(parse(['--xlink-pairs', '2:4', '--xlink-gap', '0']))
    with pytest.raises(SystemExit, match='one value, or one per listed pair'):
        track.xlink_pairs(parse(['--xlink-pairs', '2:4,1:4', '--xlink-iou', '0.5,0.5,0.5']))
    with pytest.raises(SystemExit, match='pairs of classes'):
        track.xlink_pairs(parse(['--xlink-pairs', '2:4:1']))
    # the pass sits between stitching and the suppression of duplicates
    names = [asked.__name__ for asked, _ in track.CHAIN]
    assert names == ['splits', 'stitches', 'xlinks', 'dedups', 'xclasses', 'refines', 'smooths']
    assert [asked for asked, _ in track.CHAIN if asked is not track.xlinks] == [asked for asked, _ in track.PASSES]


def test_workspace_depends_on_the_five_sizes_only():
    _lib, xlink = _modules()
    import ctypes as C
    ws = lambda J, nt, mt, S=40, nr=300000: int(_lib.lib().wt_xlink_tracks_workspace(C.c_int32(J), C.c_int32(S), C.c_int64(nr), C.c_int64(nt), C.c_int64(mt)))
    small = ws(64, 40000, 1000)
    assert 0 < small <= 4 * 64 * 40 + 32 * 40001 + 8192                                     # up to the LDS limit: rounds and the summary, shared by all jobs
    big = ws(64, 40000, 2000)
    assert small < big <= small + 64 * 40000 * 36 + 4096                                    # beyond it: 36 bytes per (job, trajectory)
    assert ws(-1, 1, 1) == 0 and ws(64, 40000, 1000, nr=5) == small
    limit = C.c_int32(0)
    _lib.lib().wt_xlink_tracks_limits(C.byref(limit))
    assert limit.value == 1024
