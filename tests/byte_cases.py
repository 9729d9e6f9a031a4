"""Inputs for the tracker's second association with low-score detections, each built to reach one path of
sort_streams_kernel<false, true> / tracker_step_byte.  tests/test_byte_cases.py proves on the CPU, from the reference's counters
(tests/byte_ref.py 'stats'), that every case reaches the path it is named for; tests/test_gpu_track_byte.py runs them on the GPU.

A case is a dict: packed (tracking/utils.pack_streams layout), max_age, min_hits, score / iou (the high thresholds), low_score /
low_iou, `reach` (counter -> least value the reference must report) and, for the hand-worked ones, `rows`: the expected
(frame, category, object_id) of every output row and `births`."""
import os

import numpy as np

from waymo_2d_tracking_amd.tracking import utils as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
HIGH, LOW = 0.6, 0.1          # scores: 0.9 is high, 0.3 is low, 0.05 is invalid
C4 = 4


def packed_from(streams, camera='FRONT'):
    """streams: list of streams; a stream is a list of frames; a frame is a list of (x, y, w, h, score, category)."""
    pred = {}
    for s, frames in enumerate(streams):
        cam = pred.setdefault('seg%04d' % s, {}).setdefault(camera, {})
        for f, dets in enumerate(frames):
            cam[f] = [{'bbox': [d[0], d[1], d[2], d[3]], 'score': d[4], 'category_id': d[5]} for d in dets]
    return T.pack_streams(pred)


def case(packed, max_age=1, min_hits=0, score=HIGH, iou=0.3, low_score=LOW, low_iou=0.5, reach=None, rows=None, births=None, n=C4):
    one = lambda v: [float(v)] * n if np.isscalar(v) else [float(u) for u in v]
    return dict(packed=packed, max_age=max_age, min_hits=min_hits, score=one(score), iou=one(iou), low_score=one(low_score),
                low_iou=one(low_iou), reach=reach or {}, rows=rows, births=births)


BOX = (100, 100, 50, 80)


def dip():
    """One still object whose score dips below high for two frames, max_age = 1.  Plain SORT at the high threshold loses it in
    frame 3 (time_since_update 2 > max_age) and starts id 2 in frame 4; with the second association the low detections of frames
    2 and 3 continue id 1, and those frames emit a row.  Frames 2 and 3 have no high detection: the first association is skipped."""
    scores = [0.9, 0.9, 0.3, 0.3, 0.9, 0.9]
    frames = [[BOX + (s, 1)] for s in scores]
    return case(packed_from([frames]), reach={'second_run': 2, 'second_match': 2, 'first_skipped': 2},
                rows=[(f, 1, 1) for f in range(6)], births=1)


def lone_low():
    """A low detection with no track creates nothing: frames 0 and 1 hold one low detection each (the tracker exists and ticks,
    no row, no id); the high detection of frame 2 starts id 1."""
    frames = [[BOX + (0.3, 1)], [BOX + (0.3, 1)], [BOX + (0.9, 1)]]
    return case(packed_from([frames]), reach={'low_created': 1}, rows=[(2, 1, 1)], births=1)


def high_keeps_track():
    """A low detection never takes a track that a high one matched: in frame 1 the low detection sits exactly on the track and
    the high one is shifted (IoU 0.6); the high one gets the track, no track is left and the low one is dropped - one row."""
    frames = [[BOX + (0.9, 1)], [(110, 100, 50, 80, 0.9, 1), BOX + (0.3, 1)], [(110, 100, 50, 80, 0.9, 1)]]
    return case(packed_from([frames]), reach={'second_no_track': 1}, rows=[(0, 1, 1), (1, 1, 1), (2, 1, 1)], births=1)


def edge(low_iou):
    """A still 60 x 60 track and, in frame 1, one low detection shifted by 7 pixels; frame 2 brings the high detection back.
    The test sets low_iou from the pair's float32 IoU (byte_ref.low_pair_iou): just above it the pair is rejected - no row in frame 1,
    no birth, and the track (max_age 1) is still id 1 in frame 2."""
    frames = [[(100, 100, 60, 60, 0.9, 1)], [(107, 100, 60, 60, 0.3, 1)], [(100, 100, 60, 60, 0.9, 1)]]
    return case(packed_from([frames]), low_iou=low_iou)


EDGE_TRACK, EDGE_DET = (100, 100, 60, 60), (107, 100, 60, 60)


def contested_two_tracks():
    """Two tracks left over (60 x 60 at x = 100 and x = 140) and one low detection at x = 120 with the same IoU to both: the
    assignment's tie-break decides (1 x 2 cost matrix, not transposed)."""
    a, b, d = (100, 100, 60, 60), (140, 100, 60, 60), (120, 100, 60, 60)
    frames = [[a + (0.9, 1), b + (0.9, 1)], [d + (0.3, 1)], [a + (0.9, 1), b + (0.9, 1)]]
    return case(packed_from([frames]), iou=0.2, low_iou=0.2, reach={'second_run': 1, 'second_match': 1})


def contested_two_dets():
    """One track left over (x = 120) and two low detections (x = 100 and x = 140) with the same IoU to it: fewer tracks than
    detections, so the second association runs transposed."""
    a, b, d = (100, 100, 60, 60), (140, 100, 60, 60), (120, 100, 60, 60)
    frames = [[d + (0.9, 1)], [a + (0.3, 1), b + (0.3, 1)], [d + (0.9, 1)]]
    return case(packed_from([frames]), iou=0.2, low_iou=0.2, reach={'second_run': 1, 'second_match': 1, 'second_transposed': 1})


def grid_boxes(n, jitter=None):
    """n disjoint 40 x 40 boxes on a 60-pixel grid, 30 to a row; jitter: integer offsets (n, 2) added to x, y."""
    k = np.arange(n)
    xy = np.stack([20 + 60 * (k % 30), 20 + 60 * (k // 30)], 1)
    if jitter is not None:
        xy = xy + jitter
    return [(int(x), int(y), 40, 40) for x, y in xy]


def wave_edges(n_low, n_left, seed=0):
    """n_left tracks (frame 0, all high) meet n_low low detections and no high one in frame 1: the second cost matrix is
    n_low x n_left, detections over lanes and tracks broadcast 64 at a time.  The low detections sit on the first grid places,
    shifted by up to 9 pixels (IoU from about 0.4 up), so some pairs fall under low_iou = 0.5.  Frame 2 repeats frame 0."""
    rng = np.random.default_rng(seed + 1000 * n_low + n_left)
    first = [b + (0.9, 1) for b in grid_boxes(n_left)]
    second = [b + (0.3, 1) for b in grid_boxes(n_low, rng.integers(-9, 10, (n_low, 2)))]
    reach = {'second_run': 1, 'second_match': 1, 'second_reject': 1, 'first_skipped': 1}
    if n_left < n_low:
        reach['second_transposed'] = 1
    return case(packed_from([[first, second, first]]), reach=reach)


def off_lds():
    """More than 256 trackers (65 streams x 4 classes: the small LDS budget) and one stream whose frame 0 has 100 high
    detections and whose frame 1 has 100 low ones: the second cost matrix is 100 x 100 with leading dimension 101, more floats
    than the LDS cost buffer holds, so it lives in global memory.  The other 64 streams hold one detection each."""
    rng = np.random.default_rng(7)
    first = [b + (0.9, 1) for b in grid_boxes(100)]
    second = [b + (0.3, 1) for b in grid_boxes(100, rng.integers(-9, 10, (100, 2)))]
    streams = [[first, second, first]] + [[[(50, 50, 40, 40, 0.9, 1 + s % 4)]] for s in range(64)]
    return case(packed_from(streams), reach={'second_run': 1, 'second_match': 1})


def low_creates_class():
    """Class 2's first valid detection is low (frame 0) and precedes class 1's first (frame 1, where class 1 even comes first in
    input order): class 2 is first in the id order, so its track of frame 1 is id 1 and its row comes first."""
    frames = [[(300, 300, 50, 50, 0.3, 2)], [BOX + (0.9, 1), (300, 300, 50, 50, 0.9, 2)]]
    return case(packed_from([frames]), reach={'low_created': 1}, rows=[(1, 2, 1), (1, 1, 2)], births=2)


def nonfinite():
    """The boxes of tests/golden/sort_g9_nonfinite.npz (a 3e19-wide detection whose float32 area overflows: its track's
    predicted box is not finite and the track is dropped at the next predict), one class, with the score of every frame's first
    detection made low in the frames after the first: the frames that drop a track also continue one through the second association."""
    z = np.load(os.path.join(GOLDEN, 'sort_g9_nonfinite.npz'))
    frames = []
    for i in range(len(z['in_off']) - 1):
        d = z['dets'][z['in_off'][i]:z['in_off'][i + 1]].astype(np.float64)
        frames.append([(r[0], r[1], r[2] - r[0], r[3] - r[1], 0.3 if (k == 0 and i > 0) else 0.9, 1) for k, r in enumerate(d)])
    return case(packed_from([frames]), max_age=2, iou=0.1, low_iou=0.1, reach={'nonfinite': 2, 'nonfinite_second': 1, 'second_match': 3})


def random_streams(seed, n_segments, n_frames, n_objects, max_age, min_hits, streams=None):
    """Waymo-shaped synthetic streams with uniform scores: with low 0.3 and high 0.6 about 30 % lie between."""
    from waymo_2d_tracking_amd import synthetic as syn
    dets = syn.make_sequence_json(seed, n_segments=n_segments, n_frames=n_frames, n_objects=n_objects)
    pred = {}
    for e in dets:
        seg, fr, cam = e['image_id'].split('/')
        pred.setdefault(seg, {}).setdefault(cam, {}).setdefault(int(fr), []).append(
            {'bbox': e['bbox'], 'score': e['score'], 'category_id': e['category_id']})
    packed = T.pack_streams(pred)
    if streams is not None:
        packed = T.slice_streams(packed, 0, streams)
    return case(packed, max_age=max_age, min_hits=min_hits, score=[0.6, 0.6, 1.0, 0.6], iou=[0.2, 0.1, 1.0, 0.05],
                low_score=[0.3, 0.3, 1.0, 0.3], low_iou=[0.4, 0.3, 1.0, 0.2],
                reach={'second_run': 10, 'second_match': 10, 'second_reject': 1, 'second_transposed': 1})


HAND = {'dip': dip, 'lone_low': lone_low, 'high_keeps_track': high_keeps_track}
WAVE_EDGES = [(nl, nr) for nl in (63, 64, 65) for nr in (63, 64, 65)] + [(130, 70)]
AGE_HITS = [(1, 0), (3, 1), (2, 3)]
PATHS = dict(HAND, contested_two_tracks=contested_two_tracks, contested_two_dets=contested_two_dets, off_lds=off_lds,
             low_creates_class=low_creates_class, nonfinite=nonfinite)
