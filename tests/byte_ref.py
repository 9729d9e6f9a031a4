"""CPU reference of the tracker's second association with low-score detections: builds tests/native/byte_sort_ref.c (which
includes oracle/sort_oracle.c, so Kalman filter, IoU and assignment are the oracle's own) with gcc and the oracle Makefile's flags
into a temporary directory, once per process."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ['-O2', '-std=c11', '-fPIC', '-ffp-contract=off', '-fno-fast-math']
STATS = ('second_run', 'second_match', 'second_reject', 'second_transposed', 'first_skipped', 'second_no_track', 'nonfinite',
         'nonfinite_second', 'low_created')
_state = {}


def lib():
    if 'lib' not in _state:
        tmp = tempfile.TemporaryDirectory(prefix='byte_ref_')
        so = os.path.join(tmp.name, 'libbyte_sort_ref.so')
        subprocess.run(['gcc'] + FLAGS + ['-shared', '-o', so, os.path.join(ROOT, 'tests', 'native', 'byte_sort_ref.c'), '-lm'], check=True)
        _state['tmp'] = tmp
        _state['lib'] = C.CDLL(so)
    return _state['lib']


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def low_pair_iou(track_xywh, det_xywh):
    """The float32 IoU the association stores for a detection and the predicted box, one frame later, of a track that a
    detection `track_xywh` founded in the frame before (the oracle's own track_init, predict and iou)."""
    L = lib()
    L.wto_sort_create.restype = C.c_void_p
    L.wto_iou.restype = C.c_double
    row = lambda b: np.asarray([[b[0], b[1], b[0] + b[2], b[1] + b[3], 1.0]], np.float32)
    s = C.c_void_p(L.wto_sort_create(C.c_int(1), C.c_int(0), None))
    out6, k = np.zeros(12), C.c_int(0)
    assert L.wto_sort_update(s, _p(row(track_xywh)), C.c_int(1), C.c_double(0.3), _p(out6), C.c_int(2), C.byref(k)) == 0
    box, nb = np.zeros(4), C.c_int(0)
    assert L.wto_sort_predicted(s, C.c_int(1), _p(box), C.byref(nb)) == 0 and nb.value == 1
    v = np.float32(L.wto_iou(_p(row(det_xywh)), _p(box)))
    L.wto_sort_destroy(s)
    return v


def track_streams(packed, max_age, min_hits, score_threshold, iou_threshold, low_score, low_iou, id_base=0):
    """The reference's answer for a packed set of streams (tracking/utils.pack_streams): dict of output arrays, 'n_births' and
    'stats' (named counters over all trackers: what the second association did)."""
    n = int(packed['x'].size)
    st, it = np.ascontiguousarray(score_threshold, dtype=np.float64), np.ascontiguousarray(iou_threshold, dtype=np.float64)
    ls, li = np.ascontiguousarray(low_score, dtype=np.float64), np.ascontiguousarray(low_iou, dtype=np.float64)
    assert len(st) == len(it) == len(ls) == len(li)
    out_frame = np.zeros(n + 1, np.int64); out_cat = np.zeros(n + 1, np.int32)
    out_bbox = np.zeros((n + 1, 4), np.float64); out_score = np.zeros(n + 1, np.float64)
    out_id = np.zeros(n + 1, np.int64)
    stats = np.zeros(len(STATS), np.int64)
    n_out = C.c_int64(0); n_births = C.c_int64(0)
    rc = lib().wtb_track_streams(
        C.c_int64(n), _p(packed['x']), _p(packed['y']), _p(packed['w']), _p(packed['h']), _p(packed['score']),
        _p(packed['category']), C.c_int64(packed['frame_det_offsets'].size - 1), _p(packed['frame_det_offsets']),
        C.c_int32(packed['stream_frame_offsets'].size - 1), _p(packed['stream_frame_offsets']),
        _p(packed['clip_w']), _p(packed['clip_h']), C.c_int(max_age), C.c_int(min_hits), C.c_int(len(st)),
        _p(st), _p(it), _p(ls), _p(li), C.c_int64(id_base), _p(out_frame), _p(out_cat), _p(out_bbox), _p(out_score), _p(out_id),
        C.byref(n_out), C.byref(n_births), _p(stats))
    assert rc == 0, rc
    k = n_out.value
    return dict(frame=out_frame[:k], category=out_cat[:k], bbox=out_bbox[:k], score=out_score[:k], object_id=out_id[:k],
                n_births=n_births.value, stats=dict(zip(STATS, stats.tolist())))
