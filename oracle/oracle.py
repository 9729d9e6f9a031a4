"""TEST INFRASTRUCTURE ONLY - ctypes front-end of the CPU oracle (oracle/_build/libwt_oracle.so).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module, and only as
the checker / reported baseline.  The product package never imports it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, '_build', 'libwt_oracle.so')


def build(force=False):
    srcs = [os.path.join(HERE, f) for f in os.listdir(HERE) if f.endswith(('.c', '.h')) or f == 'Makefile']
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        subprocess.check_call(['make', '-s', '-C', HERE])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        _lib = C.CDLL(LIB_PATH)
        _lib.wto_iou.restype = C.c_double
        _lib.wto_sort_create.restype = C.c_void_p
        _lib.wto_sort_create.argtypes = [C.c_int, C.c_int, C.c_void_p]
        _lib.wto_sort_destroy.argtypes = [C.c_void_p]
    return _lib


def _p(a, t=None):
    return a.ctypes.data_as(C.c_void_p)


def iou(det, trk):
    det = np.ascontiguousarray(det, dtype=np.float32)
    trk = np.ascontiguousarray(trk, dtype=np.float64)
    return float(lib().wto_iou(_p(det), _p(trk)))


def linear_assignment(cost):
    cost = np.ascontiguousarray(cost, dtype=np.float32)
    n, m = cost.shape
    pairs = np.zeros((min(n, m) + 1, 2), dtype=np.int32)
    k = C.c_int(0)
    rc = lib().wto_linear_assignment_f32(_p(cost), C.c_int(n), C.c_int(m), _p(pairs), C.byref(k))
    assert rc == 0, rc
    return pairs[:k.value].astype(np.int64)


def linear_assignment_stats(cost):
    """linear_assignment plus the oracle's work counters: (pairs, dict(step6=executions of step 6 that changed the matrix,
    paths=augmenting paths, longest_path=stars on the longest augmenting path))."""
    cost = np.ascontiguousarray(cost, dtype=np.float32)
    n, m = cost.shape
    pairs = np.zeros((min(n, m) + 1, 2), dtype=np.int32)
    k = C.c_int(0)
    stats = np.zeros(3, dtype=np.int64)
    rc = lib().wto_linear_assignment_stats_f32(_p(cost), C.c_int(n), C.c_int(m), _p(pairs), C.byref(k), _p(stats))
    assert rc == 0, rc
    return pairs[:k.value].astype(np.int64), dict(step6=int(stats[0]), paths=int(stats[1]), longest_path=int(stats[2]))


def iou_cost(dets5, trks4):
    """The float32 matrix associate() hands to the assignment: -iou, shape (n, t)."""
    dets5 = np.ascontiguousarray(dets5, dtype=np.float32).reshape(-1, 5)
    trks4 = np.ascontiguousarray(trks4, dtype=np.float64).reshape(-1, 4)
    neg = np.zeros((len(dets5), len(trks4)), dtype=np.float32)
    if neg.size:
        lib().wto_iou_cost(_p(dets5), C.c_int(len(dets5)), _p(trks4), C.c_int(len(trks4)), _p(neg))
    return neg


def associate(dets5, trks4, iou_threshold):
    dets5 = np.ascontiguousarray(dets5, dtype=np.float32).reshape(-1, 5)
    trks4 = np.ascontiguousarray(trks4, dtype=np.float64).reshape(-1, 4)
    n, t = len(dets5), len(trks4)
    matches = np.zeros((min(n, t) + 1, 2), np.int32)
    ud = np.zeros(2 * n + 1, np.int32)
    ut = np.zeros(2 * t + 1, np.int32)
    nm, nud, nut = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = lib().wto_associate(_p(dets5), C.c_int(n), _p(trks4), C.c_int(t), C.c_double(iou_threshold),
                             _p(matches), C.byref(nm), _p(ud), C.byref(nud), _p(ut), C.byref(nut))
    assert rc == 0, rc
    return matches[:nm.value].copy(), ud[:nud.value].copy(), ut[:nut.value].copy()


class Sort(object):
    """oracle twin of tracking/sort/sort.py:233 Sort (ids through a shared int64 counter array)."""

    def __init__(self, max_age=1, min_hits=3, counter=None):
        self.counter = counter if counter is not None else np.zeros(1, dtype=np.int64)
        self._h = lib().wto_sort_create(C.c_int(max_age), C.c_int(min_hits), _p(self.counter))

    def update(self, dets, iou_threshold):
        dets = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 5)
        cap = len(dets) + 4096
        out = np.zeros((cap, 6), dtype=np.float64)
        k = C.c_int(0)
        rc = lib().wto_sort_update(C.c_void_p(self._h), _p(dets), C.c_int(len(dets)), C.c_double(iou_threshold),
                                   _p(out), C.c_int(cap), C.byref(k))
        assert rc == 0, rc
        return out[:k.value].copy()

    def state(self, cap=8192):
        ids = np.zeros(cap, np.int64); x = np.zeros((cap, 7)); P = np.zeros((cap, 49)); n = C.c_int(0)
        rc = lib().wto_sort_state(C.c_void_p(self._h), C.c_int(cap), _p(ids), _p(x), _p(P), C.byref(n))
        assert rc == 0, rc
        return ids[:n.value].copy(), x[:n.value].copy(), P[:n.value].copy()

    def predicted(self, cap=8192):
        """Predicted boxes (t, 4) the next update() associates against; the tracker is not changed."""
        boxes = np.zeros((cap, 4)); n = C.c_int(0)
        rc = lib().wto_sort_predicted(C.c_void_p(self._h), C.c_int(cap), _p(boxes), C.byref(n))
        assert rc == 0, rc
        return boxes[:n.value].copy()

    def __del__(self):
        if getattr(self, '_h', None):
            lib().wto_sort_destroy(C.c_void_p(self._h))
            self._h = None


def track_streams(packed, max_age, min_hits, score_threshold, iou_threshold, id_base=0):
    """packed: dict from waymo_2d_tracking_amd.tracking.pack.pack_streams().  Returns dict of output arrays."""
    n = int(packed['x'].size)
    st = np.ascontiguousarray(score_threshold, dtype=np.float64)
    it = np.ascontiguousarray(iou_threshold, dtype=np.float64)
    out_frame = np.zeros(n + 1, np.int64); out_cat = np.zeros(n + 1, np.int32)
    out_bbox = np.zeros((n + 1, 4), np.float64); out_score = np.zeros(n + 1, np.float64)
    out_id = np.zeros(n + 1, np.int64)
    n_out = C.c_int64(0); n_births = C.c_int64(0)
    rc = lib().wto_track_streams(
        C.c_int64(n), _p(packed['x']), _p(packed['y']), _p(packed['w']), _p(packed['h']), _p(packed['score']),
        _p(packed['category']), C.c_int64(packed['frame_det_offsets'].size - 1), _p(packed['frame_det_offsets']),
        C.c_int32(packed['stream_frame_offsets'].size - 1), _p(packed['stream_frame_offsets']),
        _p(packed['clip_w']), _p(packed['clip_h']), C.c_int(max_age), C.c_int(min_hits), C.c_int(len(st)),
        _p(st), _p(it), C.c_int64(id_base), _p(out_frame), _p(out_cat), _p(out_bbox), _p(out_score), _p(out_id),
        C.byref(n_out), C.byref(n_births))
    assert rc == 0, rc
    k = n_out.value
    return dict(frame=out_frame[:k], category=out_cat[:k], bbox=out_bbox[:k], score=out_score[:k],
                object_id=out_id[:k], n_births=n_births.value)


def softnms(boxes, scores, overlap=0.5, cut=1.0, conf_thresh=0.0, top_k=0):
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 4)
    scores = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    n = len(scores)
    keep = np.zeros(n + 1, np.int64); out = np.zeros(n + 1, np.float64); k = C.c_int(0)
    rc = lib().wto_softnms(_p(boxes), _p(scores), C.c_int(n), C.c_double(overlap), C.c_double(cut),
                           C.c_double(conf_thresh), C.c_int(top_k), _p(keep), _p(out), C.byref(k))
    assert rc == 0, rc
    return keep[:k.value].copy(), out[:k.value].copy()


def hardnms(boxes, scores, overlap=0.5, top_k=0):
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 4)
    scores = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    n = len(scores)
    keep = np.zeros(n + 1, np.int64); out = np.zeros(n + 1, np.float64); k = C.c_int(0)
    rc = lib().wto_hardnms(_p(boxes), _p(scores), C.c_int(n), C.c_double(overlap), C.c_int(top_k), _p(keep), _p(out),
                           C.byref(k))
    assert rc == 0, rc
    return keep[:k.value].copy(), out[:k.value].copy()


def nms_detections(detections, iou_thresh=0.5, soft=False, soft_nms_cut=1.0):
    d = np.ascontiguousarray(np.vstack([np.asarray(x, dtype=np.float64).reshape(-1, 5) for x in detections]))
    n = len(d)
    out = np.zeros((n + 1, 5)); k = C.c_int(0)
    rc = lib().wto_nms_detections(_p(d), C.c_int(n), C.c_double(iou_thresh), C.c_int(1 if soft else 0),
                                  C.c_double(soft_nms_cut), _p(out), C.byref(k))
    assert rc == 0, rc
    return out[:k.value].copy()


def merge_detections(detections, nms_thresh=0.5):
    dl = [np.asarray(x, dtype=np.float64).reshape(-1, 5) for x in detections]
    d = np.ascontiguousarray(np.vstack(dl))
    sizes = np.array([len(x) for x in dl], dtype=np.int32)
    n = len(d)
    out = np.zeros((n + 1, 5)); k = C.c_int(0)
    rc = lib().wto_merge_detections(_p(d), _p(sizes), C.c_int(len(dl)), C.c_double(nms_thresh), _p(out), C.c_int(n + 1),
                                    C.byref(k))
    assert rc == 0, rc
    return out[:k.value].copy()


def ensemble_groups(dets5, group_offsets, input_sizes, k_inputs, method, iou_thresh, cut):
    d = np.ascontiguousarray(dets5, dtype=np.float64).reshape(-1, 5)
    go = np.ascontiguousarray(group_offsets, dtype=np.int64)
    isz = np.ascontiguousarray(input_sizes, dtype=np.int32)
    G = go.size - 1
    out = np.zeros((len(d) + 1, 5)); counts = np.zeros(G + 1, np.int64)
    rc = lib().wto_ensemble_groups(_p(d), _p(go), _p(isz), C.c_int64(G), C.c_int(k_inputs), C.c_int(method),
                                   C.c_double(iou_thresh), C.c_double(cut), _p(out), _p(counts))
    assert rc == 0, rc
    return out[:len(d)], counts[:G]
