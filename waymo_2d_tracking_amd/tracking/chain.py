"""The tracking sweep with the rows resident in HBM: tracker -> layout -> refinement -> metric order -> CLEAR-MOT counts.

    chain = DeviceChain(packed, gt, n_classes=4, iou_threshold=(0.7, 0.5, 0.5, 0.5))
    results = chain.run([(max_age, min_hits, score, iou), ...], [{'max_gap': 1, 'min_len': 2}, ...])

DESIGN.md section 29 has the two definitions.  Between any two stages the other route of tracking/evaluate.py copies every row to
the host and lays it out again in numpy (_trackset.prepare, evaluate._align, evaluate.pack_results); here the two layout steps are
the HIP kernels behind ``wt_tracks_layout_dev`` and ``wt_tracks_to_eval_dev`` (include/waymotrack.h), and what crosses to the
host is a handful of scalars and the final count tables.  ``evaluate.sweep(..., device_chain=True)`` is the caller; the results
equal the other route's.  No arithmetic runs on the host; without a GPU the calls fail.
"""
import ctypes as C

import numpy as np

from .. import _lib
from . import _trackset as TS
from . import evaluate as E

_EVAL_COLUMNS = ('x', 'y', 'w', 'h', 'category', 'h_id', 'set_row_offsets', 'frame_hyp_offsets', 'order', 'max_frame_boxes')


def slot_map(packed, gt):
    """Per frame slot of `packed` the ground truth's frame slot, or -1 where the ground truth has no such frame or stream: the
    frames evaluate._align finds for the rows of a slot.  Host code over the keys, once per sweep; no ground-truth slot is named
    twice because a (stream, frame id) names one slot on either side."""
    sfo = np.asarray(packed['stream_frame_offsets'], dtype=np.int64)
    n_frames = int(sfo[-1])
    frame_id = np.asarray(packed['frame_ids'], dtype=np.int64)[:n_frames]
    stream = np.searchsorted(sfo, np.arange(n_frames), side='right') - 1
    to_gt = np.asarray([gt['stream_index'].get(k, -1) for k in packed['stream_keys']] + [-1], dtype=np.int64)
    s = to_gt[stream]
    fv, fkeys = gt['frame_values'], gt['frame_keys']
    r = np.searchsorted(fv, frame_id)
    known = (s >= 0) & (r < fv.size)
    if fv.size:
        known &= fv[np.minimum(r, fv.size - 1)] == frame_id
    key = np.where(known, s * max(1, fv.size) + r, -1)
    pos = np.searchsorted(fkeys, key)
    known &= (pos < fkeys.size) & (fkeys[np.minimum(pos, fkeys.size - 1)] == key) if fkeys.size else False
    return np.ascontiguousarray(np.where(known, pos, -1), dtype=np.int64)


def _eval_outputs(make, K, n_rows, n_gt_frames):
    n = max(1, n_rows)
    o = dict((k, make(n, np.float64)) for k in ('x', 'y', 'w', 'h'))
    o.update(category=make(n, np.int32), h_id=make(n, np.int32), set_row_offsets=make(K + 1, np.int64),
             frame_hyp_offsets=make((K, n_gt_frames + 1), np.int64), order=make(n, np.int64), max_frame_boxes=make(1, np.int64))
    return o


def to_eval_host(layout, boxes, smap, n_gt_frames, n_classes, box_stride=1):
    """wt_tracks_to_eval_host.  layout: set_row_offsets, frame_row_offsets (K, n_frames + 1), category and local as numpy arrays;
    boxes: the four columns x, y, w, h (box_stride 1) or one (n, 4) array (box_stride 4).  Returns the outputs by the names of
    evaluate.pack_results, 'orders' a list per result, plus 'max_frame_boxes'."""
    sro = np.ascontiguousarray(layout['set_row_offsets'], dtype=np.int64)
    fro = np.ascontiguousarray(layout['frame_row_offsets'], dtype=np.int64)
    K, n_frames, n = int(sro.size - 1), int(fro.shape[1] - 1), int(sro[-1])
    if box_stride == 4:
        bbox = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 4)
        cols = [bbox.reshape(-1)[i:] if bbox.size else bbox.reshape(-1) for i in range(4)]
        ptrs = [C.c_void_p(bbox.ctypes.data + 8 * i) for i in range(4)]
    else:
        cols = [np.ascontiguousarray(b, dtype=np.float64) for b in boxes]
        ptrs = [_lib.ptr(c) for c in cols]
    cat, local = np.ascontiguousarray(layout['category'], dtype=np.int32), np.ascontiguousarray(layout['local'], dtype=np.int32)
    smap = np.ascontiguousarray(smap, dtype=np.int64)
    o = _eval_outputs(np.zeros, K, n, n_gt_frames)
    ptr = _lib.ptr
    rc = _lib.lib().wt_tracks_to_eval_host(C.c_int64(n_frames), C.c_int32(K), ptr(sro), ptr(fro), *ptrs, C.c_int64(box_stride), ptr(cat), ptr(local), ptr(smap),
                                           C.c_int64(n_gt_frames), C.c_int32(n_classes), *[ptr(o[k]) for k in _EVAL_COLUMNS])
    _lib.check(rc, 'wt_tracks_to_eval_host')
    out = dict((k, o[k][:n]) for k in ('x', 'y', 'w', 'h', 'category', 'h_id'))
    out.update(set_row_offsets=o['set_row_offsets'], frame_hyp_offsets=o['frame_hyp_offsets'], max_frame_boxes=int(o['max_frame_boxes'][0]),
               orders=[o['order'][int(sro[k]):int(sro[k + 1])] for k in range(K)])
    return out


class DeviceToEval(object):
    """wt_tracks_to_eval_dev on K results that are in HBM in the shared layout: the device twin of evaluate._align + pack_results.
    `source` is a _trackset.DeviceTrackSet after wait(), or a refine.DeviceRefine after emit().  ``launch()`` enqueues the call on
    the current torch stream; ``wait()`` synchronises, raises what the kernel reported and reads ``max_frame_boxes``; ``out`` holds
    the output tensors by the names of evaluate.pack_results."""
    name = 'wt_tracks_to_eval_dev'

    def __init__(self, source, smap, n_gt_frames, n_classes, workspace_bytes=None):
        import torch
        self.torch = torch
        self.lib = _lib.lib()
        self.device = torch.device('cuda', torch.cuda.current_device())
        if isinstance(source, TS.DeviceTrackSet):
            t = source.t
            self.K, self.n_rows, self.n_frames, self.box_stride = source.R, source.n_rows, source.n_frames, 1
            self.inputs = [t['set_row_offsets'], t['frame_row_offsets'], t['x'], t['y'], t['w'], t['h'], t['category'], t['local']]
            self.box_ptrs = [t[k].data_ptr() for k in ('x', 'y', 'w', 'h')]
        else:                                            # DeviceRefine: one job = one result, the boxes are the rows of out['bbox']
            o = source.out
            self.K, self.n_rows, self.n_frames, self.box_stride = source.p['J'], int(o['frame'].numel()) - 1, source.p['n_frames'], 4
            self.inputs = [source.job_row_offsets, o['frame_row_offsets'], o['bbox'], o['category'], o['local']]
            self.box_ptrs = [o['bbox'].data_ptr() + 8 * i for i in range(4)]
        if self.K < 1:
            raise ValueError('at least one result is needed')
        self.n_gt_frames, self.n_classes = int(n_gt_frames), int(n_classes)
        self.smap = smap
        make = lambda shape, dtype: torch.zeros(shape, dtype=getattr(torch, np.dtype(dtype).name), device=self.device)
        self.out = _eval_outputs(make, self.K, self.n_rows, self.n_gt_frames)
        self.status = make(1, np.int32)
        self.lib.wt_tracks_to_eval_workspace.restype = C.c_size_t
        self.ws_bytes = int(self.lib.wt_tracks_to_eval_workspace(C.c_int32(self.K), C.c_int64(self.n_rows)))
        if not self.ws_bytes:
            _lib.check(4, 'wt_tracks_to_eval_workspace')
        self.ws = torch.empty(self.ws_bytes if workspace_bytes is None else int(workspace_bytes), dtype=torch.uint8, device=self.device)
        self.max_frame_boxes = None

    def nbytes(self):
        return sum(int(v.numel()) * v.element_size() for v in self.out.values()) + int(self.ws.numel())

    def launch(self):
        d = lambda v: C.c_void_p(v.data_ptr())
        sro, fro = self.inputs[0], self.inputs[1]
        cat, local = self.inputs[-2], self.inputs[-1]
        rc = self.lib.wt_tracks_to_eval_dev(
            C.c_int64(self.n_frames), C.c_int32(self.K), C.c_int64(self.n_rows), d(sro), d(fro), *[C.c_void_p(p) for p in self.box_ptrs],
            C.c_int64(self.box_stride), d(cat), d(local), d(self.smap), C.c_int64(self.n_gt_frames), C.c_int32(self.n_classes),
            *[d(self.out[k]) for k in _EVAL_COLUMNS], d(self.status), d(self.ws), C.c_size_t(int(self.ws.numel())),
            C.c_void_p(self.torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, self.name)
        self.max_frame_boxes = None

    def wait(self):
        if self.max_frame_boxes is None:
            self.torch.cuda.current_stream().synchronize()
            st = int(self.status.item())
            if st:
                raise _lib.WaymoTrackError('%s failed: %s (status reported by the kernel)' % (self.name, _lib._STATUS.get(st, st)))
            self.max_frame_boxes = int(self.out['max_frame_boxes'].item())
        return self


class DeviceChain(object):
    """Tracker settings scored with the rows resident in HBM.  The detections of `packed` and the ground truth are uploaded once; ``run(points, jobs)``
    takes the tracked points - (max_age, min_hits, score, iou), or with the second association (..., low_score, low_iou), as
    evaluate._tracked_points gives them - and the refinement jobs (dicts with 'max_gap' and 'min_len'; None or empty: no
    refinement, the layout goes straight to the metric order) and returns one evaluate.MotResult per (point, job), points outermost:
    the order of evaluate.sweep_settings().  Per round it runs the trackers, ONE wt_tracks_layout_dev over all their results, ONE
    refine plan + emit over results x jobs, ONE wt_tracks_to_eval_dev and ONE wt_mot_eval_dev.  What crosses to the host per round:
    the layout's three scalars and its status, the planned row count the refine emit reads, max_frame_boxes and the status of the
    metric order, and the count tables with the offsets their ignored_rows are read from.

    Rounds.  The points are split so that the buffers of one round stay below `workspace_limit_bytes`.  A point is counted at its
    capacity, n = detections + 1 rows: the tracker's outputs (60 n) and workspace, the layout's columns, trajectory ids and
    workspace (76 n), and per job the refinement's workspace (its sizer at n rows and n trajectories) and outputs (64 n) and the
    metric order's outputs and workspace (52 n).  Rows that a gap fill adds are not foreseen, and a round holds at least one point.
    ``peak_bytes`` is the largest sum of the tensors a round really held, ``copied_bytes`` what went up and came down."""

    def __init__(self, packed, gt, n_classes=4, iou_threshold=E.DEFAULT_IOU_THRESHOLD, workspace_limit_bytes=E.DEFAULT_WORKSPACE_LIMIT):
        import torch
        from .. import devpath
        self.torch, self.devpath = torch, devpath
        self.packed, self.gt, self.n_classes, self.iou_threshold = packed, gt, int(n_classes), tuple(iou_threshold)
        self.limit = int(workspace_limit_bytes)
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.base = devpath.DeviceTracker(packed, [0.0] * self.n_classes, 1, 0, [0.0] * self.n_classes)     # the upload; never run
        smap = slot_map(packed, gt)
        self.smap = torch.from_numpy(smap).to(self.device) if smap.size else torch.zeros(1, dtype=torch.int64, device=self.device)
        self.n_gt_frames = int(gt['frame_ids'].size)
        self.g = None
        self.peak_bytes, self.rounds = 0, 0
        self.tracked_rows, self.scored_rows = [], []      # per round: the rows of the tracked points, the rows that were scored
        self.copied_bytes = sum(int(getattr(self.base, k).numel()) * getattr(self.base, k).element_size() for k in self.base._INPUTS) + smap.nbytes
        self.events = []                                 # per round, when record_events is set: {stage: (start, end)} torch events
        self.record_events = False

    def _tracker(self, point):
        max_age, min_hits, score, iou = point[:4]
        C_ = self.n_classes
        if len(point) > 4:
            return self.devpath.DeviceTrackerByte(self.packed, [iou] * C_, max_age, min_hits, [score] * C_, [point[4]] * C_, [point[5]] * C_, share=self.base)
        return self.devpath.DeviceTracker(self.packed, [iou] * C_, max_age, min_hits, [score] * C_, share=self.base)

    def points_per_round(self, n_jobs):
        """how many tracked points one round holds (the class docstring has the count)"""
        n = self.base.n_dets + 1
        J = max(1, n_jobs)
        per_point = 60 * n + self.base.ws_bytes + 76 * n + J * (64 + 52) * n
        if n_jobs:
            per_point += int(_lib.lib().wt_refine_tracks_workspace(C.c_int32(J), C.c_int32(self.base.n_streams), C.c_int64(n), C.c_int64(n), C.c_int64(n)))
        return max(1, self.limit // max(1, per_point))

    def _timed(self, marks, stage, call):
        if not self.record_events:
            return call()
        start, end = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        start.record()
        value = call()
        end.record()
        marks.setdefault(stage, []).append((start, end))
        return value

    def _round(self, points, jobs):
        marks = {}
        trackers = [self._tracker(p) for p in points]
        self._timed(marks, 'track', lambda: [t.run() for t in trackers])
        ts = TS.DeviceTrackSet(self.packed, trackers, self.n_classes)
        self._timed(marks, 'layout', ts.launch)
        ts.wait()
        held = sum(sum(int(v.numel()) * v.element_size() for v in (t.out_frame, t.out_category, t.out_bbox, t.out_score, t.out_id, t.workspace)) for t in trackers)
        held += ts.nbytes()
        down = 3 * 8 + 4
        source = ts
        if jobs:
            from . import refine
            source = refine.DeviceRefine(self.packed, ts, [dict(job, result=k) for k in range(len(points)) for job in jobs], self.n_classes)
            self._timed(marks, 'refine', lambda: (source.launch(), source.emit()))
            held += int(source.ws.numel()) + sum(int(v.numel()) * v.element_size() for v in source.out.values())
            self.copied_bytes += sum(int(source.t[k].numel()) * source.t[k].element_size() for k in ('job_result', 'job_max_gap', 'job_min_len', 'job_score_mode'))
            down += 8 + 4
        order = DeviceToEval(source, self.smap, self.n_gt_frames, len(self.iou_threshold))
        self._timed(marks, 'to_eval', order.launch)
        order.wait()
        if jobs:
            source.wait('wt_refine_tracks_emit_dev')
        ev = E.DeviceEvaluation.from_device(self.gt, order.out, order.n_rows, order.max_frame_boxes, self.iou_threshold, g=self.g)
        if self.g is None:                               # the ground truth goes up with the first round
            self.g = ev.g
            self.copied_bytes += sum(int(v.numel()) * v.element_size() for v in ev.g.values())
        self._timed(marks, 'mot_eval', ev.launch)
        results = ev.results()
        held += order.nbytes() + int(ev.ws.numel()) + sum(int(v.numel()) * v.element_size() for v in (ev.counts, ev.iou_sum))
        down += 8 + 4 + 4 + (order.K + 1) * 8 + order.K * 8 + int(ev.counts.numel()) * 8 + int(ev.iou_sum.numel()) * 8
        self.copied_bytes += down + int(ts.tables.numel()) * 8
        self.peak_bytes = max(self.peak_bytes, held)
        self.rounds += 1
        self.tracked_rows.append(ts.n_rows)
        self.scored_rows.append(order.n_rows)
        if self.record_events:
            self.events.append(marks)
        return results

    def run(self, points, jobs=None):
        points, jobs = list(points), list(jobs or [])
        step = self.points_per_round(len(jobs))
        results = []
        for lo in range(0, len(points), step):
            results += self._round(points[lo:lo + step], jobs)
        return results
