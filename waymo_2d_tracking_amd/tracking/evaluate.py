"""MOTA / MOTP of tracking results against ground truth, and the threshold sweep that tunes the tracker's flags.

    python -m waymo_2d_tracking_amd.tracking.evaluate --annotations GT.json TRACKS.json [TRACKS2.json ...]
        [--iou-threshold 0.7,0.5,0.5,0.5] [--json OUT] [--identity] [--hota] [--coverage]
    python -m waymo_2d_tracking_amd.tracking.evaluate --annotations GT.json --sweep DETECTIONS.json
        --score-grid 0.5:1.0:0.05 --iou-grid 0.0,0.01,0.1,0.3 --max-age 1,2,3 --min-hits 0,1 [--low-score-grid 0.2,0.4 --low-iou-grid 0.3,0.5] [--link-gap-grid 0,2,4 --link-iou-grid 0.3,0.5] [--dedup-frames-grid 0,3,5 --dedup-iou-grid 0.5,0.7] [--gap-grid 0,1,2 --min-len-grid 1,2,3] [--identity] [--hota] [--coverage] [--rank-by idf1|hota|mt] [--device-chain]

The metric is CLEAR-MOT (Bernardin & Stiefelhagen 2008) per class and Waymo difficulty level; DESIGN.md ("Tracking metric")
has the exact definition.  Every (result, segment, camera, class) is an independent problem and one wavefront of the HIP
kernel behind ``wt_mot_eval_host`` (include/waymotrack.h): K results are scored in one launch, which is what makes a
sweep over tracker settings cost seconds.  --identity adds identity preservation (IDF1 / IDP / IDR, Ristani et al. 2016; DESIGN.md
section 18) through ``wt_mot_identity_host``: per problem one trajectory-by-trajectory overlap matrix and one global assignment.
--hota adds HOTA / DetA / AssA / LocA (Luiten et al. 2021) through ``wt_mot_hota_host``: one wavefront per
problem and difficulty level, one assignment per frame scored at 19 localisation thresholds.  --coverage adds what became of every
ground-truth trajectory (mostly tracked / partially tracked / mostly lost, fragmentations) through
``wt_mot_coverage_host``, which reads the matches of the CLEAR-MOT kernel where they lie in device memory.  --device-chain runs a sweep
of the tracker, refinement and MOTA with the rows resident in HBM from the detections to the count tables (tracking/chain.py).  No arithmetic of the metric runs on the host; without a GPU the calls fail.
"""
import argparse
import collections
import ctypes as C
import importlib
import itertools
import json
import math

import numpy as np

from .. import _lib
from . import utils as T

DEFAULT_IOU_THRESHOLD = (0.7, 0.5, 0.5, 0.5)       # Waymo: 0.7 vehicles, 0.5 pedestrians and cyclists
ALL_CLASSES = (1, 2, 4)                            # the three evaluated types (3 = sign is not tracked)
FIELDS = ('gt', 'tp', 'fn', 'fp', 'idsw')
LEVELS = (1, 2)


def _floats(s):
    return [float(item) for item in s.split(',')]


def _split(image_id):
    segment_id, frame_id, camera_id = image_id.split('/')
    return segment_id, int(frame_id), camera_id


def _columns(rows, stream_index, with_level):
    n = len(rows)
    stream = np.zeros(n, np.int64)
    frame = np.zeros(n, np.int64)
    box = np.zeros((n, 4), np.float64)
    cat = np.zeros(n, np.int32)
    level = np.ones(n, np.int32)
    oid = np.empty(n, dtype=object)
    for i, e in enumerate(rows):
        segment_id, frame_id, camera_id = _split(e['image_id'])
        key = (segment_id, camera_id)
        s = stream_index.get(key)
        if s is None:
            s = stream_index[key] = len(stream_index)
        stream[i] = s
        frame[i] = frame_id
        box[i] = e['bbox']
        cat[i] = e['category_id']
        oid[i] = str(e['object_id'])
        if with_level and e.get('tracking_difficulty_level', 1) == 2:
            level[i] = 2
    return stream, frame, box, cat, level, oid


def _dense_ids(stream, oid, per_stream):
    """Object ids -> int32, equal ids inside a stream <-> equal numbers; per_stream: numbered from 0 in every stream."""
    if oid.size == 0:
        return np.zeros(0, np.int32), 0
    _, inv = np.unique(oid.astype(str), return_inverse=True)
    n_names = int(inv.max()) + 1
    pair, ids = np.unique(stream * n_names + inv, return_inverse=True)
    if not per_stream:
        return ids.astype(np.int32), int(pair.size)
    first = np.searchsorted(pair // n_names, np.arange(int(stream.max()) + 1))
    ids = ids - first[stream]
    return ids.astype(np.int32), int(ids.max()) + 1


def load_ground_truth(path_or_json):
    """Ground-truth COCO file (dict with 'annotations' and optionally 'images', or a bare list) -> packed columns.

    Streams are numbered by first appearance; a stream's frames are those of 'images' when the file has that list,
    otherwise those that carry at least one annotation.  Rows with w < 1 or h < 1 are dropped (tracking/utils.py:79)."""
    data = path_or_json
    if isinstance(path_or_json, str):
        with open(path_or_json) as fp:
            data = json.load(fp)
    annotations = data['annotations'] if isinstance(data, dict) else data
    images = data.get('images') if isinstance(data, dict) else None
    stream_index = {}
    if images is not None:
        im_stream = np.zeros(len(images), np.int64)
        im_frame = np.zeros(len(images), np.int64)
        for i, im in enumerate(images):
            segment_id, frame_id, camera_id = _split(im['id'])
            im_stream[i] = stream_index.setdefault((segment_id, camera_id), len(stream_index))
            im_frame[i] = frame_id
    stream, frame, box, cat, level, oid = _columns(annotations, stream_index, True)
    if images is None:
        im_stream, im_frame = stream, frame
    n_streams = len(stream_index)
    # frames: unique (stream, frame id), streams in first-appearance order, frame ids ascending
    frame_values = np.unique(np.concatenate([im_frame, frame]))
    nv = max(1, frame_values.size)
    fkeys = np.unique(im_stream * nv + np.searchsorted(frame_values, im_frame))
    frame_stream = fkeys // nv
    frame_ids = frame_values[fkeys % nv] if fkeys.size else np.zeros(0, np.int64)
    stream_frame_offsets = np.searchsorted(frame_stream, np.arange(n_streams + 1)).astype(np.int64)
    row_key = stream * nv + np.searchsorted(frame_values, frame)
    pos = np.searchsorted(fkeys, row_key)
    on_frame = np.zeros(row_key.size, bool)         # with 'images', an annotation on a frame outside that list takes no part
    if fkeys.size:
        on_frame = (pos < fkeys.size) & (fkeys[np.minimum(pos, fkeys.size - 1)] == row_key)
    keep = on_frame & ~((box[:, 2] < 1) | (box[:, 3] < 1))
    src = np.nonzero(keep)[0]
    order = src[np.argsort(pos[src], kind='stable')]
    gframe = pos[order]
    gt_id, max_ids = _dense_ids(stream[order], oid[order], per_stream=True)
    frame_gt_offsets = np.searchsorted(gframe, np.arange(fkeys.size + 1)).astype(np.int64)
    keys = [None] * n_streams
    for key, s in stream_index.items():
        keys[s] = key
    return dict(
        x=np.ascontiguousarray(box[order, 0]), y=np.ascontiguousarray(box[order, 1]),
        w=np.ascontiguousarray(box[order, 2]), h=np.ascontiguousarray(box[order, 3]),
        category=np.ascontiguousarray(cat[order]), level=np.ascontiguousarray(level[order]), gt_id=gt_id, max_gt_ids=max_ids,
        object_id=oid[order],
        source_row=order.astype(np.int64), frame_gt_offsets=frame_gt_offsets, stream_frame_offsets=stream_frame_offsets,
        frame_ids=frame_ids.astype(np.int64), frame_values=frame_values, frame_keys=fkeys, stream_keys=keys,
        stream_index=dict((k, i) for i, k in enumerate(keys)))


def load_tracks(path_or_rows):
    """Tracking JSON as tracking/track.py writes it -> columns in file order (streams numbered on their own)."""
    rows = path_or_rows
    if isinstance(path_or_rows, str):
        with open(path_or_rows) as fp:
            rows = json.load(fp)
    stream_index = {}
    stream, frame, box, cat, _, oid = _columns(rows, stream_index, False)
    keys = [None] * len(stream_index)
    for key, s in stream_index.items():
        keys[s] = key
    return dict(stream=stream, frame_id=frame, x=box[:, 0].copy(), y=box[:, 1].copy(), w=box[:, 2].copy(), h=box[:, 3].copy(),
                category=cat, object_id=oid, stream_keys=keys)


def tracks_from_packed(packed, out):
    """Output of utils.track_packed -> the columns load_tracks() gives for the file track.py would write from it."""
    f = np.asarray(out['frame'], dtype=np.int64)
    stream = np.searchsorted(packed['stream_frame_offsets'], f, side='right') - 1
    bbox = np.asarray(out['bbox'], dtype=np.float64).reshape(-1, 4)
    return dict(stream=stream.astype(np.int64), frame_id=np.asarray(packed['frame_ids'], dtype=np.int64)[f],
                x=bbox[:, 0].copy(), y=bbox[:, 1].copy(), w=bbox[:, 2].copy(), h=bbox[:, 3].copy(),
                category=np.asarray(out['category'], dtype=np.int32), object_id=np.asarray(out['object_id']),
                stream_keys=list(packed['stream_keys']))


def _align(gt, tr, n_classes):
    """Rows of one result in the kernel's order: those on the ground truth's frames sorted by frame (file order inside),
    then the ignored ones.  Returns (order, frame_hyp_offsets, h_id)."""
    n = int(tr['stream'].size)
    n_frames = int(gt['frame_ids'].size)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(n_frames + 1, np.int64), np.zeros(0, np.int32)
    to_gt = np.asarray([gt['stream_index'].get(k, -1) for k in tr['stream_keys']] + [-1], dtype=np.int64)
    s = to_gt[tr['stream']]
    fv, fkeys = gt['frame_values'], gt['frame_keys']
    nv = max(1, fv.size)
    r = np.searchsorted(fv, tr['frame_id'])
    known = (s >= 0) & (r < fv.size)
    if fv.size:
        known &= fv[np.minimum(r, fv.size - 1)] == tr['frame_id']
    key = np.where(known, s * nv + r, -1)
    pos = np.searchsorted(fkeys, key)
    if fkeys.size:
        known &= (pos < fkeys.size) & (fkeys[np.minimum(pos, fkeys.size - 1)] == key)
    else:
        known &= False
    known &= (tr['category'] >= 1) & (tr['category'] <= n_classes)
    pos = np.where(known, pos, n_frames)
    order = np.argsort(pos, kind='stable')
    offsets = np.searchsorted(pos[order], np.arange(n_frames + 1)).astype(np.int64)
    oid = tr['object_id']
    if oid.dtype == object or oid.dtype.kind in 'US':
        h_id, _ = _dense_ids(tr['stream'], oid, per_stream=False)
    else:                                            # integer ids straight from the tracker: unique over the whole result
        _, h_id = np.unique(oid, return_inverse=True)
        h_id = h_id.astype(np.int32)
    return order.astype(np.int64), offsets, np.ascontiguousarray(h_id[order])


def _check_unique(gt, tr, order, offsets, h_id, set_index):
    """An object id twice in one frame of one class: no metric is defined (WT_ERR_INVALID, with the image id)."""
    n_on = int(offsets[-1])
    if n_on == 0:
        return
    frame = np.searchsorted(offsets, np.arange(n_on), side='right') - 1
    cat = tr['category'][order[:n_on]].astype(np.int64)
    key = (frame * 64 + cat) * (int(h_id.max()) + 1) + h_id[:n_on]
    u, first, count = np.unique(key, return_index=True, return_counts=True)
    if (count > 1).any():
        i = int(first[np.argmax(count > 1)])
        f = int(frame[i])
        s = int(np.searchsorted(gt['stream_frame_offsets'], f, side='right') - 1)
        segment_id, camera_id = gt['stream_keys'][s]
        raise _lib.WaymoTrackError('wt_mot_eval failed: WT_ERR_INVALID (result %d: object_id %s occurs twice in image %s/%d/%s)'
                                   % (set_index, tr['object_id'][order[i]], segment_id, int(gt['frame_ids'][f]), camera_id))


class _Scores(object):
    """What the four result classes share: `table` {class id or 'ALL': {1: row, 2: row}} ('ALL' = classes 1, 2, 4), every row made
    by the subclass's row(classes, level index) from its per-stream counts, and the JSON form."""

    def fill_table(self, n_classes):
        self.table = {}
        for c in list(range(1, n_classes + 1)) + ['ALL']:
            classes = [c] if c != 'ALL' else [x for x in ALL_CLASSES if x <= n_classes]
            self.table[c] = dict((lv, self.row(classes, li)) for li, lv in enumerate(LEVELS))

    def as_json(self):
        return {'ignored_rows': int(self.ignored_rows),
                'table': dict((str(c), dict(('LEVEL_%d' % lv, r) for lv, r in rows.items())) for c, rows in self.table.items())}


def _added(counts, classes, li):
    """Counts (n_streams, n_classes, 2, fields) of `classes` at level index li, added over the streams."""
    return counts[:, [c - 1 for c in classes], li, :].reshape(-1, counts.shape[-1]).sum(axis=0)


class MotResult(_Scores):
    """Scores of one tracking result.

    counts    (n_streams, n_classes, 2, 5) int64: gt, tp, fn, fp, idsw for LEVEL_1, LEVEL_2, per stream
    iou_sum   (n_streams, n_classes, 2) float64
    table     row = gt, tp, fn, fp, idsw, iou_sum, MOTA, MOTP
    ignored_rows   result rows that took no part (frames or streams the ground truth does not have)
    hyp_match / hyp_switch (with per_row=True), one entry per result row in file order: index of the matched annotation in the
        ground-truth file's list (-1 false positive, -2 ignored) and 1 where that match is an identity switch."""

    def __init__(self, counts, iou_sum, ignored_rows, stream_keys, hyp_match=None, hyp_switch=None):
        self.counts, self.iou_sum, self.ignored_rows, self.stream_keys = counts, iou_sum, ignored_rows, stream_keys
        self.hyp_match, self.hyp_switch = hyp_match, hyp_switch
        self.fill_table(counts.shape[1])

    def row(self, classes, li):
        row = dict(zip(FIELDS, (int(v) for v in _added(self.counts, classes, li))))
        # the order of this sum is part of the definition: class by class, stream by stream (cumsum adds one by one)
        parts = np.concatenate([self.iou_sum[:, c - 1, li] for c in classes]) if classes else np.zeros(0)
        total = float(np.cumsum(parts)[-1]) if parts.size else 0.0
        row['iou_sum'] = total
        row['MOTA'] = 1.0 - (row['fn'] + row['fp'] + row['idsw']) / row['gt'] if row['gt'] else math.nan
        row['MOTP'] = total / row['tp'] if row['tp'] else math.nan
        return row

    def mota(self, level=2, category='ALL'):
        return self.table[category][level]['MOTA']


def pack_results(gt, tracks_list, n_classes):
    """K results -> the concatenated columns and offsets wt_mot_eval_* takes (include/waymotrack.h)."""
    if len(tracks_list) < 1:
        raise ValueError('at least one result is needed')
    orders, offsets, cols = [], [], dict((k, []) for k in ('x', 'y', 'w', 'h', 'category', 'h_id'))
    set_rows = [0]
    for k, tr in enumerate(tracks_list):
        order, off, h_id = _align(gt, tr, n_classes)
        _check_unique(gt, tr, order, off, h_id, k)
        orders.append(order)
        offsets.append(off)
        for name in ('x', 'y', 'w', 'h'):
            cols[name].append(np.asarray(tr[name], dtype=np.float64)[order])
        cols['category'].append(np.asarray(tr['category'], dtype=np.int32)[order])
        cols['h_id'].append(h_id)
        set_rows.append(set_rows[-1] + int(order.size))
    out = dict((n, np.ascontiguousarray(np.concatenate(cols[n]), dtype=np.float64)) for n in ('x', 'y', 'w', 'h'))
    out['category'] = np.ascontiguousarray(np.concatenate(cols['category']), dtype=np.int32)
    out['h_id'] = np.ascontiguousarray(np.concatenate(cols['h_id']), dtype=np.int32)
    out['set_row_offsets'] = np.asarray(set_rows, dtype=np.int64)
    out['frame_hyp_offsets'] = np.ascontiguousarray(np.stack(offsets), dtype=np.int64)
    out['orders'] = orders
    return out


def max_frame_boxes(gt, packed, n_classes):
    """Most boxes of one class in one frame, on either side (sizes the kernel's per-wavefront scratch)."""
    n_frames = int(gt['frame_ids'].size)
    best = 0

    def side(cat, frame_offsets):
        n = int(frame_offsets[-1])
        if n == 0:
            return 0
        frame = np.searchsorted(frame_offsets, np.arange(n), side='right') - 1
        ok = (cat[:n] >= 1) & (cat[:n] <= n_classes)
        return int(np.bincount(frame[ok] * n_classes + cat[:n][ok] - 1, minlength=1).max()) if ok.any() else 0
    best = side(gt['category'], gt['frame_gt_offsets']) if n_frames else 0
    for k in range(packed['frame_hyp_offsets'].shape[0]):
        lo = int(packed['set_row_offsets'][k])
        best = max(best, side(packed['category'][lo:], packed['frame_hyp_offsets'][k]))
    return best


def _result_sets(packed):
    """(k, first row, end row, rows that took no part) of every result in pack_results() output."""
    set_rows = packed['set_row_offsets']
    for k in range(len(set_rows) - 1):
        lo, hi = int(set_rows[k]), int(set_rows[k + 1])
        yield k, lo, hi, (hi - lo) - int(packed['frame_hyp_offsets'][k][-1])


def _file_order(gt, packed, k, m):
    """Matches of result k's rows in the kernel's order -> the file's row order, ground-truth rows as annotation indices."""
    match = np.empty(m.shape, np.int64)
    match[packed['orders'][k]] = np.where(m >= 0, gt['source_row'][np.maximum(m, 0)], m) if gt['source_row'].size else m
    return match


def _results(gt, packed, counts, iou_sum, hyp_match, hyp_switch, per_row):
    results = []
    for k, lo, hi, _ in _result_sets(packed):
        m = hyp_match[lo:hi]
        match = switch = None
        if per_row:
            match = _file_order(gt, packed, k, m)
            switch = np.empty(hi - lo, np.uint8)
            switch[packed['orders'][k]] = hyp_switch[lo:hi]
        results.append(MotResult(counts[k], iou_sum[k], int((m == -2).sum()), gt['stream_keys'], match, switch))
    return results


_BOX = ('x', 'y', 'w', 'h')


def _gt_args(gt, g, ids, ptr):
    """The ground-truth arguments every wt_mot_* call begins with.  g: the columns by name (gt itself, or its tensors), ids: the
    id / trajectory column; ptr makes a pointer (_lib.ptr of numpy arrays for the host forms, the data pointer of tensors for the
    device forms)."""
    return ([C.c_int64(gt['x'].size)] + [ptr(g[n]) for n in _BOX + ('category', 'level')] +
            [ptr(ids), C.c_int64(gt['frame_ids'].size), ptr(g['frame_gt_offsets']), C.c_int32(len(gt['stream_keys'])), ptr(g['stream_frame_offsets'])])


def _hyp_args(K, n_hyp, h, ids, ptr):
    """The result arguments that follow them.  n_hyp: None for the host forms, which read it from set_row_offsets."""
    return ([C.c_int32(K)] + ([] if n_hyp is None else [C.c_int64(n_hyp)]) + [ptr(h['set_row_offsets']), ptr(h['frame_hyp_offsets'])] +
            [ptr(h[n]) for n in _BOX + ('category',)] + [ptr(ids)])


def evaluate_tracks(gt, tracks_list, iou_threshold=DEFAULT_IOU_THRESHOLD, per_row=False, packed=None):
    """Score K tracking results (load_tracks / tracks_from_packed) against one ground truth (load_ground_truth) in ONE
    wt_mot_eval_host call.  packed: pack_results() of the same arguments, when the caller has it.  Returns a list of K MotResult."""
    lib = _lib.lib()
    thr = _lib.as_f64(iou_threshold)
    n_classes = int(thr.size)
    p = packed if packed is not None else pack_results(gt, tracks_list, n_classes)
    K = len(tracks_list)
    n_streams = len(gt['stream_keys'])
    counts = np.zeros((K, n_streams, n_classes, 2, 5), np.int64)
    iou_sum = np.zeros((K, n_streams, n_classes, 2), np.float64)
    n_hyp = int(p['set_row_offsets'][-1])
    hyp_match = np.full(n_hyp, -2, np.int64)
    hyp_switch = np.zeros(n_hyp, np.uint8)
    rc = lib.wt_mot_eval_host(
        *_gt_args(gt, gt, gt['gt_id'], _lib.ptr), *_hyp_args(K, None, p, p['h_id'], _lib.ptr),
        C.c_int32(n_classes), _lib.ptr(thr), _lib.ptr(counts), _lib.ptr(iou_sum),
        _lib.ptr(hyp_match), _lib.ptr(hyp_switch) if per_row else None)
    _lib.check(rc, 'wt_mot_eval_host')
    return _results(gt, p, counts, iou_sum, hyp_match, hyp_switch, per_row)


class _DeviceForm(object):
    """What DeviceEvaluation and DeviceIdentity share: the packed results, the ground-truth and result columns as torch tensors
    in HBM (self.g, self.h; the subclass adds its id columns), the status word, and the wait for a launch."""
    name = None                                     # the C entry point, for messages

    def __init__(self, gt, tracks_list, iou_threshold):
        import torch
        self.torch = torch
        self.lib = _lib.lib()
        self.gt = gt
        self.thr = _lib.as_f64(iou_threshold)
        self.n_classes = int(self.thr.size)
        self.p = pack_results(gt, tracks_list, self.n_classes)
        self.K = len(tracks_list)
        self.n_streams = len(gt['stream_keys'])
        self.n_hyp = int(self.p['set_row_offsets'][-1])
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.g = dict((n, self.up(gt[n])) for n in _BOX + ('category', 'level', 'frame_gt_offsets', 'stream_frame_offsets'))
        self.h = dict((n, self.up(self.p[n])) for n in _BOX + ('category', 'set_row_offsets', 'frame_hyp_offsets'))
        self.status = self.zeros(1, torch.int32)

    def up(self, a):
        """numpy array -> tensor on the device (one element where the array is empty: a pointer the library may be handed)."""
        t = self.torch.from_numpy(np.ascontiguousarray(a))
        return t.to(self.device) if a.size else self.zeros(1, t.dtype)

    def zeros(self, shape, dtype):
        return self.torch.zeros(shape, dtype=dtype, device=self.device)

    def d(self, t):
        """Device pointer of a tensor; an empty one (no streams) has none, and the library wants one it then never follows."""
        return C.c_void_p(t.data_ptr() if t.numel() else self.status.data_ptr())

    def leading_args(self, g_ids, h_ids):
        return _gt_args(self.gt, self.g, g_ids, self.d) + _hyp_args(self.K, self.n_hyp, self.h, h_ids, self.d)

    def wait(self):
        """Synchronise the current stream and raise what the kernel reported."""
        self.torch.cuda.current_stream().synchronize()
        st = int(self.status.item())
        if st:
            raise _lib.WaymoTrackError('%s failed: %s (status reported by the kernel)' % (self.name, _lib._STATUS.get(st, st)))


class DeviceEvaluation(_DeviceForm):
    """The same evaluation with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues one
    wt_mot_eval_dev on the current torch stream and returns at once, ``results()`` synchronises and reads the outputs back.
    This is the form a device-resident sweep (tracker output scored without leaving the GPU) builds on - tracking/chain.py, through
    ``from_device()``; the layout checks of the host form are done here when the inputs are packed."""
    name = 'wt_mot_eval_dev'

    def __init__(self, gt, tracks_list, iou_threshold=DEFAULT_IOU_THRESHOLD):
        _DeviceForm.__init__(self, gt, tracks_list, iou_threshold)
        torch = self.torch
        self.max_boxes = max_frame_boxes(gt, self.p, self.n_classes)
        self.g['gt_id'], self.h['h_id'] = self.up(gt['gt_id']), self.up(self.p['h_id'])
        self.hyp_match = self.zeros(max(1, self.n_hyp), torch.int64)
        self.hyp_switch = self.zeros(max(1, self.n_hyp), torch.uint8)
        self._outputs()

    @classmethod
    def from_device(cls, gt, columns, n_hyp, hyp_max_boxes, iou_threshold=DEFAULT_IOU_THRESHOLD, g=None):
        """The same form over result columns that are in HBM already: `columns` holds the output tensors of wt_tracks_to_eval_dev by
        the names x, y, w, h, category, h_id, set_row_offsets and frame_hyp_offsets (K, frames + 1), n_hyp is their row count and
        hyp_max_boxes the scalar that call left (the result side of max_frame_boxes; the ground-truth side is computed as in the
        other form).  g: the ground-truth tensors ``self.g`` of an earlier form over the same `gt`, to be used again instead of
        uploaded.  No per-row output is kept: results() gives the tables and ignored_rows, read off the offsets."""
        import torch
        self = cls.__new__(cls)
        self.torch, self.lib, self.gt, self.p = torch, _lib.lib(), gt, None
        self.thr = _lib.as_f64(iou_threshold)
        self.n_classes = int(self.thr.size)
        self.K, self.n_streams, self.n_hyp = int(columns['frame_hyp_offsets'].shape[0]), len(gt['stream_keys']), int(n_hyp)
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.g = g if g is not None else dict((n, self.up(gt[n])) for n in _BOX + ('category', 'level', 'frame_gt_offsets', 'stream_frame_offsets', 'gt_id'))
        self.h = dict(columns)
        self.status = self.zeros(1, torch.int32)
        self.max_boxes = max(int(hyp_max_boxes), max_frame_boxes(gt, {'frame_hyp_offsets': np.zeros((0, 1), np.int64)}, self.n_classes))
        self.hyp_match = self.hyp_switch = None
        self._outputs()
        return self

    def _outputs(self):
        torch = self.torch
        self.counts = self.zeros((self.K, self.n_streams, self.n_classes, 2, 5), torch.int64)
        self.iou_sum = self.zeros((self.K, self.n_streams, self.n_classes, 2), torch.float64)
        self.lib.wt_mot_eval_workspace.restype = C.c_size_t
        self.ws_bytes = int(self.lib.wt_mot_eval_workspace(C.c_int32(self.K), C.c_int32(self.n_streams), C.c_int32(self.n_classes),
                                                           C.c_int64(self.max_boxes), C.c_int32(int(self.gt['max_gt_ids']))))
        if not self.ws_bytes:
            _lib.check(4, 'wt_mot_eval_workspace')
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)

    def launch(self):
        d = self.d
        rc = self.lib.wt_mot_eval_dev(
            *self.leading_args(self.g['gt_id'], self.h['h_id']),
            C.c_int32(self.n_classes), _lib.ptr(self.thr), C.c_int64(self.max_boxes), C.c_int32(int(self.gt['max_gt_ids'])),
            d(self.counts), d(self.iou_sum), d(self.hyp_match) if self.hyp_match is not None else None,
            d(self.hyp_switch) if self.hyp_switch is not None else None, d(self.status),
            d(self.ws), C.c_size_t(self.ws_bytes), C.c_void_p(self.torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, self.name)

    def results(self, per_row=False):
        self.wait()
        if self.p is None:                               # from_device: the rows stayed in HBM, so there is nothing per row to give
            if per_row:
                raise ValueError('a DeviceEvaluation over device-resident columns keeps no per-row output')
            rows = np.diff(self.h['set_row_offsets'].cpu().numpy()[:self.K + 1])
            on = self.h['frame_hyp_offsets'][:, -1].cpu().numpy()
            counts, iou_sum = self.counts.cpu().numpy(), self.iou_sum.cpu().numpy()
            return [MotResult(counts[k], iou_sum[k], int(rows[k] - on[k]), self.gt['stream_keys']) for k in range(self.K)]
        return _results(self.gt, self.p, self.counts.cpu().numpy(), self.iou_sum.cpu().numpy(),
                        self.hyp_match.cpu().numpy()[:self.n_hyp], self.hyp_switch.cpu().numpy()[:self.n_hyp], per_row)


class _DeviceTrajectoryForm(_DeviceForm):
    """What DeviceIdentity and DeviceHota share beyond _DeviceForm: the trajectory columns and counts in HBM, their maxima, the
    offsets of every problem's matrices, and the workspace tensor."""

    def set_up_matrices(self, sizes, workspace, workspace_bytes):
        """sizes(g_ntraj, h_ntraj): the matrix elements per problem; workspace(total elements) -> bytes, 0 is refused.  Returns the total."""
        g_traj, self.g_ntraj, h_traj, self.h_ntraj = trajectory_indices(self.gt, self.p, self.n_classes)
        self.max_g, self.max_h = _max(self.g_ntraj), _max(self.h_ntraj)
        mat_offsets = np.concatenate([[0], np.cumsum(sizes(self.g_ntraj, self.h_ntraj).reshape(-1))]).astype(np.int64)
        self.ws_bytes = workspace(int(mat_offsets[-1]))
        if not self.ws_bytes:
            _lib.check(4, self.name.replace('_dev', '_workspace'))
        self.g['traj'], self.h['traj'] = self.up(g_traj), self.up(h_traj)
        self.g['ntraj'], self.h['ntraj'], self.mat_offsets = self.up(self.g_ntraj), self.up(self.h_ntraj), self.up(mat_offsets)
        self.ws = self.torch.empty(self.ws_bytes if workspace_bytes is None else int(workspace_bytes), dtype=self.torch.uint8, device=self.device)
        return int(mat_offsets[-1])


# ---------------------------------------------------------------------------------------------------------------
# identity preservation (IDF1 / IDP / IDR)
ID_FIELDS = ('idtp', 'gt', 'hyp')
DEFAULT_WORKSPACE_LIMIT = 1 << 30                  # bytes of device workspace one wt_mot_identity call may ask for


def _local_index(group, ident, n_groups):
    """Rows with group >= 0: number the distinct `ident` values inside every group from 0.  Returns (index per row, 0 for the
    other rows; count per group)."""
    index = np.zeros(group.size, np.int32)
    ok = group >= 0
    if not ok.any():
        return index, np.zeros(n_groups, np.int32)
    base = int(ident[ok].max()) + 1
    u, inv = np.unique(group[ok] * base + ident[ok], return_inverse=True)
    ug = u // base
    first = np.searchsorted(ug, np.arange(n_groups))
    index[ok] = (inv - first[ug[inv]]).astype(np.int32)
    return index, np.bincount(ug, minlength=n_groups).astype(np.int32)


def trajectory_indices(gt, packed, n_classes):
    """Class-local trajectory indices of wt_mot_identity_* (include/waymotrack.h) for pack_results() output:
    g_traj, g_ntraj (n_streams, n_classes), h_traj, h_ntraj (K, n_streams, n_classes)."""
    n_streams = len(gt['stream_keys'])
    sfo = gt['stream_frame_offsets']

    def groups(cat, frame_offsets, first):
        n = int(frame_offsets[-1])
        frame = np.searchsorted(frame_offsets, np.arange(n), side='right') - 1
        stream = np.searchsorted(sfo, frame, side='right') - 1
        c = cat[:n].astype(np.int64)
        return np.where((c >= 1) & (c <= n_classes), (first + stream) * n_classes + c - 1, -1)
    g_group = groups(gt['category'], gt['frame_gt_offsets'], 0) if gt['frame_ids'].size else np.zeros(0, np.int64)
    g_traj, g_ntraj = _local_index(g_group, gt['gt_id'].astype(np.int64)[:g_group.size], n_streams * n_classes)
    set_rows = packed['set_row_offsets']
    K = len(set_rows) - 1
    h_group = np.full(int(set_rows[-1]), -1, np.int64)
    for k in range(K):
        lo = int(set_rows[k])
        on = groups(packed['category'][lo:], packed['frame_hyp_offsets'][k], k * n_streams)
        h_group[lo:lo + on.size] = on
    h_traj, h_ntraj = _local_index(h_group, packed['h_id'].astype(np.int64), K * n_streams * n_classes)
    return (np.ascontiguousarray(g_traj), g_ntraj.reshape(n_streams, n_classes),
            np.ascontiguousarray(h_traj), h_ntraj.reshape(K, n_streams, n_classes))


def _matrix_floats(g_ntraj, h_ntraj):
    """Per problem, the floats of its two matrices: 2 * min * (max | 1) (munkres_ld of csrc/sort_device.h)."""
    g = np.broadcast_to(g_ntraj.astype(np.int64), h_ntraj.shape)
    h = h_ntraj.astype(np.int64)
    return 2 * np.minimum(g, h) * (np.maximum(g, h) | 1)


def identity_row(idtp, gt, hyp):
    return {'idtp': int(idtp), 'idfn': int(gt - idtp), 'idfp': int(hyp - idtp), 'gt': int(gt), 'hyp': int(hyp),
            'idp': idtp / hyp if hyp else math.nan, 'idr': idtp / gt if gt else math.nan,
            'idf1': 2 * idtp / (gt + hyp) if gt + hyp else math.nan}


class IdentityResult(_Scores):
    """Identity scores of one tracking result.

    id_counts   (n_streams, n_classes, 2, 3) int64: idtp, gt, hyp for LEVEL_1, LEVEL_2, per stream
    table       row = idtp, idfn, idfp, gt, hyp, idp, idr, idf1 (counts summed stream by stream)
    ignored_rows   result rows that took no part
    hyp_idmatch (with per_row=True) (rows, 2) int64 in file order, LEVEL_1 then LEVEL_2: index of the identity-matched annotation
                in the ground-truth file's list, -1 not matched, -2 took no part or left out at that level."""

    def __init__(self, id_counts, ignored_rows, stream_keys, hyp_idmatch=None):
        self.id_counts, self.ignored_rows, self.stream_keys, self.hyp_idmatch = id_counts, ignored_rows, stream_keys, hyp_idmatch
        self.fill_table(id_counts.shape[1])

    def row(self, classes, li):
        return identity_row(*(int(v) for v in _added(self.id_counts, classes, li)))

    def idf1(self, level=2, category='ALL'):
        return self.table[category][level]['idf1']


def _identity_results(gt, packed, id_counts, hyp_idmatch, per_row):
    return [IdentityResult(id_counts[k], ignored, gt['stream_keys'], _file_order(gt, packed, k, hyp_idmatch[lo:hi]) if per_row else None)
            for k, lo, hi, ignored in _result_sets(packed)]


def _identity_workspace(lib, k, n_streams, n_classes, max_g, max_h, floats):
    lib.wt_mot_identity_workspace.restype = C.c_size_t
    return int(lib.wt_mot_identity_workspace(C.c_int32(k), C.c_int32(n_streams), C.c_int32(n_classes), C.c_int64(max_g), C.c_int64(max_h),
                                             C.c_int64(floats)))


def _max(a):
    return int(a.max()) if a.size else 0


def _calls(K, need, limit):
    """Consecutive result sets per call: as many as fit the workspace limit, at least one.  need(k0, k1): the bytes sets k0:k1 ask for
    (0 = more than the library sizes)."""
    calls, k0 = [], 0
    while k0 < K:
        k1 = k0 + 1
        while k1 < K:
            n = need(k0, k1 + 1)
            if n == 0 or (limit and n > limit):
                break
            k1 += 1
        calls.append((k0, k1))
        k0 = k1
    return calls


def _identity_calls(lib, g_ntraj, h_ntraj, limit):
    K, n_streams, n_classes = h_ntraj.shape
    floats = _matrix_floats(g_ntraj, h_ntraj).reshape(K, -1).sum(axis=1)
    max_g = _max(g_ntraj)
    return _calls(K, lambda k0, k1: _identity_workspace(lib, k1 - k0, n_streams, n_classes, max_g, _max(h_ntraj[k0:k1]), int(floats[k0:k1].sum())), limit)


def _call_slice(p, h_traj, h_ntraj, k0, k1):
    """Result sets k0:k1 of pack_results() output as the input of a call of their own: (first row, end row, the columns with
    offsets from 0, their trajectory column, their trajectory counts)."""
    set_rows = p['set_row_offsets']
    lo, hi = int(set_rows[k0]), int(set_rows[k1])
    h = dict((n, p[n][lo:hi]) for n in _BOX + ('category',))
    h['set_row_offsets'] = np.ascontiguousarray(set_rows[k0:k1 + 1] - lo)
    h['frame_hyp_offsets'] = np.ascontiguousarray(p['frame_hyp_offsets'][k0:k1])
    return lo, hi, h, h_traj[lo:hi], np.ascontiguousarray(h_ntraj[k0:k1])


def evaluate_identity(gt, tracks_list, iou_threshold=DEFAULT_IOU_THRESHOLD, per_row=False, workspace_limit_bytes=DEFAULT_WORKSPACE_LIMIT,
                      packed=None):
    """IDF1 / IDP / IDR of K tracking results against one ground truth through wt_mot_identity_host: as few calls as the workspace
    limit allows (the results do not depend on the split).  packed: pack_results() of the same arguments, when the caller has it.
    Returns a list of K IdentityResult."""
    lib = _lib.lib()
    thr = _lib.as_f64(iou_threshold)
    n_classes = int(thr.size)
    p = packed if packed is not None else pack_results(gt, tracks_list, n_classes)
    g_traj, g_ntraj, h_traj, h_ntraj = trajectory_indices(gt, p, n_classes)
    K = len(tracks_list)
    n_streams = len(gt['stream_keys'])
    id_counts = np.zeros((K, n_streams, n_classes, 2, 3), np.int64)
    hyp_idmatch = np.full((int(p['set_row_offsets'][-1]), 2), -2, np.int64)
    g_ntraj_c = np.ascontiguousarray(g_ntraj)
    for k0, k1 in _identity_calls(lib, g_ntraj, h_ntraj, workspace_limit_bytes):
        lo, hi, h, ht, hn = _call_slice(p, h_traj, h_ntraj, k0, k1)
        cnt = np.zeros((k1 - k0, n_streams, n_classes, 2, 3), np.int64)
        match = np.full((hi - lo, 2), -2, np.int64)
        rc = lib.wt_mot_identity_host(
            *_gt_args(gt, gt, g_traj, _lib.ptr), *_hyp_args(k1 - k0, None, h, ht, _lib.ptr),
            _lib.ptr(g_ntraj_c), _lib.ptr(hn),
            C.c_int32(n_classes), _lib.ptr(thr), C.c_size_t(int(workspace_limit_bytes or 0)), _lib.ptr(cnt),
            _lib.ptr(match) if per_row else None)
        _lib.check(rc, 'wt_mot_identity_host')
        id_counts[k0:k1] = cnt
        hyp_idmatch[lo:hi] = match
    return _identity_results(gt, p, id_counts, hyp_idmatch, per_row)


class DeviceIdentity(_DeviceTrajectoryForm):
    """evaluate_identity with everything resident in HBM, beside DeviceEvaluation: ``launch()`` enqueues one wt_mot_identity_dev
    on the current torch stream and returns at once, ``results()`` synchronises and reads the outputs back.  All K results go into
    one call; workspace_bytes overrides the size of the workspace tensor (a smaller one is refused by the library)."""
    name = 'wt_mot_identity_dev'

    def __init__(self, gt, tracks_list, iou_threshold=DEFAULT_IOU_THRESHOLD, workspace_bytes=None):
        _DeviceForm.__init__(self, gt, tracks_list, iou_threshold)
        self.matrix_floats = self.set_up_matrices(_matrix_floats, lambda n: _identity_workspace(
            self.lib, self.K, self.n_streams, self.n_classes, self.max_g, self.max_h, n), workspace_bytes)
        self.id_counts = self.zeros((self.K, self.n_streams, self.n_classes, 2, 3), self.torch.int64)
        self.hyp_idmatch = self.zeros((max(1, self.n_hyp), 2), self.torch.int64)

    def launch(self):
        d = self.d
        rc = self.lib.wt_mot_identity_dev(
            *self.leading_args(self.g['traj'], self.h['traj']),
            d(self.g['ntraj']), d(self.h['ntraj']), d(self.mat_offsets), C.c_int64(self.matrix_floats),
            C.c_int32(self.n_classes), _lib.ptr(self.thr), C.c_int64(self.max_g), C.c_int64(self.max_h),
            d(self.id_counts), d(self.hyp_idmatch), d(self.status),
            d(self.ws), C.c_size_t(int(self.ws.numel())), C.c_void_p(self.torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, self.name)

    def results(self, per_row=False):
        self.wait()
        return _identity_results(self.gt, self.p, self.id_counts.cpu().numpy(), self.hyp_idmatch.cpu().numpy()[:self.n_hyp], per_row)


# ---------------------------------------------------------------------------------------------------------------
# HOTA (DetA / AssA / LocA over 19 localisation thresholds)
N_ALPHAS = 19
HOTA_SUMS = ('ass', 'assre', 'asspr', 'loc')
HOTA_NAMES = ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA')


def _matrix_cells(g_ntraj, h_ntraj):
    """Per problem, the cells of its two matrices (LEVEL_1, LEVEL_2): 2 * g * h."""
    return 2 * np.broadcast_to(g_ntraj.astype(np.int64), h_ntraj.shape) * h_ntraj.astype(np.int64)


def hota_row(gt, hyp, tp, sums):
    """Added counts (gt, hyp, tp[19]) and sums ((19, 4): ass, assre, asspr, loc) -> the reported row: the eight scores averaged
    over the thresholds (LocA over those with a match), HOTA(0), LocA(0) and 'per_alpha' with the 19 values of each.  NaN where a
    denominator is 0; the association scores of a threshold without a match are 0."""
    gt, hyp = int(gt), int(hyp)
    per = dict((n, []) for n in HOTA_NAMES)
    div = lambda a, b: a / b if b else math.nan
    for a in range(N_ALPHAS):
        t = int(tp[a])
        ass, assre, asspr, loc = (float(v) for v in sums[a])
        per['DetA'].append(div(t, gt + hyp - t))
        per['DetRe'].append(div(t, gt))
        per['DetPr'].append(div(t, hyp))
        per['AssA'].append(ass / t if t else 0.0)
        per['AssRe'].append(assre / t if t else 0.0)
        per['AssPr'].append(asspr / t if t else 0.0)
        per['LocA'].append(div(loc, t))
        per['HOTA'].append(math.sqrt(per['DetA'][a] * per['AssA'][a]) if gt + hyp else math.nan)
    row = {'gt': gt, 'hyp': hyp, 'tp': [int(v) for v in tp]}
    for n in HOTA_NAMES:
        vals = per[n] if n != 'LocA' else [v for v, t in zip(per[n], tp) if t > 0]
        total = 0.0
        for v in vals:                               # one after the other, a ascending
            total = total + v
        row[n] = total / len(vals) if vals else math.nan
    row['HOTA(0)'], row['LocA(0)'] = per['HOTA'][0], per['LocA'][0]
    row['per_alpha'] = per
    return row


def _hota_added(counts, sums, classes, li):
    """Counts and sums of `classes` at level index li, added class by class, stream by stream (the order is part of the definition)."""
    cnt = np.zeros(2 + N_ALPHAS, np.int64)
    tot = np.zeros((N_ALPHAS, 4), np.float64)
    for cc in classes:
        for s in range(counts.shape[0]):
            cnt += counts[s, cc - 1, li]
            tot = tot + sums[s, cc - 1, li]
    return cnt, tot


class HotaResult(_Scores):
    """HOTA scores of one tracking result.

    hota_counts (n_streams, n_classes, 2, 21) int64: gt, hyp, tp[19] for LEVEL_1, LEVEL_2, per stream
    hota_sums   (n_streams, n_classes, 2, 19, 4) float64: ass, assre, asspr, loc per threshold alpha_a = (a + 1) / 20
    table       row = hota_row() of the added counts, plus 'sums'
    ignored_rows   result rows that took no part
    hyp_match   (with per_row=True) (rows, 2) int64 in file order, LEVEL_1 then LEVEL_2: index of the annotation in the ground-truth
                file's list that the frame's assignment gave the box, -1 unmatched, -2 took no part or removed at that level."""

    def __init__(self, hota_counts, hota_sums, ignored_rows, stream_keys, hyp_match=None):
        self.hota_counts, self.hota_sums, self.ignored_rows, self.stream_keys = hota_counts, hota_sums, ignored_rows, stream_keys
        self.hyp_match = hyp_match
        self.fill_table(hota_counts.shape[1])

    def row(self, classes, li):
        cnt, tot = _hota_added(self.hota_counts, self.hota_sums, classes, li)
        row = hota_row(cnt[0], cnt[1], cnt[2:], tot)
        row['sums'] = dict((n, tot[:, i].tolist()) for i, n in enumerate(HOTA_SUMS))
        return row

    def hota(self, level=2, category='ALL'):
        return self.table[category][level]['HOTA']


def _hota_results(gt, packed, hota_counts, hota_sums, hyp_match, per_row):
    return [HotaResult(hota_counts[k], hota_sums[k], ignored, gt['stream_keys'], _file_order(gt, packed, k, hyp_match[lo:hi]) if per_row else None)
            for k, lo, hi, ignored in _result_sets(packed)]


def _hota_workspace(lib, k, n_streams, n_classes, max_boxes, max_g, max_h, cells):
    lib.wt_mot_hota_workspace.restype = C.c_size_t
    return int(lib.wt_mot_hota_workspace(C.c_int32(k), C.c_int32(n_streams), C.c_int32(n_classes), C.c_int64(max_boxes), C.c_int64(max_g),
                                         C.c_int64(max_h), C.c_int64(cells)))


def _hota_calls(lib, g_ntraj, h_ntraj, max_boxes, limit):
    """max_boxes: the bound of the whole input (a smaller per-call bound would only shrink the workspace)."""
    K, n_streams, n_classes = h_ntraj.shape
    cells = _matrix_cells(g_ntraj, h_ntraj).reshape(K, -1).sum(axis=1)
    max_g = _max(g_ntraj)
    return _calls(K, lambda k0, k1: _hota_workspace(lib, k1 - k0, n_streams, n_classes, max_boxes, max_g, _max(h_ntraj[k0:k1]), int(cells[k0:k1].sum())), limit)


def evaluate_hota(gt, tracks_list, iou_threshold=DEFAULT_IOU_THRESHOLD, per_row=False, workspace_limit_bytes=DEFAULT_WORKSPACE_LIMIT,
                  packed=None):
    """HOTA / DetA / AssA / LocA of K tracking results against one ground truth through wt_mot_hota_host: as few calls as the
    workspace limit allows (the results do not depend on the split).  iou_threshold: the class thresholds, used by LEVEL_1's
    removal rule only.  packed: pack_results() of the same arguments, when the caller has it.  Returns a list of K HotaResult."""
    lib = _lib.lib()
    thr = _lib.as_f64(iou_threshold)
    n_classes = int(thr.size)
    p = packed if packed is not None else pack_results(gt, tracks_list, n_classes)
    g_traj, g_ntraj, h_traj, h_ntraj = trajectory_indices(gt, p, n_classes)
    K = len(tracks_list)
    n_streams = len(gt['stream_keys'])
    hota_counts = np.zeros((K, n_streams, n_classes, 2, 2 + N_ALPHAS), np.int64)
    hota_sums = np.zeros((K, n_streams, n_classes, 2, N_ALPHAS, 4), np.float64)
    hyp_match = np.full((int(p['set_row_offsets'][-1]), 2), -2, np.int64)
    g_ntraj_c = np.ascontiguousarray(g_ntraj)
    for k0, k1 in _hota_calls(lib, g_ntraj, h_ntraj, max_frame_boxes(gt, p, n_classes), workspace_limit_bytes):
        lo, hi, h, ht, hn = _call_slice(p, h_traj, h_ntraj, k0, k1)
        cnt = np.zeros((k1 - k0,) + hota_counts.shape[1:], np.int64)
        sums = np.zeros((k1 - k0,) + hota_sums.shape[1:], np.float64)
        match = np.full((hi - lo, 2), -2, np.int64)
        rc = lib.wt_mot_hota_host(
            *_gt_args(gt, gt, g_traj, _lib.ptr), *_hyp_args(k1 - k0, None, h, ht, _lib.ptr),
            _lib.ptr(g_ntraj_c), _lib.ptr(hn),
            C.c_int32(n_classes), _lib.ptr(thr), C.c_size_t(int(workspace_limit_bytes or 0)), _lib.ptr(cnt), _lib.ptr(sums),
            _lib.ptr(match) if per_row else None)
        _lib.check(rc, 'wt_mot_hota_host')
        hota_counts[k0:k1] = cnt
        hota_sums[k0:k1] = sums
        hyp_match[lo:hi] = match
    return _hota_results(gt, p, hota_counts, hota_sums, hyp_match, per_row)


class DeviceHota(_DeviceTrajectoryForm):
    """evaluate_hota with everything resident in HBM, beside DeviceEvaluation and DeviceIdentity: ``launch()`` enqueues one
    wt_mot_hota_dev on the current torch stream and returns at once, ``results()`` synchronises and reads the outputs back.  All K
    results go into one call; workspace_bytes overrides the size of the workspace tensor (a smaller one is refused by the library)."""
    name = 'wt_mot_hota_dev'

    def __init__(self, gt, tracks_list, iou_threshold=DEFAULT_IOU_THRESHOLD, workspace_bytes=None):
        _DeviceForm.__init__(self, gt, tracks_list, iou_threshold)
        self.max_boxes = max_frame_boxes(gt, self.p, self.n_classes)
        self.matrix_cells = self.set_up_matrices(_matrix_cells, lambda n: _hota_workspace(
            self.lib, self.K, self.n_streams, self.n_classes, self.max_boxes, self.max_g, self.max_h, n), workspace_bytes)
        self.hota_counts = self.zeros((self.K, self.n_streams, self.n_classes, 2, 2 + N_ALPHAS), self.torch.int64)
        self.hota_sums = self.zeros((self.K, self.n_streams, self.n_classes, 2, N_ALPHAS, 4), self.torch.float64)
        self.hyp_match = self.zeros((max(1, self.n_hyp), 2), self.torch.int64)

    def launch(self):
        d = self.d
        rc = self.lib.wt_mot_hota_dev(
            *self.leading_args(self.g['traj'], self.h['traj']),
            d(self.g['ntraj']), d(self.h['ntraj']), d(self.mat_offsets), C.c_int64(self.matrix_cells),
            C.c_int32(self.n_classes), _lib.ptr(self.thr), C.c_int64(self.max_boxes), C.c_int64(self.max_g), C.c_int64(self.max_h),
            d(self.hota_counts), d(self.hota_sums), d(self.hyp_match), d(self.status),
            d(self.ws), C.c_size_t(int(self.ws.numel())), C.c_void_p(self.torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, self.name)

    def results(self, per_row=False):
        self.wait()
        return _hota_results(self.gt, self.p, self.hota_counts.cpu().numpy(), self.hota_sums.cpu().numpy(),
                             self.hyp_match.cpu().numpy()[:self.n_hyp], per_row)


# ---------------------------------------------------------------------------------------------------------------
# trajectory coverage (MT / PT / ML, fragmentations)
COV_FIELDS = ('traj', 'mt', 'pt', 'ml', 'frag')
TRAJ_FIELDS = ('len', 'tracked', 'frag', 'idsw')


def coverage_row(traj, mt, pt, ml, frag):
    """Added counts -> the reported row: the counts, MT = mt / traj, ML = ml / traj (NaN without a trajectory) and FM = frag."""
    traj, mt, pt, ml, frag = int(traj), int(mt), int(pt), int(ml), int(frag)
    return {'traj': traj, 'mt': mt, 'pt': pt, 'ml': ml, 'frag': frag,
            'MT': mt / traj if traj else math.nan, 'ML': ml / traj if traj else math.nan, 'FM': frag}


class CoverageResult(_Scores):
    """What became of the ground-truth trajectories under one tracking result (the matching is that of MotResult).

    cov_counts  (n_streams, n_classes, 2, 5) int64: traj, mt, pt, ml, frag for LEVEL_1, LEVEL_2, per stream
    table       row = coverage_row() of the added counts
    ignored_rows   result rows that took no part
    traj_stats  (with per_trajectory=True) (trajectories, 2, 4) int32: len, tracked, frag, idsw for LEVEL_1, LEVEL_2
    traj_keys   (with per_trajectory=True) one (stream key, class, object id) per row of traj_stats."""

    def __init__(self, cov_counts, ignored_rows, stream_keys, traj_stats=None, traj_keys=None):
        self.cov_counts, self.ignored_rows, self.stream_keys = cov_counts, ignored_rows, stream_keys
        self.traj_stats, self.traj_keys = traj_stats, traj_keys
        self.fill_table(cov_counts.shape[1])

    def row(self, classes, li):
        return coverage_row(*_added(self.cov_counts, classes, li))

    def mt(self, level=2, category='ALL'):
        return self.table[category][level]['MT']


def _traj_keys(gt, g_traj, g_ntraj):
    """(stream key, class, object id) of every ground-truth trajectory, in the order of traj_stats."""
    n_classes = g_ntraj.shape[1]
    offsets = np.concatenate([[0], np.cumsum(g_ntraj.reshape(-1))]).astype(np.int64)
    keys = [None] * int(offsets[-1])
    n = int(gt['frame_gt_offsets'][-1]) if gt['frame_ids'].size else 0
    frame = np.searchsorted(gt['frame_gt_offsets'], np.arange(n), side='right') - 1
    stream = np.searchsorted(gt['stream_frame_offsets'], frame, side='right') - 1
    for r in range(n):
        c = int(gt['category'][r])
        if 1 <= c <= n_classes:
            s = int(stream[r])
            keys[int(offsets[s * n_classes + c - 1]) + int(g_traj[r])] = (gt['stream_keys'][s], c, gt['object_id'][r])
    return keys


def _coverage_results(gt, packed, cov_counts, traj_stats, keys):
    return [CoverageResult(cov_counts[k], ignored, gt['stream_keys'], None if traj_stats is None else traj_stats[k], keys)
            for k, _, _, ignored in _result_sets(packed)]


def evaluate_coverage(gt, tracks_list, iou_threshold=DEFAULT_IOU_THRESHOLD, per_trajectory=False, packed=None):
    """MT / PT / ML and fragmentations of K tracking results against one ground truth in ONE wt_mot_coverage_host call (the
    CLEAR-MOT matching of evaluate_tracks, then the coverage kernels on the same stream).  packed: pack_results() of the same
    arguments, when the caller has it.  Returns a list of K CoverageResult."""
    lib = _lib.lib()
    thr = _lib.as_f64(iou_threshold)
    n_classes = int(thr.size)
    p = packed if packed is not None else pack_results(gt, tracks_list, n_classes)
    g_traj, g_ntraj, _, _ = trajectory_indices(gt, p, n_classes)
    K = len(tracks_list)
    n_streams = len(gt['stream_keys'])
    total = int(g_ntraj.sum())
    cov_counts = np.zeros((K, n_streams, n_classes, 2, len(COV_FIELDS)), np.int64)
    traj_stats = np.zeros((K, total, 2, len(TRAJ_FIELDS)), np.int32) if per_trajectory else None
    g_args = _gt_args(gt, gt, gt['gt_id'], _lib.ptr)
    rc = lib.wt_mot_coverage_host(
        *(g_args[:8] + [_lib.ptr(g_traj)] + g_args[8:]),               # the trajectory column follows the id column
        *_hyp_args(K, None, p, p['h_id'], _lib.ptr), _lib.ptr(np.ascontiguousarray(g_ntraj)),
        C.c_int32(n_classes), _lib.ptr(thr), _lib.ptr(cov_counts), _lib.ptr(traj_stats) if per_trajectory else None)
    _lib.check(rc, 'wt_mot_coverage_host')
    return _coverage_results(gt, p, cov_counts, traj_stats, _traj_keys(gt, g_traj, g_ntraj) if per_trajectory else None)


class DeviceCoverage(_DeviceForm):
    """evaluate_coverage with everything resident in HBM: ``launch()`` enqueues the evaluation and one wt_mot_coverage_dev on the
    current torch stream and returns at once, ``results()`` synchronises and reads the outputs back.  evaluation: a
    DeviceEvaluation of the same arguments whose launch the caller has already enqueued on this stream (its hyp_match and
    hyp_switch are read where they lie, and only the coverage kernels are paid for); without one the object owns and launches its
    own.  workspace_bytes overrides the size of the workspace tensor (a smaller one is refused by the library)."""
    name = 'wt_mot_coverage_dev'

    def __init__(self, gt, tracks_list, iou_threshold=DEFAULT_IOU_THRESHOLD, per_trajectory=False, evaluation=None, workspace_bytes=None):
        self.own = evaluation is None
        self.ev = DeviceEvaluation(gt, tracks_list, iou_threshold) if self.own else evaluation
        for name in ('torch', 'lib', 'gt', 'thr', 'n_classes', 'p', 'K', 'n_streams', 'n_hyp', 'device', 'g', 'h'):
            setattr(self, name, getattr(self.ev, name))             # the packed results and the columns already in HBM
        torch = self.torch
        self.status = self.zeros(1, torch.int32)                    # a word of its own: the evaluation's is read as well
        g_traj, g_ntraj, _, _ = trajectory_indices(gt, self.p, self.n_classes)
        self.g_traj, self.g_ntraj = g_traj, g_ntraj
        traj_offsets = np.concatenate([[0], np.cumsum(g_ntraj.reshape(-1))]).astype(np.int64)
        self.total_traj = int(traj_offsets[-1])
        self.per_trajectory = per_trajectory
        self.d_traj, self.d_ntraj, self.d_offsets = self.up(g_traj), self.up(g_ntraj), self.up(traj_offsets)
        self.cov_counts = self.zeros((self.K, self.n_streams, self.n_classes, 2, len(COV_FIELDS)), torch.int64)
        self.traj_stats = self.zeros((self.K, max(1, self.total_traj), 2, len(TRAJ_FIELDS)), torch.int32) if per_trajectory else None
        self.lib.wt_mot_coverage_workspace.restype = C.c_size_t
        self.ws_bytes = int(self.lib.wt_mot_coverage_workspace(C.c_int32(self.K), C.c_int32(self.n_streams), C.c_int32(self.n_classes),
                                                               C.c_int64(int(gt['x'].size)), C.c_int64(self.total_traj)))
        if not self.ws_bytes:
            _lib.check(4, 'wt_mot_coverage_workspace')
        self.ws = torch.empty(self.ws_bytes if workspace_bytes is None else int(workspace_bytes), dtype=torch.uint8, device=self.device)

    def launch(self, pass_events=None):
        """pass_events: four recorded torch.cuda.Event(enable_timing=True), re-recorded around the passes (tools/mot_coverage_bench.py)."""
        if self.own:
            self.ev.launch()
        d, g = self.d, self.g
        events = None
        if pass_events is not None:
            events = (C.c_void_p * 4)(*[e.cuda_event for e in pass_events])
        rc = self.lib.wt_mot_coverage_dev(
            C.c_int64(self.gt['x'].size), d(g['category']), d(g['level']), d(self.d_traj),
            C.c_int64(self.gt['frame_ids'].size), d(g['frame_gt_offsets']), C.c_int32(self.n_streams), d(g['stream_frame_offsets']),
            C.c_int32(self.n_classes), d(self.d_ntraj), d(self.d_offsets), C.c_int64(self.total_traj),
            C.c_int32(self.K), C.c_int64(self.n_hyp), d(self.h['set_row_offsets']), d(self.ev.hyp_match), d(self.ev.hyp_switch),
            d(self.cov_counts), d(self.traj_stats) if self.per_trajectory else None, d(self.status),
            d(self.ws), C.c_size_t(int(self.ws.numel())), C.c_void_p(self.torch.cuda.current_stream().cuda_stream), events)
        _lib.check(rc, self.name)

    def results(self):
        self.ev.wait()
        self.wait()
        stats = self.traj_stats.cpu().numpy()[:, :self.total_traj] if self.per_trajectory else None
        return _coverage_results(self.gt, self.p, self.cov_counts.cpu().numpy(), stats,
                                 _traj_keys(self.gt, self.g_traj, self.g_ntraj) if self.per_trajectory else None)


# ---------------------------------------------------------------------------------------------------------------
# the printed tables: one formatter, one column spec (row key = heading, format) per metric
_D, _F = '%9d', '%9.5f'
_MOT_COLUMNS = tuple((k, _D) for k in FIELDS[:4]) + (('idsw', '%7d'), ('MOTA', _F), ('MOTP', _F))
_ID_COLUMNS = tuple((k, _D) for k in ('idtp', 'idfn', 'idfp')) + tuple((k, _F) for k in ('idf1', 'idp', 'idr'))
_HOTA_COLUMNS = tuple((k, _F) for k in HOTA_NAMES + ('HOTA(0)', 'LocA(0)'))
_COV_COLUMNS = tuple((k, _D) for k in ('traj', 'mt', 'pt', 'ml')) + (('MT', _F), ('ML', _F), ('FM', _D))


def _format_rows(result, title, columns, heading=str):
    lines = [title, '%-6s %-8s' % ('class', 'level') + ''.join(' %*s' % (int(f[1]), heading(k)) for k, f in columns)]
    for c, rows in result.table.items():
        for lv in LEVELS:
            lines.append('%-6s LEVEL_%d ' % (c, lv) + ''.join(' ' + f % rows[lv][k] for k, f in columns))
    return '\n'.join(lines)


def format_table(result, name=''):
    return _format_rows(result, '%s  (ignored rows: %d)' % (name, result.ignored_rows), _MOT_COLUMNS)


def format_identity_table(result, name=''):
    return _format_rows(result, '%s  identity' % name, _ID_COLUMNS, str.upper)


def format_hota_table(result, name=''):
    return _format_rows(result, '%s  HOTA' % name, _HOTA_COLUMNS)


def format_coverage_table(result, name=''):
    return _format_rows(result, '%s  coverage' % name, _COV_COLUMNS)


# ---------------------------------------------------------------------------------------------------------------
# the metrics, as the sweep's ranking and main() use them
def _counter(fields):
    """(start, add) of a total that adds `fields` of class rows."""
    def add(total, row):
        for f in fields:
            total[f] += row[f]
        return total
    return (lambda: dict((f, 0) for f in fields)), add


def _highest(key):
    """Class pick: the highest row[key], NaN (nothing on either side) last."""
    return lambda row: -row[key] if row[key] == row[key] else math.inf


def _hota_add(total, r):
    return [total[0] + np.asarray([r['gt'], r['hyp']] + r['tp'], np.int64), total[1] + np.asarray([r['sums'][n] for n in HOTA_SUMS], np.float64).T]


def _hota_finish(total):
    r = hota_row(total[0][0], total[0][1], total[0][2:], total[1])
    out = dict((n, r[n]) for n in ('HOTA', 'DetA', 'AssA', 'LocA'))
    out['hota_counts'] = {'gt': r['gt'], 'hyp': r['hyp'], 'tp': r['tp'], 'sums': dict((n, total[1][:, i].tolist()) for i, n in enumerate(HOTA_SUMS))}
    return out


def _coverage_finish(total):
    r = coverage_row(*[total[f] for f in COV_FIELDS])
    return {'MT': r['MT'], 'PT': r['pt'] / r['traj'] if r['traj'] else math.nan, 'ML': r['ML'], 'FM': r['FM'], 'coverage_counts': total}


# name: the --rank-by value; option: what switches the metric on (None: always); evaluate: the function, looked up when it is called;
# results / tables / section: its keys in sweep()'s return value, the sweep's JSON document and a result's JSON document; pick: class
# row -> what the per-class pick minimises (ties: grid order); start, add, finish: the total of the picks' class rows, added class
# by class, and the keys it gives the combined row, `key` being the one the rows are ranked by; table, line: the printed forms
_Metric = collections.namedtuple('_Metric', 'name option evaluate results tables section key pick start add finish table line')
METRICS = (
    # gt is the same for every setting: fewest errors = highest MOTA
    _Metric('mota', None, 'evaluate_tracks', 'results', 'tables', None, 'MOTA', lambda row: row['fn'] + row['fp'] + row['idsw'], *_counter(FIELDS),
            finish=lambda t: {'MOTA': 1.0 - (t['fn'] + t['fp'] + t['idsw']) / t['gt'] if t['gt'] else math.nan, 'counts': t},
            table=format_table, line=lambda r: '  MOTA %9.5f' % r['MOTA']),
    _Metric('idf1', 'identity', 'evaluate_identity', 'id_results', 'identity_tables', 'identity', 'IDF1', _highest('idf1'), *_counter(ID_FIELDS),
            finish=lambda t: {'IDF1': identity_row(t['idtp'], t['gt'], t['hyp'])['idf1'], 'id_counts': t},
            table=format_identity_table, line=lambda r: '  IDF1 %9.5f' % r['IDF1']),
    _Metric('hota', 'hota', 'evaluate_hota', 'hota_results', 'hota_tables', 'hota', 'HOTA', _highest('HOTA'),
            lambda: [np.zeros(2 + N_ALPHAS, np.int64), np.zeros((N_ALPHAS, 4), np.float64)], _hota_add, _hota_finish,
            table=format_hota_table, line=lambda r: '  HOTA %9.5f' % r['HOTA']),
    # traj is the same for every setting: most mostly-tracked trajectories = highest MT
    _Metric('mt', 'coverage', 'evaluate_coverage', 'coverage_results', 'coverage_tables', 'coverage', 'MT', _highest('mt'), *_counter(COV_FIELDS),
            finish=_coverage_finish, table=format_coverage_table, line=lambda r: '  MT %9.5f  ML %9.5f  FM %d' % (r['MT'], r['ML'], r['FM'])))
_PRINT_ORDER = (METRICS[0], METRICS[3], METRICS[1], METRICS[2])       # a result's coverage table follows the matching it reads


# ---------------------------------------------------------------------------------------------------------------
# threshold sweep ("Structure of the sweep")
def _grid_values(text):
    """'0.5:1.0:0.05' (inclusive range) or '0.0,0.01,0.1' -> list of floats."""
    if ':' in text:
        lo, hi, step = (float(v) for v in text.split(':'))
        n = int(math.floor((hi - lo) / step + 1e-9)) + 1
        return [round(lo + i * step, 10) for i in range(n)]
    return [float(v) for v in text.split(',')]


def _int_values(text):
    return [int(v) for v in text.split(',')]


class _Axis(object):
    """One swept parameter of a pass.  grid[key] lists its values (`text`: the default as --KEY-grid takes it); a value becomes
    job[job] of the stage call and row[row] of the setting, and the combined row lists one value per class under `combined`,
    which tracking/track.py takes as `flag`.  switch: the pass is live when the values differ from the default.  A class that is
    not evaluated gets, in the combined row, the default (off) value of a switch and the first grid value of another axis - or a
    copy of the combined row's `rest` list."""

    def __init__(self, key, text, cast, job, flag, help, row=None, combined=None, switch=True, rest=None):
        self.key, self.text, self.cast, self.job, self.flag, self.help, self.switch, self.rest = key, text, cast, job, flag, help, switch, rest
        self.row = row or key
        self.combined = combined or self.row
        self.default = self.parse(text)

    def parse(self, text):
        if not text and not self.text:                # an axis that is empty by default
            return []
        return _int_values(text) if self.cast is int else _grid_values(text)

    def join(self, values):
        return ','.join('%d' % v if self.cast is int else repr(float(v)) for v in values)


class _Single(object):
    """One parameter of a pass that is not swept: grid[key] (one value) goes into every job as job[job] and into the combined
    row under its key; tracking/track.py takes it as --KEY, written when it differs from the default (always: in any case)."""

    def __init__(self, key, default, cast, job, fmt, help, choices=None, always=False):
        self.key, self.default, self.cast, self.job, self.fmt, self.help, self.choices, self.always = key, default, cast, job, fmt, help, choices, always
        self.flag = '--' + key.replace('_', '-')


class _Pass(object):
    """One entry of the table of passes.  stage: the function of tracking/<name>.py that runs it - module and function are looked
    up when a live pass runs, not before; indexed: its jobs carry 'result', the index of their input among the results so far."""

    def __init__(self, name, axes, singles=(), stage=None, indexed=True):
        self.name, self.axes, self.singles, self.stage, self.indexed = name, axes, singles, stage, indexed

    def run(self, packed, outs, jobs, n_classes):
        """Every result of `outs` under every job in ONE call of the stage; the outputs are result-major, job-minor."""
        if self.indexed:
            jobs = [dict(job, result=k) for k in range(len(outs)) for job in jobs]
        return getattr(importlib.import_module('.' + self.name, __package__), self.stage)(packed, outs, jobs, n_classes)


# the tracker's second association (utils.track_packed_byte): its points are tracked, the axes just inside (score, iou)
SECOND = _Pass('second', (
    _Axis('low_score', '', float, 'low_score', '--low-score-threshold', 'second association of the tracker: detections from this score on may continue an unmatched track '
          '(tracking/track.py --low-score-threshold; a value above the point\'s score is clamped to it; empty = off)',
          combined='low_score_threshold', rest='score_threshold'),   # classes that are not evaluated have nothing between low and high
    _Axis('low_iou', '0.5', float, 'low_iou', '--low-iou-threshold', 'second association: lowest IoU of a low-score detection and its track; read when --low-score-grid is set',
          combined='low_iou_threshold', switch=False)))
# the post-passes in the order tracking/track.py chains them: outermost axes first
PASSES = (
    _Pass('split', (
        _Axis('split_iou', '0', float, 'split_iou', '--split-iou', 'track splitting: a track is cut where the extrapolated boxes overlap by less than this IoU (tracking/split.py)'),), (
        _Single('split_gap', 0, int, 'split_gap', '%d', 'track splitting: a track is cut where more than this many frames lie between two boxes; read when --split-iou-grid is set'),
        _Single('split_motion', 'linear', str, 'motion', '%s', 'track splitting: how a box is extrapolated', choices=('linear', 'hold'))),
        stage='split_tracks', indexed=False),
    _Pass('stitch', (
        _Axis('link_gap', '0', int, 'max_link', '--link-gap', 'track stitching: tracks are linked across up to this many frames (tracking/stitch.py)'),
        _Axis('link_iou', '0.3', float, 'link_iou', '--link-iou', 'track stitching: lowest IoU of the extrapolated and the new box; read when --link-gap-grid is set', switch=False)), (
        _Single('link_motion', 'hold', str, 'motion', '%s', 'track stitching: how an ended track is extrapolated', choices=('hold', 'linear')),),
        stage='stitch_tracks', indexed=False),
    _Pass('dedup', (
        _Axis('dedup_frames', '0', int, 'min_frames', '--dedup-frames', 'track deduplication: a track is dropped when a stronger one overlaps it in this many frames (tracking/dedup.py)'),
        _Axis('dedup_iou', '0.7', float, 'dup_iou', '--dedup-iou', 'track deduplication: lowest IoU of the two boxes that counts; read when --dedup-frames-grid is set', switch=False)), (
        _Single('dedup_frac', 0.5, float, 'dup_frac', '%r', 'track deduplication: lowest share of the shorter track\'s frames that must count', always=True),),
        stage='dedup_tracks'),
    _Pass('refine', (
        _Axis('gap', '0', int, 'max_gap', '--interpolate-gap', 'track refinement: gaps of up to this many frames are interpolated (tracking/refine.py)', row='interp_gap'),
        _Axis('min_len', '1', int, 'min_len', '--min-track-len', 'track refinement: tracks observed in fewer frames are dropped')),
        stage='refine_tracks'),
    _Pass('smooth', (
        _Axis('smooth_window', '0', int, 'window', '--smooth-window', 'track smoothing: boxes are averaged over up to this many frames to either side (tracking/smooth.py)'),
        _Axis('smooth_sigma', '1.0', float, 'sigma', '--smooth-sigma', 'track smoothing: width of the gaussian weights; read when --smooth-window-grid is set', switch=False)), (
        _Single('smooth_kernel', 'gaussian', str, 'kernel', '%s', 'track smoothing: the weights over the window', choices=('gaussian', 'box')),),
        stage='smooth_tracks'))
# refinement was the sweep's first pass: the keys of a ranked row and the command line's help list it before the others
_KEY_ORDER = (SECOND, PASSES[3]) + PASSES[:3] + PASSES[4:]


class _Plan(object):
    """A pass under one grid: values (one list per axis), singles {key: value}, on, and points - one (job, keys of the setting row)
    per combination of the values, first axis outermost.  The one empty point of a pass that is off leaves results and rows alone."""

    def __init__(self, p, grid):
        self.values = [[a.cast(v) for v in grid.get(a.key, a.default)] for a in p.axes]
        self.singles = dict((s.key, s.cast(grid.get(s.key, s.default))) for s in p.singles)
        self.on = any(v != a.default for a, v in zip(p.axes, self.values) if a.switch)
        fixed = [(s.job, self.singles[s.key]) for s in p.singles]
        self.points = [({}, {})]
        if self.on:
            self.points = [(dict([(a.job, v) for a, v in zip(p.axes, point)] + fixed), dict((a.row, v) for a, v in zip(p.axes, point)))
                           for point in itertools.product(*self.values)]
        self.jobs = [job for job, _ in self.points]


def _tracked_points(grid, second):
    """The tracker's runs in grid order - max_age, min_hits, score, iou, then the second association's points: (the row the run's
    settings begin with, the tracker's arguments).  A low score above the point's score is clamped to it: that point is plain tracking."""
    for max_age, min_hits, score, iou, low in itertools.product(grid['max_age'], grid['min_hits'], grid['score'], grid['iou'], second.jobs):
        row = {'max_age': int(max_age), 'min_hits': int(min_hits), 'score': float(score), 'iou': float(iou)}
        if second.on:
            low = (min(low['low_score'], float(score)), low['low_iou'])
            row.update(low_score=low[0], low_iou=low[1])
        yield row, (max_age, min_hits, score, iou) + (low if second.on else ())


def sweep_settings(grid):
    """Enumerate: (settings, plans).  One row per setting - the tracker's axes outermost, then the live passes in chain order, a
    pass's first axis outside its second - and {pass name: _Plan}."""
    plans = dict((p.name, _Plan(p, grid)) for p in (SECOND,) + PASSES)
    settings = []
    for row, _ in _tracked_points(grid, plans['second']):
        rows = [row]
        for p in PASSES:
            rows = [dict(row, **keys) for row in rows for _, keys in plans[p.name].points]
        settings += rows
    return settings, plans


def run_settings(packed, grid, plans, n_classes):
    """Run: the tracks of every setting, in the order of sweep_settings().  One tracker call per tracked point; the first pass of
    the chain fans its result out in one call; then every output goes through the other live passes ON ITS OWN, a pass taking all
    results so far times all of its jobs in one call - a stage's workspace grows with jobs x rows in the call."""
    first, others = PASSES[0], [p for p in PASSES[1:] if plans[p.name].on]
    tracks = []
    for _, (max_age, min_hits, score, iou, *low) in _tracked_points(grid, plans['second']):
        if low:
            out, _ = T.track_packed_byte(packed, [iou] * n_classes, max_age, min_hits, [score] * n_classes, [low[0]] * n_classes, [low[1]] * n_classes)
        else:
            out, _ = T.track_packed(packed, [iou] * n_classes, max_age, min_hits, [score] * n_classes)
        for out in first.run(packed, [out], plans[first.name].jobs, n_classes) if plans[first.name].on else [out]:
            results = [out]
            for p in others:
                results = p.run(packed, results, plans[p.name].jobs, n_classes)
            tracks += [tracks_from_packed(packed, result) for result in results]
    return tracks


def _class_columns(p, plan, row, settings, pick, n_classes):
    """The keys a live pass adds to a combined row: per axis one value per class, the pick's where the class is evaluated."""
    columns = {}
    for a, values in zip(p.axes, plan.values):
        column = list(row[a.rest]) if a.rest else [a.default[0] if a.switch else values[0]] * n_classes
        for c, k in pick.items():
            column[c - 1] = settings[k][a.row]
        columns[a.combined] = column
    columns.update(plan.singles)
    return columns


def rank_settings(settings, plans, scored, rank_by, group, n_classes):
    """Rank: pure host code.  scored: {metric name: one result per setting} of the live metrics; group: the settings of one
    (max_age, min_hits), which are consecutive.  Per group and level every evaluated class takes the setting that is best for it
    under the metric `rank_by` (METRICS: pick), ties going to grid order; the combined row lists the picks' parameters per class
    and every live metric over the picks' class rows, and the rows are ranked by rank_by's key, NaN last, ties in grid order.
    Returns (ranked {level: rows}, best {level: row or None})."""
    by = next(m for m in METRICS if m.name == rank_by)
    live = [m for m in METRICS if m.name in scored]
    classes = [c for c in ALL_CLASSES if c <= n_classes]
    ranked, best = {}, {}
    for lv in LEVELS:
        combos = []
        for g in range(0, len(settings), group):
            pick = dict((c, min(range(g, g + group), key=lambda k: by.pick(scored[by.name][k].table[c][lv]))) for c in classes)
            totals = dict((m.name, m.start()) for m in live)
            score_thr, iou_thr = [1.0] * n_classes, [1.0] * n_classes      # classes that are not evaluated are not tracked
            for c, k in pick.items():
                score_thr[c - 1], iou_thr[c - 1] = settings[k]['score'], settings[k]['iou']
                for m in live:
                    totals[m.name] = m.add(totals[m.name], scored[m.name][k].table[c][lv])
            row = {'max_age': settings[g]['max_age'], 'min_hits': settings[g]['min_hits'], 'score_threshold': score_thr, 'iou_threshold': iou_thr}
            row.update(live[0].finish(totals[live[0].name]))
            for p in _KEY_ORDER:
                if plans[p.name].on:
                    row.update(_class_columns(p, plans[p.name], row, settings, pick, n_classes))
            for m in live[1:]:
                row.update(m.finish(totals[m.name]))
            combos.append(row)
        order = sorted(range(len(combos)), key=lambda i: (-(combos[i][by.key] if combos[i][by.key] == combos[i][by.key] else -math.inf), i))
        ranked[lv] = [combos[i] for i in order]
        best[lv] = ranked[lv][0] if ranked[lv] else None
    return ranked, best


def _detections(path):
    """utils.read_data_file without the score filter: the tracker applies it per setting."""
    with open(path) as fp:
        raw = json.load(fp)
    if 'annotations' in raw:
        raw = raw['annotations']
    entries = {}
    for entry in raw:
        segment_id, frame_id, camera_id = _split(entry['image_id'])
        bucket = entries.setdefault(segment_id, {}).setdefault(camera_id, {}).setdefault(frame_id, [])
        bbox = entry['bbox']
        if bbox[2] < 1 or bbox[3] < 1:
            continue
        bucket.append({'bbox': bbox, 'score': entry['score'] if 'score' in entry else 1.0, 'category_id': entry['category_id']})
    return entries


def _chain_scores(packed, gt, grid, plans, live, iou_threshold, n_classes):
    """The MotResults of every setting through tracking/chain.py, in the order of sweep_settings(); ValueError for what it does not carry."""
    beyond = ['the %s pass (--%s-grid)' % (p.name, p.axes[0].key.replace('_', '-')) for p in PASSES if plans[p.name].on and p.name != 'refine']
    beyond += ['the %s metric (--%s)' % (m.name, m.option) for m in live if m.option is not None]
    if beyond:
        raise ValueError('the device chain carries the tracker, refinement and MOTA, not ' + ', '.join(beyond))
    chain = importlib.import_module('.chain', __package__).DeviceChain(packed, gt, n_classes, iou_threshold)
    return chain.run([args for _, args in _tracked_points(grid, plans['second'])], plans['refine'].jobs if plans['refine'].on else None)


def sweep(detections_path, gt, grid, iou_threshold=DEFAULT_IOU_THRESHOLD, n_classes=4, identity=False, rank_by='mota', hota=False, coverage=False,
          device_chain=False):
    """Track `detections_path` under every setting of `grid`, score all results in ONE call per metric and rank the settings.

    grid: lists 'score' and 'iou' (the tracker's thresholds, one grid point for all classes), 'max_age' and 'min_hits', and
    optionally the keys of SECOND and PASSES: per axis a list, per single parameter one value; the defaults switch a pass off, and
    its module is then not imported and the setting rows carry none of its keys.  The work is sweep_settings() (enumerate),
    run_settings() (run) and rank_settings() (rank); their docstrings and DESIGN.md section 15 have the order of the settings, the
    call structure and the ranking.  Classes are tracked and post-processed independently, so a class's counts depend only on its
    own parameters and on (max_age, min_hits), which the tracker shares: the grid is tracked with ONE point for all classes, and
    the best point is read off per class for each (max_age, min_hits); no product over classes is tracked.
    MOTA is always scored; identity / hota / coverage (and the rank_by that needs them: 'idf1', 'hota', 'mt') add their metric's
    keys to every ranked row (METRICS).  Ranking by anything but 'mota' is not the argmax of the ALL score over one shared grid
    point: per-class flags can only be tuned per class (DESIGN.md sections 18, 19 and 27).
    device_chain: run and score through tracking/chain.py - the rows of a result stay in HBM from the tracker to the count tables
    (DESIGN.md section 29).  The chain carries the tracker, its second association, refinement and MOTA; a grid that switches on
    another pass or metric is a ValueError that names it.  Settings, results, ranked and best equal the other route's.
    Returns {'settings': [...], 'results': [MotResult...], 'ranked': {level: [...]}, 'best': {level: {...}}} and, per further
    metric, its results under 'id_results', 'hota_results', 'coverage_results'."""
    if rank_by not in [m.name for m in METRICS]:
        raise ValueError("rank_by must be 'mota', 'idf1', 'hota' or 'mt'")
    if isinstance(gt, str):
        gt = load_ground_truth(gt)
    packed = T.pack_streams(_detections(detections_path))
    settings, plans = sweep_settings(grid)
    asked = {'identity': identity, 'hota': hota, 'coverage': coverage}
    live = [m for m in METRICS if m.option is None or asked[m.option] or rank_by == m.name]
    if device_chain:
        scored = {'mota': _chain_scores(packed, gt, grid, plans, live, iou_threshold, n_classes)}
    else:
        tracks = run_settings(packed, grid, plans, n_classes)
        packed_results = pack_results(gt, tracks, len(iou_threshold))       # once, for all metrics
        scored = dict((m.name, globals()[m.evaluate](gt, tracks, iou_threshold, packed=packed_results)) for m in live)
    group = len(grid['score']) * len(grid['iou']) * math.prod(len(plan.points) for plan in plans.values())
    ranked, best = rank_settings(settings, plans, scored, rank_by, group, n_classes)
    out = {'settings': settings, 'results': scored['mota'], 'ranked': ranked, 'best': best}
    out.update((m.results, scored[m.name]) for m in live[1:])
    return out


def flag_line(setting):
    """The tracking/track.py flags of a sweep result."""
    join = lambda v: ','.join(repr(float(x)) for x in v)
    line = '--score-threshold=%s --iou-threshold=%s --max-age=%d --min-hits=%d' % (
        join(setting['score_threshold']), join(setting['iou_threshold']), setting['max_age'], setting['min_hits'])
    for p in (SECOND,) + PASSES:
        if p.axes[0].combined not in setting:
            continue
        line += ''.join(' %s=%s' % (a.flag, a.join(setting[a.combined])) for a in p.axes)
        for s in p.singles:
            value = s.cast(setting.get(s.key, s.default))
            if s.always or value != s.default:
                line += ' %s=%s' % (s.flag, s.fmt % value)
    return line


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('tracks', nargs='*', help='tracking JSON files written by tracking/track.py')
    parser.add_argument('--annotations', required=True, help='ground-truth COCO json (waymo_to_coco.py)')
    parser.add_argument('--iou-threshold', type=_floats, default=list(DEFAULT_IOU_THRESHOLD), help='matching IoU per class')
    parser.add_argument('--json', help='write the tables (or the sweep) to this file')
    parser.add_argument('--sweep', help='detections JSON: track it under every grid setting and rank the settings')
    parser.add_argument('--score-grid', default='0.5:1.0:0.05')
    parser.add_argument('--iou-grid', default='0.0,0.01,0.1,0.3')
    parser.add_argument('--max-age', default='1,2,3')
    parser.add_argument('--min-hits', default='0,1')
    for p in _KEY_ORDER:
        for a in p.axes:
            parser.add_argument('--%s-grid' % a.key.replace('_', '-'), default=a.text, help=a.help)
        for s in p.singles:
            parser.add_argument(s.flag, default=s.default, help=s.help, **({'choices': s.choices} if s.choices else {'type': s.cast}))
    parser.add_argument('--top', type=int, default=10, help='ranked settings to print per level')
    parser.add_argument('--identity', action='store_true', help='also score identity preservation: IDF1 / IDP / IDR / IDTP / IDFP / IDFN')
    parser.add_argument('--hota', action='store_true', help='also score HOTA / DetA / AssA / LocA over the 19 localisation thresholds')
    parser.add_argument('--coverage', action='store_true', help='also score trajectory coverage: mostly tracked / partially tracked / mostly lost, fragmentations')
    parser.add_argument('--device-chain', action='store_true', help='sweep: keep the rows in HBM from the tracker to the count tables (tracker, refinement and MOTA only)')
    parser.add_argument('--rank-by', choices=tuple(m.name for m in METRICS), default='mota',
                        help='what the sweep ranks by (idf1 implies --identity, hota implies --hota, mt implies --coverage)')
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    gt = load_ground_truth(args.annotations)
    live = [m for m in METRICS if m.option is None or getattr(args, m.option) or (args.sweep and args.rank_by == m.name)]
    if args.sweep:
        grid = {'score': _grid_values(args.score_grid), 'iou': _grid_values(args.iou_grid),
                'max_age': _int_values(args.max_age), 'min_hits': _int_values(args.min_hits)}
        for p in (SECOND,) + PASSES:
            grid.update((a.key, a.parse(getattr(args, a.key + '_grid'))) for a in p.axes)
            grid.update((s.key, getattr(args, s.key)) for s in p.singles)
        res = sweep(args.sweep, gt, grid, args.iou_threshold, len(args.iou_threshold), rank_by=args.rank_by, device_chain=args.device_chain,
                    **dict((m.option, True) for m in live[1:]))
        for lv in LEVELS:
            print('LEVEL_%d: %d settings tracked, best per class combined for each (max_age, min_hits)' % (lv, len(res['settings'])))
            for r in res['ranked'][lv][:args.top]:
                print(''.join(m.line(r) for m in live) + '  ' + flag_line(r))
        if args.json:
            doc = {'settings': res['settings'], 'tables': [r.as_json() for r in res['results']],
                   'ranked': dict(('LEVEL_%d' % lv, v) for lv, v in res['ranked'].items())}
            for m in live[1:]:
                doc[m.tables] = [r.as_json() for r in res[m.results]]
                doc['rank_by'] = args.rank_by
            with open(args.json, 'wt') as fp:
                json.dump(doc, fp)
        if res['best'][2] is not None:
            print(flag_line(res['best'][2]))
        return 0
    if not args.tracks:
        raise SystemExit('give at least one tracking JSON, or --sweep DETECTIONS.json')
    tracks = [load_tracks(p) for p in args.tracks]
    scored = dict((m.name, globals()[m.evaluate](gt, tracks, args.iou_threshold)) for m in live)
    for k, path in enumerate(args.tracks):
        for m in _PRINT_ORDER:
            if m in live:
                print(m.table(scored[m.name][k], path))
    if args.json:
        doc = dict((p, r.as_json()) for p, r in zip(args.tracks, scored['mota']))
        for m in live[1:]:
            for p, r in zip(args.tracks, scored[m.name]):
                doc[p][m.section] = r.as_json()['table']
        with open(args.json, 'wt') as fp:
            json.dump(doc, fp)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
