"""AP / AR of detection results against ground truth on the GPU, and the sweep that tunes the ensemble's flags.

    python -m waymo_2d_tracking_amd.detnet.evaluate --annotations GT.json DETS.json [DETS2.json ...]
        [--metric waymo|voc] [--min-conf 0.01] [--json OUT]
    python -m waymo_2d_tracking_amd.detnet.evaluate --annotations GT.json --coco [--dt-images] DETS.json [DETS2.json ...]
    python -m waymo_2d_tracking_amd.detnet.evaluate --annotations GT.json --sweep A.json B.json ...
        --method soft_nms,nms --iou-grid 0.4:0.8:0.05 --cut-grid 0.9,1.0 --min-score-grid 0,0.01 [--weights 1,1] [--coco]

The metric is the one detnet/data/metric.py computes on one host thread (the reference's evaluation after inference), with
the order of equal confidences defined; DESIGN.md section 16 has the exact definition.  Every (result, image, class) is an
independent problem and one wavefront of the HIP kernels behind ``wt_det_eval_host`` (include/waymotrack.h): K results are
scored in one call, which is what makes a sweep over ensemble settings cost seconds.  No arithmetic of the metric runs on the
host; without the library or a GPU the calls fail.  --coco scores with the COCO metric instead (AP@[.5:.95] and the other eleven
numbers): another algorithm with its own kernels behind ``wt_det_coco_host``; `detnet/eval.py` is its
drop-in command line.
"""
import argparse
import ctypes as C
import json
import math

import numpy as np

from .. import _lib
from .data.metric import load_ground_truth

BUCKETS = ('', 'S', 'M', 'L')                       # the order of the last axis of every output
METRICS = {'waymo': lambda name: (0.7,) if name == 'vehicle' else (0.5,), 'voc': lambda name: (0.5, 0.75)}
DET_COLUMNS = ('conf', 'cx', 'cy', 'w', 'h')


# ---------------------------------------------------------------------------------------------------------------
# packing
def pack_ground_truth(annotations):
    """COCO-format dict / file -> the columns wt_det_eval_* takes: boxes as metric.load_ground_truth gives them (float32-rounded,
    normalised, duplicates removed) in ascending image-id order, with image_gt_offsets and image_area = width * height."""
    if isinstance(annotations, dict) and 'image_gt_offsets' in annotations:
        return annotations
    image_ids, sizes, gt, classnames = load_ground_truth(annotations)
    rows = [gt[k] for k in image_ids]
    allrows = np.concatenate(rows).reshape(-1, 5) if rows else np.zeros((0, 5))
    offsets = np.zeros(len(image_ids) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    col = lambda j: np.ascontiguousarray(allrows[:, j], dtype=np.float64)
    return dict(image_ids=image_ids, index={k: i for i, k in enumerate(image_ids)}, sizes=sizes, classnames=classnames,
                n_classes=len(classnames) - 1, x1=col(0), y1=col(1), x2=col(2), y2=col(3),
                label=np.ascontiguousarray(allrows[:, 4], dtype=np.int32), image_gt_offsets=offsets,
                image_area=np.asarray([float(sizes[k][0] * sizes[k][1]) for k in image_ids], np.float64))


def _class_labels(gt, classnames):
    """[(name, ground-truth label)] of the classes that are evaluated (metric.evaluate_detections skips unknown names)."""
    names = list(classnames)
    if names and names[0] == 'background':
        names = names[1:]
    known = gt['classnames']
    return names, [(i, n, known.index(n)) for i, n in enumerate(names) if n in known and known.index(n) > 0]


def _bad(message):
    return _lib.WaymoTrackError('wt_det_eval failed: WT_ERR_INVALID (%s)' % message)


def _wire_columns(gt, cols):
    """Wire rows (pixel [x, y, w, h], score) as columns -> normalised float64 rows, the inverse of load_prediction:
    conf = score, cx = (x + w / 2) / W, cy = (y + h / 2) / H, w = w / W, h = h / H, in that operation order."""
    to_gt = np.asarray([gt['index'].get(str(k), -1) for k in cols['image_ids']], np.int64).reshape(-1)
    image = to_gt[np.asarray(cols['image'], np.int64)]
    if (image < 0).any():
        k = cols['image_ids'][int(np.asarray(cols['image'])[np.argmax(image < 0)])]
        raise _bad('detection on image %s, which the ground truth does not list: its size is unknown' % k)
    cat = np.asarray(cols['category'], np.int64)
    if ((cat < 1) | (cat > gt['n_classes'])).any():
        i = int(np.argmax((cat < 1) | (cat > gt['n_classes'])))
        raise _bad('category_id %d outside 1..%d in image %s' % (cat[i], gt['n_classes'], gt['image_ids'][image[i]]))
    wh = np.asarray([gt['sizes'][k] for k in gt['image_ids']], np.float64).reshape(-1, 2)
    W, H = wh[image, 0], wh[image, 1]
    x, y, w, h = (np.asarray(cols[k], np.float64) for k in ('x', 'y', 'w', 'h'))
    out = dict(image=image, category=cat.astype(np.int32), conf=np.asarray(cols['score'], np.float64),
               cx=(x + w / 2) / W, cy=(y + h / 2) / H, w=w / W, h=h / H, source_row=np.arange(len(image), dtype=np.int64))
    classes = [(n, i) for i, n in enumerate(gt['classnames']) if i > 0]
    return out, classes


def _set_columns(gt, s):
    """One result in any accepted form -> (columns with `image` = ground-truth image index, [(class name, label)])."""
    if isinstance(s, dict) and 'image_ids' in s and 'score' in s:              # wire rows as columns (ensemble.read_submission)
        return _wire_columns(gt, s)
    if isinstance(s, (str, bytes)) or hasattr(s, '__fspath__'):                # a detection JSON on disk
        from .ensemble import read_submission
        return _wire_columns(gt, read_submission(s))
    if isinstance(s, (list, tuple)):                                           # parsed wire rows
        from .ensemble import submission_columns
        return _wire_columns(gt, submission_columns(list(s)))
    if hasattr(s, 'classnames') and hasattr(s, 'shard_columns'):               # Predictions store
        names, classes = _class_labels(gt, s.classnames or gt['classnames'][1:])
        cols, tested = s.shard_columns()
        to_gt = np.asarray([gt['index'].get(str(k), -1) if tested[i] else -1 for i, k in enumerate(s.image_ids)] + [-1], np.int64)
        label_of = np.zeros(len(names) + 1, np.int64)
        for i, _, label in classes:
            label_of[i] = label
        if len(cols['cls']) and (cols['cls'].min() < 0 or cols['cls'].max() >= len(names)):
            bad = int(np.argmax((cols['cls'] < 0) | (cols['cls'] >= len(names))))
            raise _bad('class index %d outside the %d class names in image %s' % (cols['cls'][bad], len(names), s.image_ids[cols['image'][bad]]))
        image, label = to_gt[cols['image']], label_of[cols['cls']]
        keep = np.nonzero((image >= 0) & (label > 0))[0]
        out = dict(image=image[keep], category=label[keep].astype(np.int32), cls=cols['cls'][keep], source_row=keep.astype(np.int64),
                   conf=cols['score'][keep].astype(np.float64), cx=cols['cx'][keep].astype(np.float64), cy=cols['cy'][keep].astype(np.float64),
                   w=cols['w'][keep].astype(np.float64), h=cols['h'][keep].astype(np.float64))
        return out, [(n, label) for _, n, label in classes]
    if isinstance(s, dict):                                                    # {image_id: [per class (n, 5)]}
        names, classes = _class_labels(gt, gt['classnames'][1:])
        parts = {k: [] for k in ('image', 'category', 'cls') + DET_COLUMNS}
        for image_id, per_class in s.items():
            i = gt['index'].get(str(image_id))
            if i is None or per_class is None:
                continue
            if len(per_class) != len(names):
                raise _bad('image %s has %d class arrays, the ground truth has %d classes' % (image_id, len(per_class), len(names)))
            for ci, _, label in classes:
                a = np.asarray(per_class[ci], np.float64)
                if a.size % 5:
                    raise _bad('image %s, class %s: rows are [conf, cx, cy, w, h], got an array of shape %s' % (image_id, names[ci], a.shape))
                a = a.reshape(-1, 5)
                parts['image'].append(np.full(len(a), i, np.int64)); parts['category'].append(np.full(len(a), label, np.int32))
                parts['cls'].append(np.full(len(a), ci, np.int32))
                for j, k in enumerate(DET_COLUMNS):
                    parts[k].append(a[:, j])
        out = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in parts.items()}
        out['image'] = out['image'].astype(np.int64); out['category'] = out['category'].astype(np.int32); out['cls'] = out['cls'].astype(np.int32)
        out['source_row'] = np.arange(len(out['image']), dtype=np.int64)
        return out, [(n, label) for _, n, label in classes]
    raise TypeError('a result is a Predictions store, a {image_id: [per class (n, 5)]} dict, or a detection JSON (path or rows)')


def pack_detections(gt, sets):
    """K results -> the concatenated columns and offsets wt_det_eval_* takes: per set the rows in image order; inside an image the
    wire form keeps file order, the dict and Predictions forms go class by class in stored order."""
    gt = pack_ground_truth(gt)
    if len(sets) < 1:
        raise ValueError('at least one result is needed')
    n_images = len(gt['image_ids'])
    cols = {k: [] for k in ('category', 'source_row') + DET_COLUMNS}
    set_rows, offsets, classes = [0], [], []
    for s in sets:
        c, cls = _set_columns(gt, s)
        key = c['image'] * (int(c['cls'].max()) + 1 if len(c['cls']) else 1) + c['cls'] if 'cls' in c else c['image']
        order = np.argsort(key, kind='stable')
        offsets.append(np.searchsorted(c['image'][order], np.arange(n_images + 1)).astype(np.int64))
        for k in cols:
            cols[k].append(c[k][order])
        set_rows.append(set_rows[-1] + len(order))
        classes.append(cls)
    out = {k: np.ascontiguousarray(np.concatenate(cols[k]), dtype=np.float64) for k in DET_COLUMNS}
    out['category'] = np.ascontiguousarray(np.concatenate(cols['category']), dtype=np.int32)
    out['source_row'] = np.concatenate(cols['source_row']).astype(np.int64)
    out['set_row_offsets'] = np.asarray(set_rows, np.int64)
    out['image_det_offsets'] = np.ascontiguousarray(np.stack(offsets), dtype=np.int64)
    out['classes'] = classes
    return out


def thresholds(gt, metric):
    """(n_classes, n_thr) IoU thresholds of a preset, row c - 1 for label c."""
    if metric not in METRICS:
        raise ValueError("metric is 'waymo' or 'voc', got %r" % (metric,))
    rows = [METRICS[metric](name) for name in gt['classnames'][1:]]
    return np.ascontiguousarray(rows, dtype=np.float64).reshape(gt['n_classes'], -1)


# ---------------------------------------------------------------------------------------------------------------
# results
class DetResult(object):
    """Scores of one detection result.

    ap, ar (n_classes, n_thr, 4) float64 and npos, tp, fp (n_classes, n_thr, 4) int64; last axis = BUCKETS ('', S, M, L)
    classes   [(name, label)] of the evaluated classes, in the result's class order
    with per_row=True, per packed row of the set (source_row = its row in the input): tp_flag (n, n_thr) uint8 (2 = took no part),
    match_gt (index into the packed ground truth, -1 none), and per label c: order[c] (packed rows by descending confidence) with
    ctp[c], cfp[c] (len(order[c]), n_thr) the cumulative counts of the all-sizes bucket along it."""

    def __init__(self, metric, thr, classes, ap, ar, npos, tp, fp, per_row=None):
        self.metric, self.thr, self.classes = metric, thr, classes
        self.ap, self.ar, self.npos, self.tp, self.fp = ap, ar, npos, tp, fp
        for k, v in (per_row or {}).items():
            setattr(self, k, v)

    def summary(self):
        """The dict metric.evaluate_detections returns for this metric (same keys, same nesting)."""
        out = {}
        for name, c in self.classes:
            ap, ar = self.ap[c - 1], self.ar[c - 1]
            if self.metric == 'waymo':
                out[name] = dict(ap=float(ap[0, 0]), ar=float(ar[0, 0]), T=int(self.npos[c - 1, 0, 0]), score=float(ap[0, 0]),
                                 by_size={b: float(ap[0, i]) for i, b in enumerate(BUCKETS) if b})
            else:
                s = {}
                for t, tv in enumerate(self.thr[c - 1].tolist()):
                    for b in (('S', 'M', 'L', '') if tv == 0.5 else ('',)):
                        s['ap@%s%s' % (tv, b)] = float(ap[t, BUCKETS.index(b)])
                        s['ar@%s%s' % (tv, b)] = float(ar[t, BUCKETS.index(b)])
                s['T'] = int(self.npos[c - 1, 0, 0])
                s['score'] = s.get('ap@0.5')
                out[name] = s
        if self.metric == 'voc':
            mean = {k: float(np.mean([out[name][k] for name, _ in self.classes])) for k in ('ap@0.5', 'ar@0.5', 'T')}
            out['mean'] = mean
            out['score'] = mean['ap@0.5']
        return out

    def mean_ap(self):
        """Mean AP (first threshold, all sizes) over the classes that have ground truth: the figure evaluate_detections prints."""
        aps = [self.ap[c - 1, 0, 0] for _, c in self.classes if self.npos[c - 1, 0, 0] > 0]
        return float(np.mean(aps)) if aps else math.nan

    def lines(self):
        """The lines metric.evaluate_detections prints."""
        s = self.summary()
        out = ['%-12s ' % name + ' '.join('%s %.4f' % (k, x) for k, x in s[name].items() if isinstance(x, (int, float)))
               for name, _ in self.classes]
        out.append('* mean AP over classes with ground truth = %.4f' % self.mean_ap())
        return out


def _results(gt, p, metric, thr, out, per_row):
    results = []
    T = thr.shape[1]
    for k, classes in enumerate(p['classes']):
        rows = None
        if per_row:
            lo, hi = int(p['set_row_offsets'][k]), int(p['set_row_offsets'][k + 1])
            co = out['class_offsets'][k]
            rows = dict(source_row=p['source_row'][lo:hi], tp_flag=out['tp_flag'][lo:hi], match_gt=out['match_gt'][lo:hi],
                        order={}, ctp={}, cfp={})
            for c in range(1, gt['n_classes'] + 1):
                a, b = int(co[c - 1]), int(co[c])
                rows['order'][c] = out['order'][a:b] - lo
                rows['ctp'][c] = out['ctp'][a:b].reshape(-1, T)
                rows['cfp'][c] = out['cfp'][a:b].reshape(-1, T)
        results.append(DetResult(metric, thr, classes, out['ap'][k], out['ar'][k], out['npos'][k], out['tp'][k], out['fp'][k], rows))
    return results


def _min_conf(min_conf, K):
    m = np.ascontiguousarray(np.broadcast_to(np.asarray(min_conf, np.float64), (K,)) if np.ndim(min_conf) == 0 else min_conf, dtype=np.float64)
    if m.shape != (K,):
        raise ValueError('%d min_conf values for %d results' % (m.size, K))
    return m


def evaluate_detection_sets(gt, sets, metric='waymo', min_conf=0.01, per_row=False):
    """Score K detection results against one ground truth (annotations, or pack_ground_truth's output) in ONE wt_det_eval_host
    call.  min_conf: one value or one per result.  Returns a list of K DetResult."""
    lib = _lib.lib()
    gt = pack_ground_truth(gt)
    p = sets if isinstance(sets, dict) and 'set_row_offsets' in sets else pack_detections(gt, sets)
    K = len(p['set_row_offsets']) - 1
    thr = thresholds(gt, metric)
    nc, T = thr.shape
    minc = _min_conf(min_conf, K)
    n_det = int(p['set_row_offsets'][-1])
    shape = (K, nc, T, len(BUCKETS))
    out = dict(ap=np.zeros(shape), ar=np.zeros(shape), npos=np.zeros(shape, np.int64), tp=np.zeros(shape, np.int64), fp=np.zeros(shape, np.int64))
    if per_row:
        out.update(tp_flag=np.full((n_det, T), 2, np.uint8), match_gt=np.full(n_det, -1, np.int64), order=np.zeros(n_det, np.int64),
                   class_offsets=np.zeros((K, nc + 1), np.int64), ctp=np.zeros((n_det, T), np.int64), cfp=np.zeros((n_det, T), np.int64))
    opt = lambda k: _lib.ptr(out[k]) if per_row else None
    rc = lib.wt_det_eval_host(
        C.c_int64(gt['x1'].size), _lib.ptr(gt['x1']), _lib.ptr(gt['y1']), _lib.ptr(gt['x2']), _lib.ptr(gt['y2']), _lib.ptr(gt['label']),
        C.c_int64(len(gt['image_ids'])), _lib.ptr(gt['image_gt_offsets']), _lib.ptr(gt['image_area']),
        C.c_int32(K), _lib.ptr(p['set_row_offsets']), _lib.ptr(p['image_det_offsets']),
        _lib.ptr(p['conf']), _lib.ptr(p['cx']), _lib.ptr(p['cy']), _lib.ptr(p['w']), _lib.ptr(p['h']), _lib.ptr(p['category']),
        _lib.ptr(minc), C.c_int32(nc), C.c_int32(T), _lib.ptr(thr),
        _lib.ptr(out['ap']), _lib.ptr(out['ar']), _lib.ptr(out['npos']), _lib.ptr(out['tp']), _lib.ptr(out['fp']),
        opt('tp_flag'), opt('match_gt'), opt('order'), opt('class_offsets'), opt('ctp'), opt('cfp'))
    _lib.check(rc, 'wt_det_eval_host')
    return _results(gt, p, metric, thr, out, per_row)


class DeviceDetEvaluation(object):
    """The same evaluation with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues one
    wt_det_eval_dev on the current torch stream and returns at once, ``results()`` synchronises and reads the outputs back.
    This is the form a device-resident sweep (merged rows scored without leaving the GPU) builds on."""

    def __init__(self, gt, sets, metric='waymo', min_conf=0.01):
        import torch
        self.torch = torch
        self.lib = _lib.lib()
        self.gt = gt = pack_ground_truth(gt)
        self.p = p = sets if isinstance(sets, dict) and 'set_row_offsets' in sets else pack_detections(gt, sets)
        self.metric = metric
        self.thr = thresholds(gt, metric)
        self.K = len(p['set_row_offsets']) - 1
        self.minc = _min_conf(min_conf, self.K)
        self.n_det = int(p['set_row_offsets'][-1])
        self.n_images = len(gt['image_ids'])
        nc, T = self.thr.shape
        dev = torch.device('cuda', torch.cuda.current_device())
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype, device=dev)
        self.g = {n: up(gt[n]) for n in ('x1', 'y1', 'x2', 'y2', 'label', 'image_gt_offsets', 'image_area')}
        self.d = {n: up(p[n]) for n in DET_COLUMNS + ('category', 'set_row_offsets', 'image_det_offsets')}
        shape = (self.K, nc, T, len(BUCKETS))
        z = lambda s, dt: torch.zeros(s, dtype=dt, device=dev)
        n = max(1, self.n_det)
        self.out = dict(ap=z(shape, torch.float64), ar=z(shape, torch.float64), npos=z(shape, torch.int64), tp=z(shape, torch.int64),
                        fp=z(shape, torch.int64), tp_flag=z((n, T), torch.uint8), match_gt=z(n, torch.int64), order=z(n, torch.int64),
                        class_offsets=z((self.K, nc + 1), torch.int64), ctp=z((n, T), torch.int64), cfp=z((n, T), torch.int64))
        self.status = z(1, torch.int32)
        self.ws_bytes = int(self.lib.wt_det_eval_workspace(C.c_int32(self.K), C.c_int64(self.n_images), C.c_int32(nc), C.c_int32(T),
                                                           C.c_int64(gt['x1'].size), C.c_int64(self.n_det)))
        if not self.ws_bytes:
            _lib.check(4, 'wt_det_eval_workspace')
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)

    def launch(self):
        g, d, o, v = self.g, self.d, self.out, C.c_void_p
        p = lambda t: v(t.data_ptr())
        nc, T = self.thr.shape
        rc = self.lib.wt_det_eval_dev(
            C.c_int64(self.gt['x1'].size), p(g['x1']), p(g['y1']), p(g['x2']), p(g['y2']), p(g['label']),
            C.c_int64(self.n_images), p(g['image_gt_offsets']), p(g['image_area']),
            C.c_int32(self.K), C.c_int64(self.n_det), p(d['set_row_offsets']), p(d['image_det_offsets']),
            p(d['conf']), p(d['cx']), p(d['cy']), p(d['w']), p(d['h']), p(d['category']),
            _lib.ptr(self.minc), C.c_int32(nc), C.c_int32(T), _lib.ptr(self.thr),
            p(o['ap']), p(o['ar']), p(o['npos']), p(o['tp']), p(o['fp']),
            p(o['tp_flag']), p(o['match_gt']), p(o['order']), p(o['class_offsets']), p(o['ctp']), p(o['cfp']),
            p(self.status), p(self.ws), C.c_size_t(self.ws_bytes), v(self.torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, 'wt_det_eval_dev')

    def results(self, per_row=False):
        self.torch.cuda.current_stream().synchronize()
        st = int(self.status.item())
        if st:
            raise _lib.WaymoTrackError('wt_det_eval_dev failed: %s (status reported by the kernel)' % _lib._STATUS.get(st, st))
        out = {k: t.cpu().numpy() for k, t in self.out.items()}
        for k in ('tp_flag', 'match_gt', 'order', 'ctp', 'cfp'):
            out[k] = out[k][:self.n_det]
        return _results(self.gt, self.p, self.metric, self.thr, out, per_row)


# ---------------------------------------------------------------------------------------------------------------
# the COCO metric: its own packers, wt_det_coco_*; thresholds() above has no 'coco' preset on purpose
COCO_THR = np.linspace(.5, .95, 10)
COCO_REC = np.linspace(0, 1, 101)
COCO_AREAS = np.asarray([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64)
COCO_AREA_NAMES = ('all', 'small', 'medium', 'large')
COCO_MAX_DETS = np.asarray([1, 10, 100], np.int32)
COCO_STATS = ('mAP', 'AP50', 'AP75', 'mAPs', 'mAPm', 'mAPl', 'AR1', 'AR10', 'AR', 'ARs', 'ARm', 'ARl')
COCO_DET_COLUMNS = ('score', 'x', 'y', 'w', 'h')


def _bad_coco(message):
    return _lib.WaymoTrackError('wt_det_coco failed: WT_ERR_INVALID (%s)' % message)


def pack_coco_ground_truth(annotations):
    """COCO-format dict / file -> the columns wt_det_coco_* takes.  Every annotation counts: pixel [x, y, w, h] as float64 exactly
    as parsed, area = the field or w * h, iscrowd (or ignore) default 0; images in ascending sorted() order of their id,
    annotation order inside an image; cat = index into the ascending category ids."""
    if isinstance(annotations, dict) and 'image_gt_offsets' in annotations and 'cat_ids' in annotations:
        return annotations
    if not isinstance(annotations, dict):
        with open(annotations) as fp:
            annotations = json.load(fp)
    images = list(annotations['images'])
    image_ids = sorted(im['id'] for im in images)
    index = {str(k): i for i, k in enumerate(image_ids)}
    sizes = {str(im['id']): (im.get('width'), im.get('height')) for im in images}
    cats = sorted(annotations['categories'], key=lambda c: c['id'])
    cat_ids = [c['id'] for c in cats]
    cat_index = {c: i for i, c in enumerate(cat_ids)}
    anns = annotations.get('annotations', [])
    n = len(anns)
    image = np.zeros(n, np.int64)
    cat = np.zeros(n, np.int32)
    crowd = np.zeros(n, np.uint8)
    box = np.zeros((n, 4), np.float64)
    area = np.zeros(n, np.float64)
    for j, a in enumerate(anns):
        i = index.get(str(a['image_id']))
        if i is None:
            raise _bad_coco('annotation %d is on image %s, which the ground truth does not list' % (j, a['image_id']))
        if a['category_id'] not in cat_index:
            raise _bad_coco('annotation %d has category_id %s, which the ground truth does not define' % (j, a['category_id']))
        image[j], cat[j] = i, cat_index[a['category_id']]
        box[j] = [float(v) for v in a['bbox']]
        area[j] = float(a['area']) if 'area' in a else box[j, 2] * box[j, 3]
        crowd[j] = 1 if a.get('iscrowd', 0) else 0                             # an 'ignore' field is replaced by iscrowd, as the package does
    order = np.argsort(image, kind='stable')
    col = lambda v, dt: np.ascontiguousarray(v[order], dtype=dt)
    return dict(image_ids=image_ids, index=index, sizes=sizes, cat_ids=cat_ids, names=[c.get('name', str(c['id'])) for c in cats],
                n_cats=len(cat_ids), x=col(box[:, 0], np.float64), y=col(box[:, 1], np.float64), w=col(box[:, 2], np.float64),
                h=col(box[:, 3], np.float64), area=col(area, np.float64), cat=col(cat, np.int32), crowd=col(crowd, np.uint8),
                image_gt_offsets=np.searchsorted(image[order], np.arange(len(image_ids) + 1)).astype(np.int64))


def _coco_wire(gt, cols):
    """Wire rows as columns (ensemble.read_submission) -> (image index, category index or -1, score, x, y, w, h)."""
    to_gt = np.asarray([gt['index'].get(str(k), -1) for k in cols['image_ids']], np.int64).reshape(-1)
    image = to_gt[np.asarray(cols['image'], np.int64)]
    if (image < 0).any():
        i = int(np.argmax(image < 0))
        raise _bad_coco('row %d is on image %s, which the ground truth does not list' % (i, cols['image_ids'][int(np.asarray(cols['image'])[i])]))
    lut = {c: i for i, c in enumerate(gt['cat_ids'])}
    cat = np.asarray([lut.get(int(c), -1) for c in np.asarray(cols['category']).tolist()], np.int32)
    return dict(image=image, cat=cat, score=np.asarray(cols['score'], np.float64), x=np.asarray(cols['x'], np.float64), y=np.asarray(cols['y'], np.float64),
                w=np.asarray(cols['w'], np.float64), h=np.asarray(cols['h'], np.float64))


def _coco_normalised(gt, image, cat, conf, cx, cy, w, h):
    """Normalised [conf, cx, cy, w, h] rows -> pixel rows: x = (cx - w / 2) * W, y = (cy - h / 2) * H, w = w * W, h = h * H."""
    wh = np.asarray([gt['sizes'][str(k)] for k in gt['image_ids']], np.float64).reshape(-1, 2)
    W, H = wh[image, 0], wh[image, 1]
    cx, cy, w, h = (np.asarray(v, np.float64) for v in (cx, cy, w, h))
    return dict(image=np.asarray(image, np.int64), cat=np.asarray(cat, np.int32), score=np.asarray(conf, np.float64),
                x=(cx - w / 2) * W, y=(cy - h / 2) * H, w=w * W, h=h * H)


def _coco_set_columns(gt, s):
    if isinstance(s, dict) and 'image_ids' in s and 'score' in s:
        return _coco_wire(gt, s)
    if isinstance(s, (str, bytes)) or hasattr(s, '__fspath__'):
        from .ensemble import read_submission
        return _coco_wire(gt, read_submission(s))
    if isinstance(s, (list, tuple)):
        from .ensemble import submission_columns
        return _coco_wire(gt, submission_columns(list(s)))
    name_index = {n: i for i, n in enumerate(gt['names'])}
    if hasattr(s, 'classnames') and hasattr(s, 'shard_columns'):               # Predictions store
        names = list(s.classnames or gt['names'])
        if names and names[0] == 'background':
            names = names[1:]
        cols, tested = s.shard_columns()
        to_gt = np.asarray([gt['index'].get(str(k), -1) if tested[i] else -1 for i, k in enumerate(s.image_ids)] + [-1], np.int64)
        cat_of = np.asarray([name_index.get(n, -1) for n in names] + [-1], np.int64)
        image = to_gt[cols['image']]
        keep = np.nonzero(image >= 0)[0]
        return _coco_normalised(gt, image[keep], cat_of[cols['cls'][keep]], cols['score'][keep], cols['cx'][keep], cols['cy'][keep], cols['w'][keep], cols['h'][keep])
    if isinstance(s, dict):                                                    # {image_id: [per class (n, 5)]}
        parts = []
        for image_id, per_class in s.items():
            i = gt['index'].get(str(image_id))
            if i is None:
                raise _bad_coco('a detection is on image %s, which the ground truth does not list' % (image_id,))
            if per_class is None:
                continue
            if len(per_class) != gt['n_cats']:
                raise _bad_coco('image %s has %d class arrays, the ground truth has %d categories' % (image_id, len(per_class), gt['n_cats']))
            for ci, rows in enumerate(per_class):
                a = np.asarray(rows, np.float64)
                if a.size % 5:
                    raise _bad_coco('image %s, class %s: rows are [conf, cx, cy, w, h], got an array of shape %s' % (image_id, gt['names'][ci], a.shape))
                a = a.reshape(-1, 5)
                parts.append(np.concatenate([np.full((len(a), 1), i, np.float64), np.full((len(a), 1), ci, np.float64), a], axis=1))
        a = np.concatenate(parts) if parts else np.zeros((0, 7))
        return _coco_normalised(gt, a[:, 0].astype(np.int64), a[:, 1].astype(np.int32), a[:, 2], a[:, 3], a[:, 4], a[:, 5], a[:, 6])
    raise TypeError('a result is a Predictions store, a {image_id: [per class (n, 5)]} dict, or a detection JSON (path or rows)')


def pack_coco_detections(gt, sets):
    """K results -> the concatenated columns and offsets wt_det_coco_* takes: per set the rows in image order, input order inside
    an image.  Rows of a category the ground truth does not define are left out (source_row = a kept row's index in the input);
    has_rows (K, n_images) uint8 = the image has a row of any category: the images of --dt-images."""
    gt = pack_coco_ground_truth(gt)
    if len(sets) < 1:
        raise ValueError('at least one result is needed')
    n_images = len(gt['image_ids'])
    cols = {k: [] for k in ('cat', 'source_row') + COCO_DET_COLUMNS}
    set_rows, offsets, has_rows = [0], [], []
    for k, s in enumerate(sets):
        c = _coco_set_columns(gt, s)
        vals = np.stack([c[n] for n in COCO_DET_COLUMNS], axis=1) if len(c['score']) else np.zeros((0, 5))
        if not np.isfinite(vals).all():
            raise _bad_coco('result %d, row %d: the score or a coordinate is not finite' % (k, int(np.argmax(~np.isfinite(vals).all(axis=1)))))
        has = np.zeros(n_images, np.uint8)
        has[c['image']] = 1
        keep = np.nonzero(c['cat'] >= 0)[0]
        order = keep[np.argsort(c['image'][keep], kind='stable')]
        offsets.append(np.searchsorted(c['image'][order], np.arange(n_images + 1)).astype(np.int64))
        for n in COCO_DET_COLUMNS + ('cat',):
            cols[n].append(c[n][order])
        cols['source_row'].append(order.astype(np.int64))
        set_rows.append(set_rows[-1] + len(order))
        has_rows.append(has)
    out = {n: np.ascontiguousarray(np.concatenate(cols[n]), dtype=np.float64) for n in COCO_DET_COLUMNS}
    out['cat'] = np.ascontiguousarray(np.concatenate(cols['cat']), dtype=np.int32)
    out['source_row'] = np.concatenate(cols['source_row']).astype(np.int64)
    out['set_row_offsets'] = np.asarray(set_rows, np.int64)
    out['image_det_offsets'] = np.ascontiguousarray(np.stack(offsets), dtype=np.int64)
    out['has_rows'] = np.ascontiguousarray(np.stack(has_rows), dtype=np.uint8)
    return out


def coco_stats(precision, recall, thr=COCO_THR):
    """precision (T, R, C, A, M), recall (T, C, A, M) of one result -> the twelve numbers in COCO_STATS order: each the mean of the
    selected entries > -1, or -1 without any.  Host numpy on purpose: the tables are the kernels' output, this is their summary."""
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    t50, t75 = int(np.argmin(np.abs(thr - .5))), int(np.argmin(np.abs(thr - .75)))
    M = precision.shape[-1] - 1
    return np.asarray([mean(precision[:, :, :, 0, M]), mean(precision[t50, :, :, 0, M]), mean(precision[t75, :, :, 0, M]),
                       mean(precision[:, :, :, 1, M]), mean(precision[:, :, :, 2, M]), mean(precision[:, :, :, 3, M]),
                       mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, 1]), mean(recall[:, :, 0, M]),
                       mean(recall[:, :, 1, M]), mean(recall[:, :, 2, M]), mean(recall[:, :, 3, M])])


class CocoResult(object):
    """COCO scores of one detection result.

    precision (10, 101, n_cats, 4, 3), recall (10, n_cats, 4, 3) float64, -1 = no not-ignored ground truth; npig (n_cats, 4) int64
    stats     the twelve numbers, COCO_STATS order
    with per_row=True, per packed row (source_row = its row in the input): rank (-1 = beyond 100), match_gt (n, 4, 10) packed
    ground-truth row or -1, ignore (n, 4, 10) uint8."""

    def __init__(self, gt, precision, recall, npig, per_row=None, cat_ids=None):
        self.cat_ids, self.names = gt['cat_ids'], gt['names']
        self.counts = np.bincount(gt['cat'], minlength=gt['n_cats'])
        self.precision, self.recall, self.npig = precision, recall, npig
        self.selected = [i for i, c in enumerate(self.cat_ids) if cat_ids is None or c in cat_ids]
        self.stats = coco_stats(precision[:, :, self.selected], recall[:, self.selected])
        for k, v in (per_row or {}).items():
            setattr(self, k, v)

    def per_category(self):
        """[(category id, name, T = its annotation count, the twelve numbers)] of the selected categories, in id order."""
        return [(self.cat_ids[i], self.names[i], int(self.counts[i]), coco_stats(self.precision[:, :, i:i + 1], self.recall[:, i:i + 1]))
                for i in self.selected]

    def lines(self):
        """The twelve summary lines in the well-known layout."""
        out = []
        spec = [(1, None, 'all', 100), (1, .5, 'all', 100), (1, .75, 'all', 100), (1, None, 'small', 100), (1, None, 'medium', 100), (1, None, 'large', 100),
                (0, None, 'all', 1), (0, None, 'all', 10), (0, None, 'all', 100), (0, None, 'small', 100), (0, None, 'medium', 100), (0, None, 'large', 100)]
        for (ap, iou, area, md), v in zip(spec, self.stats):
            out.append(' %-18s %s @[ IoU=%-9s | area=%6s | maxDets=%3d ] = %0.3f' % (
                'Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', '0.50:0.95' if iou is None else '%0.2f' % iou, area, md, v))
        return out

    def table(self):
        """Plain-text rows of the categories that have any value >= 0, best mAP first: the twelve numbers, T, the name."""
        rows = [r for r in self.per_category() if (r[3] >= 0).any()]
        rows.sort(key=lambda r: -r[3][0])
        out = [' '.join('%6s' % n for n in COCO_STATS) + ' %8s  %s' % ('T', 'name')]
        for _, name, count, stats in rows:
            out.append(' '.join('%6.3f' % v for v in stats) + ' %8d  %s' % (count, name))
        return out


def _coco_call_host(gt, p, mask, per_row):
    """One wt_det_coco_host call -> dict of tables (and per-row arrays)."""
    lib = _lib.lib()
    K = len(p['set_row_offsets']) - 1
    T, R, A, M, nc = len(COCO_THR), len(COCO_REC), len(COCO_AREAS), len(COCO_MAX_DETS), gt['n_cats']
    n_det = int(p['set_row_offsets'][-1])
    out = dict(precision=np.zeros((K, T, R, nc, A, M)), recall=np.zeros((K, T, nc, A, M)), npig=np.zeros((K, nc, A), np.int64))
    if per_row:
        out.update(rank=np.full(n_det, -1, np.int32), match_gt=np.full((n_det, A, T), -1, np.int64), ignore=np.zeros((n_det, A, T), np.uint8))
    opt = lambda k: _lib.ptr(out[k]) if per_row else None
    thr, rec, areas, md = (np.ascontiguousarray(v) for v in (COCO_THR, COCO_REC, COCO_AREAS, COCO_MAX_DETS))
    rc = lib.wt_det_coco_host(
        C.c_int64(gt['x'].size), _lib.ptr(gt['x']), _lib.ptr(gt['y']), _lib.ptr(gt['w']), _lib.ptr(gt['h']), _lib.ptr(gt['area']),
        _lib.ptr(gt['cat']), _lib.ptr(gt['crowd']), C.c_int64(len(gt['image_ids'])), _lib.ptr(gt['image_gt_offsets']),
        C.c_int32(K), _lib.ptr(p['set_row_offsets']), _lib.ptr(p['image_det_offsets']),
        _lib.ptr(p['score']), _lib.ptr(p['x']), _lib.ptr(p['y']), _lib.ptr(p['w']), _lib.ptr(p['h']), _lib.ptr(p['cat']),
        _lib.ptr(mask) if mask is not None else None, C.c_int32(nc), C.c_int32(T), _lib.ptr(thr), C.c_int32(R), _lib.ptr(rec),
        C.c_int32(A), _lib.ptr(areas), C.c_int32(M), _lib.ptr(md),
        _lib.ptr(out['precision']), _lib.ptr(out['recall']), _lib.ptr(out['npig']), opt('rank'), opt('match_gt'), opt('ignore'))
    _lib.check(rc, 'wt_det_coco_host')
    return out


def _coco_results(gt, p, out, per_row, cat_ids):
    results = []
    for k in range(len(p['set_row_offsets']) - 1):
        rows = None
        if per_row:
            lo, hi = int(p['set_row_offsets'][k]), int(p['set_row_offsets'][k + 1])
            rows = dict(source_row=p['source_row'][lo:hi], rank=out['rank'][lo:hi], match_gt=out['match_gt'][lo:hi], ignore=out['ignore'][lo:hi])
        results.append(CocoResult(gt, out['precision'][k], out['recall'][k], out['npig'][k], rows, cat_ids))
    return results


def evaluate_coco_sets(gt, sets, dt_images=False, per_row=False, cat_ids=None, call=None):
    """Score K detection results against one ground truth (annotations, or pack_coco_ground_truth's output) with the COCO metric
    in ONE wt_det_coco_host call.  dt_images: per result only the images with at least one row take part.  cat_ids restricts
    the summary numbers (not the tables).  call(gt, packed, mask, per_row) -> tables replaces the HIP call (tests: the
    restatement).  Returns a list of K CocoResult."""
    gt = pack_coco_ground_truth(gt)
    p = sets if isinstance(sets, dict) and 'set_row_offsets' in sets else pack_coco_detections(gt, sets)
    mask = p['has_rows'] if dt_images else None
    out = (call or _coco_call_host)(gt, p, mask, per_row)
    return _coco_results(gt, p, out, per_row, cat_ids)


class DeviceCocoEvaluation(object):
    """The COCO evaluation with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues one
    wt_det_coco_dev on the current torch stream and returns at once, ``results()`` synchronises and reads the outputs back."""

    def __init__(self, gt, sets, dt_images=False, per_row=True):
        import torch
        self.torch = torch
        self.lib = _lib.lib()
        self.gt = gt = pack_coco_ground_truth(gt)
        self.p = p = sets if isinstance(sets, dict) and 'set_row_offsets' in sets else pack_coco_detections(gt, sets)
        self.K = len(p['set_row_offsets']) - 1
        self.n_det = int(p['set_row_offsets'][-1])
        self.n_images = len(gt['image_ids'])
        self.per_row = per_row
        self.host = [np.ascontiguousarray(v) for v in (COCO_THR, COCO_REC, COCO_AREAS, COCO_MAX_DETS)]
        T, R, A, M, nc = len(COCO_THR), len(COCO_REC), len(COCO_AREAS), len(COCO_MAX_DETS), gt['n_cats']
        dev = torch.device('cuda', torch.cuda.current_device())
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype, device=dev)
        self.g = {n: up(gt[n]) for n in ('x', 'y', 'w', 'h', 'area', 'cat', 'crowd', 'image_gt_offsets')}
        self.d = {n: up(p[n]) for n in COCO_DET_COLUMNS + ('cat', 'set_row_offsets', 'image_det_offsets')}
        self.mask = up(p['has_rows']) if dt_images else None
        z = lambda s, dt: torch.zeros(s, dtype=dt, device=dev)
        n = max(1, self.n_det)
        self.out = dict(precision=z((self.K, T, R, nc, A, M), torch.float64), recall=z((self.K, T, nc, A, M), torch.float64),
                        npig=z((self.K, nc, A), torch.int64))
        if per_row:
            self.out.update(rank=z(n, torch.int32), match_gt=z((n, A, T), torch.int64), ignore=z((n, A, T), torch.uint8))
        self.status = z(1, torch.int32)
        self.ws_bytes = int(self.lib.wt_det_coco_workspace(C.c_int32(self.K), C.c_int64(self.n_images), C.c_int32(nc), C.c_int32(T), C.c_int32(R),
                                                           C.c_int32(A), C.c_int32(M), C.c_int64(gt['x'].size), C.c_int64(self.n_det)))
        if not self.ws_bytes:
            _lib.check(4, 'wt_det_coco_workspace')
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)

    def launch(self):
        g, d, o, v = self.g, self.d, self.out, C.c_void_p
        p = lambda t: v(t.data_ptr()) if t is not None else None
        thr, rec, areas, md = self.host
        rc = self.lib.wt_det_coco_dev(
            C.c_int64(self.gt['x'].size), p(g['x']), p(g['y']), p(g['w']), p(g['h']), p(g['area']), p(g['cat']), p(g['crowd']),
            C.c_int64(self.n_images), p(g['image_gt_offsets']), C.c_int32(self.K), C.c_int64(self.n_det), p(d['set_row_offsets']), p(d['image_det_offsets']),
            p(d['score']), p(d['x']), p(d['y']), p(d['w']), p(d['h']), p(d['cat']), p(self.mask),
            C.c_int32(self.gt['n_cats']), C.c_int32(len(thr)), _lib.ptr(thr), C.c_int32(len(rec)), _lib.ptr(rec), C.c_int32(len(areas)), _lib.ptr(areas),
            C.c_int32(len(md)), _lib.ptr(md), p(o['precision']), p(o['recall']), p(o['npig']), p(o.get('rank')), p(o.get('match_gt')), p(o.get('ignore')),
            p(self.status), p(self.ws), C.c_size_t(self.ws_bytes), v(self.torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, 'wt_det_coco_dev')

    def results(self, cat_ids=None):
        self.torch.cuda.current_stream().synchronize()
        st = int(self.status.item())
        if st:
            raise _lib.WaymoTrackError('wt_det_coco_dev failed: %s (status reported by the kernel)' % _lib._STATUS.get(st, st))
        out = {k: t.cpu().numpy() for k, t in self.out.items()}
        for k in ('rank', 'match_gt', 'ignore'):
            if k in out:
                out[k] = out[k][:self.n_det]
        return _coco_results(self.gt, self.p, out, self.per_row, cat_ids)


# ---------------------------------------------------------------------------------------------------------------
# ensemble sweep
def _grid_values(text):
    """'0.4:0.8:0.05' (inclusive range) or '0.9,1.0' -> list of floats."""
    if ':' in text:
        lo, hi, step = (float(v) for v in text.split(':'))
        n = int(math.floor((hi - lo) / step + 1e-9)) + 1
        return [round(lo + i * step, 10) for i in range(n)]
    return [float(v) for v in text.split(',')]


# sweep names of the merge rules of detnet/ensemble_b.py -> its -m value; only iou_thresh varies for them
B_METHODS = {'weighted_fusion_b': 'weighted_fusion', 'nmw': 'nmw'}


def flag_line(setting):
    """The tail of the `python -m waymo_2d_tracking_amd.detnet.ensemble` command line of a sweep setting; for the methods of
    B_METHODS the tail of the `python -m waymo_2d_tracking_amd.detnet.ensemble_b` command line."""
    if setting['method'] in B_METHODS:
        return '-m %s --iou-thresh=%r' % (B_METHODS[setting['method']], float(setting['iou_thresh']))
    return '-m %s --iou-thresh=%r --soft-nms-cut=%r --min-score=%r' % (
        setting['method'], float(setting['iou_thresh']), float(setting['soft_nms_cut']), float(setting['min_score']))


class SweepResult(object):
    """settings (grid order), results (DetResult per setting), mean_ap per setting, ranked (indices into settings, best first),
    best (the winning setting) and flag_line() (its ensemble command-line tail)."""

    def __init__(self, settings, results, mean_ap, ranked):
        self.settings, self.results, self.mean_ap, self.ranked = settings, results, mean_ap, ranked
        self.best = settings[ranked[0]]

    def flag_line(self):
        return flag_line(self.best)


def sweep(inputs, gt, grid, weights=None, metric='waymo', min_conf=0.01, coco_call=None):
    """Merge the input detection files (paths, or parsed row lists) under every setting of `grid` - dict with lists 'method',
    'iou_thresh', 'soft_nms_cut', 'min_score', iterated in that nesting - with the ensemble's own code path, and score all K
    merged results in ONE evaluation call.  The methods 'weighted_fusion_b' and 'nmw' are the merge rules of detnet/ensemble_b.py:
    only iou_thresh varies for them (one setting per value, soft_nms_cut and min_score reported as None) and `weights` reach
    them as given.  Ranked by mean AP over the classes with ground truth; ties go to grid order.  metric='coco' scores with
    evaluate_coco_sets instead (min_conf does not apply) and ranks by stats[0], COCO mAP; the results are CocoResult.
    Returns a SweepResult."""
    from . import ensemble as E
    gt = pack_coco_ground_truth(gt) if metric == 'coco' else pack_ground_truth(gt)
    subs = [E.read_submission(f) if not isinstance(f, (list, tuple, dict)) else (f if isinstance(f, dict) else E.submission_columns(list(f)))
            for f in inputs]
    w = E.normalise_weights(weights, len(subs))
    settings, merged = [], []
    for method in grid['method']:
        if method in B_METHODS:                      # weighted boxes fusion / NMW: no cut, no minimal score - one setting per IoU value
            from . import ensemble_b as EB
            for iou in grid['iou_thresh']:
                image_ids, o = EB.fuse_submissions(subs, B_METHODS[method], iou, weights)
                b = o['bbox']
                merged.append(dict(image_ids=image_ids, image=o['image'], category=o['category'], score=o['score'],
                                   x=b[:, 0], y=b[:, 1], w=b[:, 2], h=b[:, 3]))
                settings.append({'method': method, 'iou_thresh': float(iou), 'soft_nms_cut': None, 'min_score': None})
            continue
        if method not in E.METHODS:
            raise ValueError('unknown ensemble method %r' % (method,))
        for iou in grid['iou_thresh']:
            for cut in grid['soft_nms_cut']:
                for min_score in grid['min_score']:
                    image_ids, category_ids, rows = E.merge_inputs(subs, w, min_score)
                    packed = E.pack_groups(len(image_ids), category_ids, rows, len(subs))
                    out5, counts = E.merge_groups(packed, len(subs), method, iou, cut)
                    o = E.output_rows(packed, category_ids, out5, counts, min_score)
                    b = o['bbox'].astype(np.float64).reshape(-1, 4)
                    merged.append(dict(image_ids=image_ids, image=o['image'], category=o['category'], score=o['score'],
                                       x=b[:, 0], y=b[:, 1], w=b[:, 2], h=b[:, 3]))
                    settings.append({'method': method, 'iou_thresh': float(iou), 'soft_nms_cut': float(cut), 'min_score': float(min_score)})
    if not settings:
        raise ValueError('the grid is empty')
    if metric == 'coco':                             # before thresholds(): it has no such preset, the COCO rule is another algorithm
        results = evaluate_coco_sets(gt, merged, call=coco_call)
        mean_ap = [float(r.stats[0]) for r in results]
    else:
        results = evaluate_detection_sets(gt, merged, metric, min_conf)
        mean_ap = [r.mean_ap() for r in results]
    ranked = sorted(range(len(settings)), key=lambda i: (-(mean_ap[i] if mean_ap[i] == mean_ap[i] else -math.inf), i))
    return SweepResult(settings, results, mean_ap, ranked)


# ---------------------------------------------------------------------------------------------------------------
# command line
def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('detections', nargs='*', help='detection JSON files (detnet/export.py, detnet/ensemble.py)')
    parser.add_argument('--annotations', required=True, help='ground-truth COCO json (waymo_to_coco.py)')
    parser.add_argument('--metric', choices=sorted(METRICS), default='waymo')
    parser.add_argument('--coco', action='store_true', help='score with the COCO metric (AP@[.5:.95], twelve numbers) instead of --metric; with --sweep rank by COCO mAP')
    parser.add_argument('--dt-images', action='store_true', help='--coco: per file only the images with at least one detection take part')
    parser.add_argument('--min-conf', type=float, default=0.01, help='detections with a confidence above this take part')
    parser.add_argument('--json', help='write the summaries (or the sweep) to this file')
    parser.add_argument('--sweep', nargs='+', help='input detection files: merge them under every grid setting and rank the settings')
    parser.add_argument('--method', default='soft_nms', help="comma-separated ensemble methods, e.g. 'soft_nms,nms'; 'weighted_fusion_b' and 'nmw' are the rules of detnet.ensemble_b")
    parser.add_argument('--iou-grid', default='0.4:0.8:0.05')
    parser.add_argument('--cut-grid', default='0.9,1.0')
    parser.add_argument('--min-score-grid', default='0,0.01')
    parser.add_argument('--weights', help="per-input weights, e.g. '1,0.8' (divided by their maximum)")
    parser.add_argument('--top', type=int, default=10, help='ranked settings to print')
    return parser


def grid_from_args(args):
    return {'method': [m.strip() for m in args.method.split(',')], 'iou_thresh': _grid_values(args.iou_grid),
            'soft_nms_cut': _grid_values(args.cut_grid), 'min_score': _grid_values(args.min_score_grid)}


def main(argv=None, coco_call=None):
    """coco_call replaces the HIP call of --coco (tests: the restatement)."""
    args = build_parser().parse_args(argv)
    if args.sweep:
        if args.detections:
            raise SystemExit('give either detection files to score or --sweep INPUTS, not both')
        if len(args.sweep) < 2:
            raise SystemExit('--sweep needs at least two input files to merge')
        weights = [float(v) for v in args.weights.split(',')] if args.weights else None
        res = sweep(args.sweep, args.annotations, grid_from_args(args), weights, 'coco' if args.coco else args.metric, args.min_conf, coco_call)
        print('%d settings merged and scored' % len(res.settings))
        for i in res.ranked[:args.top]:
            print('  %s %.5f  %s' % ('COCO mAP' if args.coco else 'mean AP', res.mean_ap[i], flag_line(res.settings[i])))
        if args.json:
            with open(args.json, 'wt') as fp:
                json.dump({'settings': res.settings, 'mean_ap': res.mean_ap, 'ranked': res.ranked,
                           'summaries': [dict(zip(COCO_STATS, r.stats.tolist())) if args.coco else r.summary() for r in res.results]}, fp)
        print(res.flag_line())
        return 0
    if not args.detections:
        raise SystemExit('give at least one detection JSON, or --sweep A.json B.json ...')
    if args.coco:
        results = evaluate_coco_sets(args.annotations, args.detections, dt_images=args.dt_images, call=coco_call)
        for path, r in zip(args.detections, results):
            print(path)
            for line in r.lines():
                print(line)
        if args.json:
            with open(args.json, 'wt') as fp:
                json.dump({p: dict(zip(COCO_STATS, r.stats.tolist())) for p, r in zip(args.detections, results)}, fp)
        return 0
    results = evaluate_detection_sets(args.annotations, args.detections, args.metric, args.min_conf)
    for path, r in zip(args.detections, results):
        print(path)
        for line in r.lines():
            print(line)
    if args.json:
        with open(args.json, 'wt') as fp:
            json.dump({p: r.summary() for p, r in zip(args.detections, results)}, fp)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
