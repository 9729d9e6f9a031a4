"""Smooth tracking results on the GPU: a symmetric window filter over the boxes of every trajectory (the third post-pass).

    outs = smooth_tracks(packed, [out], [{'window': 2, 'kernel': 'gaussian', 'sigma': 1.0}, {'window': [3, 1, 0, 1], 'kernel': 'box'}])

DESIGN.md section 22 has the definition.  A detector's boxes jitter from frame to frame; that jitter is what HOTA's LocA, MOTP and
every match next to the IoU threshold measure.  Every box becomes the weighted mean of itself and of its trajectory's boxes
d = 1 .. window frame slots before and after it, a distance counting only when both sides are there: the ends of a trajectory never
move, a row next to a hole is not pulled to one side, and motion at constant velocity is kept.  The weights are computed here, on
the host (the kernel never evaluates exp); every (job, row) is one lane of the HIP kernels behind ``wt_smooth_tracks_*``
(include/waymotrack.h), and R results are smoothed under J settings in one call.  No arithmetic of the smoothing runs on the host;
without a GPU the calls fail.
"""
import ctypes as C
import math

import numpy as np

from .. import _lib
from . import _trackset as TS

MAX_WINDOW = 32                                      # WT_SMOOTH_MAX_WINDOW
KERNELS = ('gaussian', 'box')
_COLUMNS = ('x', 'y', 'w', 'h', 'category', 'local')
_JOB = ('job_result', 'job_window', 'job_weights')


def _per_class(value, n_classes, kind):
    return TS.per_class(value, n_classes, kind, 'window / sigma')


def kernel_weights(kernel, sigma, n):
    """k[0 .. n - 1] of one class: 'gaussian' exp(-(d * d) / (2 sigma sigma)), 'box' all ones"""
    if kernel == 'box':
        return [1.0] * n
    if kernel != 'gaussian':
        raise ValueError("kernel must be 'gaussian' or 'box'")
    sigma = float(sigma)
    if not sigma > 0.0 or math.isinf(sigma):
        raise ValueError('sigma must be a positive number')
    return [math.exp(-(d * d) / (2.0 * sigma * sigma)) for d in range(n)]


def _job_weights(job, window, n_classes):
    """(n_classes, n) weights of one job: its 'weights' (one table, or one per class) or its 'kernel' with 'sigma'"""
    if 'weights' in job:
        k = np.asarray(job['weights'], dtype=np.float64)
        if k.ndim == 1:
            k = np.tile(k, (n_classes, 1))
        if k.ndim != 2 or k.shape[0] != n_classes or k.shape[1] < 1:
            raise ValueError('weights need one table, or one per class (%d)' % n_classes)
        return k
    sigma = _per_class(job.get('sigma', 1.0), n_classes, float)
    return np.asarray([kernel_weights(job.get('kernel', 'gaussian'), sigma[c], max(window) + 1) for c in range(n_classes)], dtype=np.float64)


def _prepare(packed, outs, jobs, n_classes):
    """Everything wt_smooth_tracks_* takes, as numpy arrays (include/waymotrack.h): the shared layout and the jobs of the
    smoothing, their weight tables padded with zeros to one length."""
    p = TS.prepare(packed, outs, jobs, n_classes, 'smooth')
    J = p['J']
    windows = [_per_class(j.get('window', 0), n_classes, int) for j in jobs]
    p['job_window'] = np.asarray(windows, dtype=np.int32).reshape(J, n_classes)
    if J and (p['job_window'].min() < 0 or p['job_window'].max() > MAX_WINDOW):
        raise ValueError('window must be in 0..%d' % MAX_WINDOW)
    tables = [_job_weights(j, w, n_classes) for j, w in zip(jobs, windows)]
    for w, k in zip(windows, tables):
        if k.shape[1] <= max(w):
            raise ValueError('a window of %d needs %d weights, %d given' % (max(w), max(w) + 1, k.shape[1]))
        if not np.isfinite(k).all() or (k < 0).any() or not (k[:, 0] > 0).all():
            raise ValueError('weights must be finite and >= 0, the first one > 0')
    n = max([k.shape[1] for k in tables] + [1])
    p['n_weights'] = n
    p['job_weights'] = np.zeros((J, n_classes, n), np.float64)
    for j, k in enumerate(tables):
        p['job_weights'][j, :, :k.shape[1]] = k
    rows = np.diff(p['set_row_offsets'])
    p['job_row_offsets'] = np.concatenate([[0], np.cumsum(rows[p['job_result']])]).astype(np.int64)
    return p


def _job_dicts(p, outs, bbox, pairs):
    """The J results as dicts of the form utils.track_packed returns - the caller's rows in the caller's order, bbox replaced by the
    smoothed one - plus 'pairs' (per row, the distances that contributed)."""
    results = []
    for j in range(p['J']):
        r = int(p['job_result'][j])
        lo, hi = int(p['job_row_offsets'][j]), int(p['job_row_offsets'][j + 1])
        order = p['orders'][r]
        out = dict((k, np.asarray(v)) for k, v in outs[r].items())
        smoothed = np.empty((hi - lo, 4), np.float64)
        smoothed[order] = bbox[lo:hi]
        n = np.empty(hi - lo, np.int32)
        n[order] = pairs[lo:hi]
        out['bbox'] = smoothed
        out['pairs'] = n
        results.append(out)
    return results


def _host_call(p, outputs):
    """wt_smooth_tracks_host on _prepare() output; outputs: bbox (n, 4) float64 and pairs (n) int32, n = job_row_offsets[-1]."""
    ptr = _lib.ptr
    return _lib.lib().wt_smooth_tracks_host(*TS.leading_args(p, p, ptr, True, _COLUMNS), ptr(p['n_traj']),
                                            *TS.job_args(p, p, ptr, _JOB, ('n_weights',)), *[ptr(x) for x in outputs])


def smooth_tracks(packed, outs, jobs, n_classes=4):
    """Smooth R tracker outputs (dicts as utils.track_packed, refine.refine_tracks or stitch.stitch_tracks return them, over the
    frame slots of `packed`) under J jobs in ONE wt_smooth_tracks_host call.  A job is a dict: 'result' (index into outs, default 0),
    'window' (frame slots to either side, one int or one per class, default 0 = untouched, at most 32) and either 'weights' (k[0 ..],
    one table or one per class) or 'kernel' ('gaussian', the default, with 'sigma', one float or one per class, default 1.0; or
    'box').  Returns J dicts of the form track_packed returns, rows in the caller's order, only bbox changed, plus 'pairs';
    utils.format_tracks, NativeDetFile.write_tracks and evaluate.tracks_from_packed take them as they are."""
    p = _prepare(packed, outs, jobs, n_classes)
    n = int(p['job_row_offsets'][-1])
    o = [np.zeros((n, 4), np.float64), np.zeros(n, np.int32)]
    _lib.check(_host_call(p, o), 'wt_smooth_tracks_host')
    return _job_dicts(p, outs, *o)


class DeviceSmooth(TS.DeviceStage):
    """The same smoothing with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues
    wt_smooth_tracks_dev on the current torch stream and returns at once - the output sizes are known up front, nothing is read
    back in between; ``results()`` synchronises and reads the outputs.  ``self.out`` holds the output tensors."""
    stage = 'smooth'
    name = 'wt_smooth_tracks_dev'

    def __init__(self, packed, outs, jobs, n_classes=4, workspace_bytes=None):
        TS.DeviceStage.__init__(self, _prepare(packed, outs, jobs, n_classes), _COLUMNS + _JOB + ('job_row_offsets',), workspace_bytes)
        self.outs = outs
        self.n_out = int(self.p['job_row_offsets'][-1])
        self.out = dict(bbox=self.zeros((max(1, self.n_out), 4), self.torch.float64), pairs=self.zeros(max(1, self.n_out), self.torch.int32))

    def launch(self):
        p, t, d, o = self.p, self.t, self.d, self.out
        rc = self.lib.wt_smooth_tracks_dev(
            *TS.leading_args(p, t, d, False, _COLUMNS), *self.traj_args(), *TS.job_args(p, t, d, _JOB, ('n_weights',)),
            d(t['job_row_offsets']), C.c_int64(self.n_out), d(o['bbox']), d(o['pairs']), *self.tail_args())
        _lib.check(rc, self.name)

    def results(self):
        self.wait()
        return _job_dicts(self.p, self.outs, self.out['bbox'].cpu().numpy()[:self.n_out], self.out['pairs'].cpu().numpy()[:self.n_out])


def smooth_one(packed, out, window, sigma=1.0, kernel='gaussian', n_classes=4):
    """One result, one setting; the input itself when every window is 0 (tracking/track.py with its default flags)."""
    w = _per_class(window, n_classes, int)
    if max(w) == 0:
        return out
    return smooth_tracks(packed, [out], [{'window': w, 'sigma': _per_class(sigma, n_classes, float), 'kernel': kernel}], n_classes)[0]
