"""Suppress duplicate tracks on the GPU: track-level non-maximum suppression per stream and class.

    outs = dedup_tracks(packed, [out], [{'min_frames': 3, 'dup_iou': 0.7}, {'min_frames': [5, 3, 0, 3], 'dup_frac': 0.8}])

DESIGN.md section 23 has the definition.  Detections that come from a soft-NMS or fusion ensemble keep a second, looser box on
many objects; the tracker starts a track on it that lives as long as the true one, every row of it a false positive.  Two
trajectories of one class whose boxes overlap by dup_iou in at least min_frames frame slots and in at least dup_frac of the shorter
one's rows are duplicates; the trajectories are walked from strongest (most rows, then highest score sum) to weakest and one is
dropped when a stronger kept one is its duplicate.  Every (job, segment, camera) is an independent problem and one wavefront of
the HIP kernels behind ``wt_dedup_tracks_*`` (include/waymotrack.h); R results are deduplicated under J settings in one call.
The decision is made on the device; the host only selects the rows with the mask.  Without a GPU the calls fail.
"""
import ctypes as C

import numpy as np

from .. import _lib
from . import _trackset as TS
from ._trackset import COLUMNS as _COLUMNS

_JOB = ('job_result', 'job_min_frames', 'job_dup_iou', 'job_dup_frac')
_OUT = ('keep', 'by', 'match', 'row_keep', 'dropped')


def _per_class(value, n_classes, kind):
    return TS.per_class(value, n_classes, kind, 'min_frames / dup_iou / dup_frac')


def _prepare(packed, outs, jobs, n_classes):
    """Everything wt_dedup_tracks_* takes, as numpy arrays (include/waymotrack.h): the shared layout, the jobs of the
    deduplication, and per trajectory the object id it has in the caller's rows."""
    p = TS.prepare(packed, outs, jobs, n_classes, 'dedup')
    J = p['J']
    p['job_min_frames'] = np.asarray([_per_class(j.get('min_frames', 0), n_classes, int) for j in jobs], dtype=np.int32).reshape(J, n_classes)
    p['job_dup_iou'] = np.asarray([_per_class(j.get('dup_iou', 0.7), n_classes, float) for j in jobs], dtype=np.float64).reshape(J, n_classes)
    p['job_dup_frac'] = np.asarray([_per_class(j.get('dup_frac', 0.5), n_classes, float) for j in jobs], dtype=np.float64).reshape(J, n_classes)
    if J and p['job_min_frames'].min() < 0:
        raise ValueError('min_frames must be >= 0')
    if np.isnan(p['job_dup_iou']).any():
        raise ValueError('dup_iou must not be NaN')
    if not ((p['job_dup_frac'] >= 0) & (p['job_dup_frac'] <= 1)).all():
        raise ValueError('dup_frac must be in 0..1')
    p['traj_ids'] = TS.traj_ids(p, outs)[1]
    return p


def _job_dicts(p, outs, keep, by, match, row_keep, dropped):
    """The J results as dicts of the form utils.track_packed returns - the surviving rows in the caller's order - plus 'keep',
    'by', 'match' per trajectory with 'traj_offsets', 'n_dropped' per stream, 'dropped' (object id, the suppressor's object id, m
    per suppressed trajectory) and 'row_keep' over the input rows."""
    S = p['n_streams']
    py = lambda v: v.item() if isinstance(v, np.generic) else v
    results = []
    for j in range(p['J']):
        r = int(p['job_result'][j])
        lo, hi = int(p['set_row_offsets'][r]), int(p['set_row_offsets'][r + 1])
        t0, t1 = int(p['traj_offsets'][r * S]), int(p['traj_offsets'][(r + 1) * S])
        mask = np.zeros(hi - lo, bool)
        mask[p['orders'][r]] = row_keep[j, lo:hi] != 0
        out = dict((k, np.asarray(v)[mask]) for k, v in outs[r].items() if k in ('frame', 'category', 'bbox', 'score', 'object_id'))
        kj, bj, mj = keep[j, t0:t1], by[j, t0:t1], match[j, t0:t1]
        offsets = (p['traj_offsets'][r * S:(r + 1) * S + 1] - t0).astype(np.int64)
        gone = np.nonzero(kj == 0)[0]
        base = offsets[np.searchsorted(offsets, gone, side='right') - 1] if gone.size else gone
        ids = p['traj_ids'][r]
        out['dropped'] = [(py(ids[t]), py(ids[b + bj[t]]), int(mj[t])) for t, b in zip(gone, base)]
        out.update(keep=kj.copy(), by=bj.copy(), match=mj.copy(), traj_offsets=offsets, n_dropped=dropped[j].copy(), row_keep=mask.astype(np.int32))
        results.append(out)
    return results


def _host_call(p, outputs):
    """wt_dedup_tracks_host on _prepare() output; outputs: keep, by, match, row_keep, dropped, each exactly (J, n) C-contiguous."""
    ptr = _lib.ptr
    return _lib.lib().wt_dedup_tracks_host(*TS.leading_args(p, p, ptr, True, _COLUMNS), ptr(p['n_traj']), *TS.job_args(p, p, ptr, _JOB),
                                           *[ptr(x) for x in outputs])


def dedup_tracks(packed, outs, jobs, n_classes=4):
    """Deduplicate R tracker outputs (dicts as utils.track_packed or stitch.stitch_tracks return them, over the frame slots of
    `packed`) under J jobs in ONE wt_dedup_tracks_host call.  A job is a dict: 'result' (index into outs, default 0), 'min_frames'
    (one int or one per class, default 0 = the class is untouched), 'dup_iou' (default 0.7) and 'dup_frac' (default 0.5), each one
    float or one per class.  Returns J dicts of the form track_packed returns, the surviving rows in the caller's order with their
    input bits, plus 'dropped'; utils.format_tracks, NativeDetFile.write_tracks, refine.refine_tracks and
    evaluate.tracks_from_packed take them as they are."""
    p = _prepare(packed, outs, jobs, n_classes)
    J, nt, nr, S = p['J'], p['n_traj_total'], p['n_rows'], p['n_streams']
    o = [np.zeros((J, nt), np.int32), np.zeros((J, nt), np.int32), np.zeros((J, nt), np.int32), np.zeros((J, nr), np.int32),
         np.zeros((J, S), np.int64)]
    _lib.check(_host_call(p, o), 'wt_dedup_tracks_host')
    return _job_dicts(p, outs, *o)


class DeviceDedup(TS.DeviceStage):
    """The same deduplication with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues
    wt_dedup_tracks_dev on the current torch stream and returns at once - the output sizes are known up front, nothing is read
    back in between; ``results()`` synchronises and reads the outputs.  ``self.out`` holds the output tensors."""
    stage = 'dedup'
    name = 'wt_dedup_tracks_dev'

    def __init__(self, packed, outs, jobs, n_classes=4, workspace_bytes=None):
        TS.DeviceStage.__init__(self, _prepare(packed, outs, jobs, n_classes), _COLUMNS + _JOB, workspace_bytes)
        torch, p = self.torch, self.p
        self.outs = outs
        J, nt, nr, S = p['J'], p['n_traj_total'], p['n_rows'], p['n_streams']
        self.shapes = dict(keep=(J, nt), by=(J, nt), match=(J, nt), row_keep=(J, nr), dropped=(J, S))
        self.out = dict((k, self.zeros(max(1, s[0] * s[1]), torch.int64 if k == 'dropped' else torch.int32)) for k, s in self.shapes.items())

    def launch(self):
        p, t, d = self.p, self.t, self.d
        rc = self.lib.wt_dedup_tracks_dev(*TS.leading_args(p, t, d, False, _COLUMNS), *self.traj_args(), *TS.job_args(p, t, d, _JOB),
                                          *[d(self.out[k]) for k in _OUT], *self.tail_args())
        _lib.check(rc, self.name)

    def rounds(self):
        """(J, n_streams): the sweeps over the slots the matching of each problem took, after a launch (a measurement)."""
        self.wait()
        J, S = self.p['J'], self.p['n_streams']
        out = np.zeros((J, S), np.int32)
        _lib.check(self.lib.wt_dedup_tracks_rounds(self.d(self.ws), C.c_int32(J), C.c_int32(S), _lib.ptr(out)), 'wt_dedup_tracks_rounds')
        return out

    def results(self):
        self.wait()
        o = dict((k, self.out[k].cpu().numpy()[:s[0] * s[1]].reshape(s)) for k, s in self.shapes.items())
        return _job_dicts(self.p, self.outs, *[o[k] for k in _OUT])


def dedup_one(packed, out, min_frames, dup_iou=0.7, dup_frac=0.5, n_classes=4):
    """One result, one setting; the input itself when the setting drops nothing (tracking/track.py with its default flags)."""
    frames = _per_class(min_frames, n_classes, int)
    if max(frames) == 0:
        return out
    job = {'min_frames': frames, 'dup_iou': _per_class(dup_iou, n_classes, float), 'dup_frac': _per_class(dup_frac, n_classes, float)}
    return dedup_tracks(packed, [out], [job], n_classes)[0]
