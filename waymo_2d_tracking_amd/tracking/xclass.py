"""Suppress duplicate tracks across classes on the GPU: the pedestrian track on the rider of a tracked cyclist.

    outs = xclass_tracks(packed, [out], [{'pairs': {(2, 4): {'frames': 3, 'overlap': 0.9, 'frac': 0.5}}, 'prio': [0, 0, 0, 1],
                                          'measure': 'iomin'}])

DESIGN.md section 26 has the definition.  The detector, its NMS, the ensembles and the tracker all work per category, so a second
box of another class on one object becomes a track that lives as long as the object, every row of it a false positive in its
class.  Two trajectories of one stream whose class pair is switched on are the same object when their boxes reach the pair's
overlap - IoU, or IoMin = intersection over the smaller area - in at least `frames` frame slots and in at least `frac` of the
weaker one's rows; the trajectories are walked from strongest (highest class priority, then most rows, then highest score sum) to
weakest and one is dropped when a stronger kept one is the same object.  Every (job, segment, camera) is an independent problem and
one wavefront of the HIP kernels behind ``wt_xclass_tracks_*`` (include/waymotrack.h); R results are judged under J settings in
one call.  The decision is made on the device; the host only selects the rows with the mask.  Without a GPU the calls fail.
"""
import ctypes as C

import numpy as np

from .. import _lib
from . import _trackset as TS
from ._trackset import COLUMNS as _COLUMNS
from .dedup import _job_dicts

_JOB = ('job_result', 'job_pair_frames', 'job_pair_overlap', 'job_pair_frac', 'job_class_prio', 'job_measure')
_OUT = ('keep', 'by', 'match', 'row_keep', 'dropped')
MEASURES = {'iou': 0, 'iomin': 1}
MAX_CLASSES = 16


def pair_tables(pairs, n_classes):
    """The symmetric (n_classes, n_classes) tables frames, overlap, frac of a job's unordered `pairs`:
    {(a, b): {'frames': 3, 'overlap': 0.7, 'frac': 0.5}}, classes from 1, (a, a) allowed; a pair that is not named is off."""
    frames = np.zeros((n_classes, n_classes), np.int32)
    overlap = np.full((n_classes, n_classes), 0.7, np.float64)
    frac = np.full((n_classes, n_classes), 0.5, np.float64)
    seen = set()
    for (a, b), v in pairs.items():
        a, b = int(a), int(b)
        if not (1 <= a <= n_classes and 1 <= b <= n_classes):
            raise ValueError('pair (%d, %d): classes are 1..%d' % (a, b, n_classes))
        if (min(a, b), max(a, b)) in seen:
            raise ValueError('pair (%d, %d) is given twice (pairs are unordered)' % (a, b))
        seen.add((min(a, b), max(a, b)))
        for i, k in ((a - 1, b - 1), (b - 1, a - 1)):
            frames[i, k], overlap[i, k], frac[i, k] = int(v.get('frames', 3)), float(v.get('overlap', 0.7)), float(v.get('frac', 0.5))
    return frames, overlap, frac


def _prepare(packed, outs, jobs, n_classes):
    """Everything wt_xclass_tracks_* takes, as numpy arrays (include/waymotrack.h): the shared layout, the jobs, and per trajectory
    the object id it has in the caller's rows."""
    if n_classes > MAX_CLASSES:
        raise ValueError('at most %d classes' % MAX_CLASSES)
    p = TS.prepare(packed, outs, jobs, n_classes, 'xclass')
    J = p['J']
    tables = [pair_tables(j.get('pairs', {}), n_classes) for j in jobs]
    for i, name in enumerate(('job_pair_frames', 'job_pair_overlap', 'job_pair_frac')):
        p[name] = np.ascontiguousarray(np.stack([t[i] for t in tables]) if J else np.zeros((0, n_classes, n_classes), np.float64 if i else np.int32))
    p['job_class_prio'] = np.asarray([TS.per_class(j.get('prio', 0), n_classes, int, 'prio') for j in jobs], dtype=np.int32).reshape(J, n_classes)
    for j in jobs:
        if j.get('measure', 'iomin') not in MEASURES:
            raise ValueError("measure must be 'iou' or 'iomin'")
    p['job_measure'] = np.asarray([MEASURES[j.get('measure', 'iomin')] for j in jobs], dtype=np.int32).reshape(J)
    if J and p['job_pair_frames'].min() < 0:
        raise ValueError('frames must be >= 0')
    if np.isnan(p['job_pair_overlap']).any():
        raise ValueError('overlap must not be NaN')
    if not ((p['job_pair_frac'] >= 0) & (p['job_pair_frac'] <= 1)).all():
        raise ValueError('frac must be in 0..1')
    p['traj_ids'] = TS.traj_ids(p, outs)[1]
    return p


def _host_call(p, outputs):
    """wt_xclass_tracks_host on _prepare() output; outputs: keep, by, match, row_keep, dropped, each exactly (J, n) C-contiguous."""
    ptr = _lib.ptr
    return _lib.lib().wt_xclass_tracks_host(*TS.leading_args(p, p, ptr, True, _COLUMNS), ptr(p['n_traj']), *TS.job_args(p, p, ptr, _JOB),
                                            *[ptr(x) for x in outputs])


def xclass_tracks(packed, outs, jobs, n_classes=4):
    """Judge R tracker outputs (dicts as utils.track_packed, stitch.stitch_tracks or dedup.dedup_tracks return them, over the frame
    slots of `packed`) under J jobs in ONE wt_xclass_tracks_host call.  A job is a dict: 'result' (index into outs, default 0),
    'pairs' {(a, b): {'frames' (default 3), 'overlap' (0.7), 'frac' (0.5)}} - unordered class pairs, (a, a) allowed, a pair that
    is not named is off - 'prio' (one int or one per class, default 0) and 'measure' ('iou' or 'iomin', default 'iomin').  Returns
    J dicts of the form dedup.dedup_tracks returns; the next pass, the writers and evaluate.tracks_from_packed take them as they
    are."""
    p = _prepare(packed, outs, jobs, n_classes)
    J, nt, nr, S = p['J'], p['n_traj_total'], p['n_rows'], p['n_streams']
    o = [np.zeros((J, nt), np.int32), np.zeros((J, nt), np.int32), np.zeros((J, nt), np.int32), np.zeros((J, nr), np.int32),
         np.zeros((J, S), np.int64)]
    _lib.check(_host_call(p, o), 'wt_xclass_tracks_host')
    return _job_dicts(p, outs, *o)


class DeviceXClass(TS.DeviceStage):
    """The same pass with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues wt_xclass_tracks_dev on
    the current torch stream and returns at once; ``results()`` synchronises and reads the outputs.  ``self.out`` holds the output
    tensors."""
    stage = 'xclass'
    name = 'wt_xclass_tracks_dev'

    def __init__(self, packed, outs, jobs, n_classes=4, workspace_bytes=None):
        TS.DeviceStage.__init__(self, _prepare(packed, outs, jobs, n_classes), _COLUMNS + _JOB, workspace_bytes)
        torch, p = self.torch, self.p
        self.outs = outs
        J, nt, nr, S = p['J'], p['n_traj_total'], p['n_rows'], p['n_streams']
        self.shapes = dict(keep=(J, nt), by=(J, nt), match=(J, nt), row_keep=(J, nr), dropped=(J, S))
        self.out = dict((k, self.zeros(max(1, s[0] * s[1]), torch.int64 if k == 'dropped' else torch.int32)) for k, s in self.shapes.items())

    def launch(self):
        p, t, d = self.p, self.t, self.d
        rc = self.lib.wt_xclass_tracks_dev(*TS.leading_args(p, t, d, False, _COLUMNS), *self.traj_args(), *TS.job_args(p, t, d, _JOB),
                                           *[d(self.out[k]) for k in _OUT], *self.tail_args())
        _lib.check(rc, self.name)

    def rounds(self):
        """(J, n_streams): the sweeps over the slots the matching of each problem took, after a launch (a measurement)."""
        self.wait()
        J, S = self.p['J'], self.p['n_streams']
        out = np.zeros((J, S), np.int32)
        _lib.check(self.lib.wt_xclass_tracks_rounds(self.d(self.ws), C.c_int32(J), C.c_int32(S), _lib.ptr(out)), 'wt_xclass_tracks_rounds')
        return out

    def results(self):
        self.wait()
        o = dict((k, self.out[k].cpu().numpy()[:s[0] * s[1]].reshape(s)) for k, s in self.shapes.items())
        return _job_dicts(self.p, self.outs, *[o[k] for k in _OUT])


def xclass_one(packed, out, pairs, prio=0, measure='iomin', n_classes=4):
    """One result, one setting; the input itself when no pair is on (tracking/track.py with its default flags)."""
    if not any(int(v.get('frames', 3)) > 0 for v in pairs.values()):
        return out
    return xclass_tracks(packed, [out], [{'pairs': pairs, 'prio': prio, 'measure': measure}], n_classes)[0]
