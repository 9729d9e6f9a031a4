"""Repair class flicker on the GPU: link tracklets of one stream across gaps AND classes, and give every chain one class.

    outs = xlink_tracks(packed, [out], [{'pairs': {(2, 4): {'max_link': 2, 'link_iou': 0.3}}, 'prio': [0, 0, 0, 1], 'motion': 'hold'}])

DESIGN.md section 31 has the definition.  The detector, its NMS, the ensembles and the tracker all work per category: when a
cyclist is called a pedestrian for two frames the cyclist track ends, a pedestrian track is born and dies, and a new cyclist track
is born - one object, three trajectories, two classes.  A tracklet that ends is linked to one that begins up to the pair's max_link
frame slots later when its (held or linearly extrapolated) last box overlaps the other's first box by at least the pair's
link_iou, the pair being (class of the tail, class of the head); linked pieces take the id of the earliest one, and every row of a
chain takes the class most of the chain's rows have (then the class priority, then the root's class, then the lower class).
Every (job, segment, camera) is an independent problem and one wavefront of the HIP kernels behind ``wt_xlink_tracks_*``
(include/waymotrack.h); R results are linked under J settings in one call.  No arithmetic of the pass runs on the host; without a
GPU the calls fail.
"""
import ctypes as C

import numpy as np

from .. import _lib
from . import _trackset as TS
from .stitch import MOTIONS, _COLUMNS, _job_dicts as _stitch_dicts

_JOB = ('job_result', 'job_pair_max_link', 'job_pair_link_iou', 'job_class_prio', 'job_motion')
_OUT = ('pred', 'root', 'affinity', 'cls', 'row_root', 'row_category', 'links', 'relabelled')
MAX_CLASSES = 16


def pair_tables(pairs, n_classes):
    """The symmetric (n_classes, n_classes) tables max_link, link_iou of a job's unordered `pairs`:
    {(a, b): {'max_link': 1, 'link_iou': 0.3}}, classes from 1, (a, a) allowed; a pair that is not named is off."""
    max_link = np.zeros((n_classes, n_classes), np.int32)
    link_iou = np.full((n_classes, n_classes), 0.3, np.float64)
    seen = set()
    for (a, b), v in pairs.items():
        a, b = int(a), int(b)
        if not (1 <= a <= n_classes and 1 <= b <= n_classes):
            raise ValueError('pair (%d, %d): classes are 1..%d' % (a, b, n_classes))
        if (min(a, b), max(a, b)) in seen:
            raise ValueError('pair (%d, %d) is given twice (pairs are unordered)' % (a, b))
        seen.add((min(a, b), max(a, b)))
        for i, k in ((a - 1, b - 1), (b - 1, a - 1)):
            max_link[i, k], link_iou[i, k] = int(v.get('max_link', 1)), float(v.get('link_iou', 0.3))
    return max_link, link_iou


def _prepare(packed, outs, jobs, n_classes):
    """Everything wt_xlink_tracks_* takes, as numpy arrays (include/waymotrack.h): the shared layout, the jobs, and per trajectory
    the object id it has in the caller's rows."""
    if n_classes > MAX_CLASSES:
        raise ValueError('at most %d classes' % MAX_CLASSES)
    p = TS.prepare(packed, outs, jobs, n_classes, 'xlink')
    J = p['J']
    tables = [pair_tables(j.get('pairs', {}), n_classes) for j in jobs]
    for i, name in enumerate(('job_pair_max_link', 'job_pair_link_iou')):
        p[name] = np.ascontiguousarray(np.stack([t[i] for t in tables]) if J else np.zeros((0, n_classes, n_classes), np.float64 if i else np.int32))
    p['job_class_prio'] = np.asarray([TS.per_class(j.get('prio', 0), n_classes, int, 'prio') for j in jobs], dtype=np.int32).reshape(J, n_classes)
    for j in jobs:
        if j.get('motion', 'hold') not in MOTIONS:
            raise ValueError("motion must be 'hold' or 'linear'")
    p['job_motion'] = np.asarray([MOTIONS[j.get('motion', 'hold')] for j in jobs], dtype=np.int32).reshape(J)
    if J and (p['job_pair_max_link'].min() < 0 or np.isnan(p['job_pair_link_iou']).any()):
        raise ValueError('max_link must be >= 0 and link_iou must not be NaN')
    p['row_stream_base'], p['traj_ids'] = TS.traj_ids(p, outs)
    return p


def _job_dicts(p, outs, pred, root, affinity, cls, row_root, row_category, n_links, n_relabelled):
    """The J results as dicts of the form utils.track_packed returns - the caller's rows in the caller's order, object_id replaced
    by the root's and category by the chain's class - plus what stitch.stitch_tracks adds ('links', 'n_links', 'pred', 'root',
    'affinity', 'row_root', 'traj_offsets'), the per-trajectory 'cls' and 'n_relabelled' per stream."""
    S = p['n_streams']
    results = _stitch_dicts(p, outs, pred, root, affinity, row_root, n_links)
    for j, out in enumerate(results):
        r = int(p['job_result'][j])
        lo, hi = int(p['set_row_offsets'][r]), int(p['set_row_offsets'][r + 1])
        t0, t1 = int(p['traj_offsets'][r * S]), int(p['traj_offsets'][(r + 1) * S])
        cat = np.asarray(out['category']).copy()
        cat[p['orders'][r]] = row_category[j, lo:hi]
        out.update(category=cat, cls=cls[j, t0:t1].copy(), n_relabelled=n_relabelled[j].copy())
    return results


def _outputs(p):
    J, nt, nr, S = p['J'], p['n_traj_total'], p['n_rows'], p['n_streams']
    return dict(pred=((J, nt), np.int32), root=((J, nt), np.int32), affinity=((J, nt), np.float64), cls=((J, nt), np.int32),
                row_root=((J, nr), np.int32), row_category=((J, nr), np.int32), links=((J, S), np.int64), relabelled=((J, S), np.int64))


def _host_call(p, outputs):
    """wt_xlink_tracks_host on _prepare() output; outputs: the arrays of _OUT in that order, each exactly (J, n) C-contiguous."""
    ptr = _lib.ptr
    return _lib.lib().wt_xlink_tracks_host(*TS.leading_args(p, p, ptr, True, _COLUMNS), ptr(p['n_traj']), *TS.job_args(p, p, ptr, _JOB),
                                           *[ptr(x) for x in outputs])


def xlink_tracks(packed, outs, jobs, n_classes=4):
    """Link R tracker outputs (dicts as utils.track_packed or an earlier pass return them, over the frame slots of `packed`) under
    J jobs in ONE wt_xlink_tracks_host call.  A job is a dict: 'result' (index into outs, default 0), 'pairs' {(a, b): {'max_link'
    (frame slots, default 1; 0 = off), 'link_iou' (default 0.3)}} - unordered class pairs, (a, a) allowed, a pair that is not named
    is off - 'prio' (one int or one per class, default 0) and 'motion' ('hold' or 'linear').  Returns J dicts of the form
    track_packed returns, rows in the caller's order, object_id and category replaced, plus 'links' and the per-trajectory
    arrays; the next pass, the writers and evaluate.tracks_from_packed take them as they are."""
    p = _prepare(packed, outs, jobs, n_classes)
    shapes = _outputs(p)
    o = [np.zeros(*shapes[k]) for k in _OUT]
    _lib.check(_host_call(p, o), 'wt_xlink_tracks_host')
    return _job_dicts(p, outs, *o)


class DeviceXLink(TS.DeviceStage):
    """The same pass with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues wt_xlink_tracks_dev on
    the current torch stream and returns at once - the output sizes are known up front, nothing is read back in between;
    ``results()`` synchronises and reads the outputs.  ``self.out`` holds the output tensors."""
    stage = 'xlink'
    name = 'wt_xlink_tracks_dev'

    def __init__(self, packed, outs, jobs, n_classes=4, workspace_bytes=None):
        TS.DeviceStage.__init__(self, _prepare(packed, outs, jobs, n_classes), _COLUMNS + _JOB, workspace_bytes)
        torch = self.torch
        self.outs = outs
        self.shapes = dict((k, s) for k, (s, _) in _outputs(self.p).items())
        self.out = dict((k, self.zeros(max(1, s[0] * s[1]), getattr(torch, np.dtype(dt).name))) for k, (s, dt) in _outputs(self.p).items())

    def launch(self):
        p, t, d = self.p, self.t, self.d
        rc = self.lib.wt_xlink_tracks_dev(*TS.leading_args(p, t, d, False, _COLUMNS), *self.traj_args(), *TS.job_args(p, t, d, _JOB),
                                          *[d(self.out[k]) for k in _OUT], *self.tail_args())
        _lib.check(rc, self.name)

    def rounds(self):
        """(J, n_streams): the rounds of the matching that accepted a link, after a launch (a measurement)."""
        self.wait()
        J, S = self.p['J'], self.p['n_streams']
        out = np.zeros((J, S), np.int32)
        _lib.check(self.lib.wt_xlink_tracks_rounds(self.d(self.ws), C.c_int32(J), C.c_int32(S), _lib.ptr(out)), 'wt_xlink_tracks_rounds')
        return out

    def results(self):
        self.wait()
        o = dict((k, self.out[k].cpu().numpy()[:s[0] * s[1]].reshape(s)) for k, s in self.shapes.items())
        return _job_dicts(self.p, self.outs, *[o[k] for k in _OUT])


def xlink_one(packed, out, pairs, prio=0, motion='hold', n_classes=4):
    """One result, one setting; the input itself when no pair is on (tracking/track.py with its default flags)."""
    if not any(int(v.get('max_link', 1)) > 0 for v in pairs.values()):
        return out
    return xlink_tracks(packed, [out], [{'pairs': pairs, 'prio': prio, 'motion': motion}], n_classes)[0]
