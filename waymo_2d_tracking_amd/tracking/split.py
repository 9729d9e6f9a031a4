"""Split impure tracks on the GPU: cut a trajectory where its motion jumps or a long gap opens (the pass before stitching).

    outs = split_tracks(packed, [out], [{'split_iou': 0.3}, {'split_iou': [0.3, 0.2, 0, 0.3], 'split_gap': 5, 'motion': 'hold'}])

DESIGN.md section 25 has the definition.  A tracker that associates at a low IoU threshold lets a track jump from one object to
another and keep going; no later pass can undo that - stitching links only tracks that ended, deduplication drops whole tracks,
smoothing smears the jump.  Two consecutive observations of a trajectory are separated when the box extrapolated forward from the
rows before them AND the box extrapolated backward from the rows after them (the held box when there is neither) overlap the other
side by less than split_iou, or when more than split_gap slots lie between them.  The first piece keeps the object id, every other
piece gets a new one from first_new_id on.  Every (job, row) is a lane and every (job, segment, camera) a wavefront of the HIP
kernels behind ``wt_split_tracks_*`` (include/waymotrack.h); R results are split under J settings in one call.  No arithmetic of
the splitting runs on the host; without a GPU the calls fail.
"""
import numpy as np

from .. import _lib
from . import _trackset as TS

MOTIONS = {'hold': 0, 'linear': 1}
_COLUMNS = ('x', 'y', 'w', 'h', 'category', 'local')
_JOB = ('job_result', 'job_split_iou', 'job_split_gap', 'job_motion')
_OUT = ('piece', 'new', 'test', 'breaks', 'new_pieces')


def _per_class(value, n_classes, kind):
    return TS.per_class(value, n_classes, kind, 'split_iou / split_gap')


def _prepare(packed, outs, jobs, n_classes):
    """Everything wt_split_tracks_* takes, as numpy arrays (include/waymotrack.h): the shared layout, the jobs of the splitting,
    and per job the id its first new piece gets."""
    for r, out in enumerate(outs):
        if np.asarray(out['object_id']).dtype.kind not in 'iu':
            raise ValueError('result %d: object ids must be integers (a new piece gets the id first_new_id + its number)' % r)
    p = TS.prepare(packed, outs, jobs, n_classes, 'split')
    J = p['J']
    p['job_split_iou'] = np.asarray([_per_class(j.get('split_iou', 0.0), n_classes, float) for j in jobs], dtype=np.float64).reshape(J, n_classes)
    p['job_split_gap'] = np.asarray([_per_class(j.get('split_gap', 0), n_classes, int) for j in jobs], dtype=np.int32).reshape(J, n_classes)
    if J and (p['job_split_gap'].min() < 0 or np.isnan(p['job_split_iou']).any()):
        raise ValueError('split_gap must be >= 0 and split_iou must not be NaN')
    p['job_motion'] = np.asarray([MOTIONS[j.get('motion', 'linear')] for j in jobs], dtype=np.int32).reshape(J)
    first = []
    for j, r in zip(jobs, p['job_result']):
        oid = p['object_ids'][int(r)]
        first.append(int(j['first_new_id']) if j.get('first_new_id') is not None else (int(oid.max()) + 1 if oid.size else 0))
    p['first_new_id'] = first
    return p


def _job_dicts(p, outs, piece, new, test, breaks, new_pieces):
    """The J results as dicts of the form utils.track_packed returns - the caller's rows in the caller's order, object_id of the
    rows of a new piece replaced by first_new_id + the piece's number - plus per row 'piece', 'new' and 'test', per trajectory
    'breaks' (with 'traj_offsets'), per stream 'n_new_pieces' and their sum 'n_new'."""
    S = p['n_streams']
    results = []
    for j in range(p['J']):
        r = int(p['job_result'][j])
        lo, hi = int(p['set_row_offsets'][r]), int(p['set_row_offsets'][r + 1])
        t0, t1 = int(p['traj_offsets'][r * S]), int(p['traj_offsets'][(r + 1) * S])
        order = p['orders'][r]
        out = dict((k, np.asarray(v)) for k, v in outs[r].items())
        n_new = int(new_pieces[j].sum())
        oid = np.asarray(out['object_id']).copy()
        first = p['first_new_id'][j]
        if n_new and (first < np.iinfo(oid.dtype).min or first + n_new - 1 > np.iinfo(oid.dtype).max):
            raise ValueError('job %d: the new ids %d..%d do not fit the object ids\' dtype %s' % (j, first, first + n_new - 1, oid.dtype))
        nj = new[j, lo:hi]
        fresh = np.nonzero(nj >= 0)[0]
        oid[order[fresh]] = (first + nj[fresh]).astype(oid.dtype)
        out['object_id'] = oid

        def by_caller(a):
            c = np.empty_like(a)
            c[order] = a
            return c
        out.update(piece=by_caller(piece[j, lo:hi]), new=by_caller(nj), test=by_caller(test[j, lo:hi]), breaks=breaks[j, t0:t1].copy(),
                   n_new_pieces=new_pieces[j].copy(), n_new=n_new, first_new_id=first,
                   traj_offsets=(p['traj_offsets'][r * S:(r + 1) * S + 1] - t0).astype(np.int64))
        results.append(out)
    return results


def _outputs(p):
    J, nt, nr, S = p['J'], p['n_traj_total'], p['n_rows'], p['n_streams']
    return dict(piece=((J, nr), np.int32), new=((J, nr), np.int64), test=((J, nr, 2), np.float64), breaks=((J, nt), np.int32),
                new_pieces=((J, S), np.int64))


def _host_call(p, outputs):
    """wt_split_tracks_host on _prepare() output; outputs: piece, new, test, breaks, new_pieces, each exactly its shape, C-contiguous."""
    ptr = _lib.ptr
    return _lib.lib().wt_split_tracks_host(*TS.leading_args(p, p, ptr, True, _COLUMNS), ptr(p['n_traj']), *TS.job_args(p, p, ptr, _JOB),
                                           *[ptr(x) for x in outputs])


def split_tracks(packed, outs, jobs, n_classes=4):
    """Split R tracker outputs (dicts as utils.track_packed returns them, over the frame slots of `packed`) under J jobs in ONE
    wt_split_tracks_host call.  A job is a dict: 'result' (index into outs, default 0), 'split_iou' (one float or one per class,
    default 0.0 = the IoU rule is off), 'split_gap' (frame slots, one int or one per class, default 0 = the gap rule is off),
    'motion' ('linear' or 'hold') and 'first_new_id' (default: the largest object id of the result + 1).  Returns J dicts of the
    form track_packed returns, rows in the caller's order, only object_id changed, plus 'piece', 'test', 'breaks', 'n_new';
    stitch.stitch_tracks, refine.refine_tracks, utils.format_tracks and the writers take them as they are."""
    p = _prepare(packed, outs, jobs, n_classes)
    o = [np.zeros(shape, dtype) for shape, dtype in (_outputs(p)[k] for k in _OUT)]
    _lib.check(_host_call(p, o), 'wt_split_tracks_host')
    return _job_dicts(p, outs, *o)


class DeviceSplit(TS.DeviceStage):
    """The same splitting with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues
    wt_split_tracks_dev on the current torch stream and returns at once - the output sizes are known up front, nothing is read
    back in between; ``results()`` synchronises and reads the outputs.  ``self.out`` holds the output tensors."""
    stage = 'split'
    name = 'wt_split_tracks_dev'

    def __init__(self, packed, outs, jobs, n_classes=4, workspace_bytes=None):
        TS.DeviceStage.__init__(self, _prepare(packed, outs, jobs, n_classes), _COLUMNS + _JOB, workspace_bytes)
        torch = self.torch
        self.outs = outs
        self.shapes = dict((k, v[0]) for k, v in _outputs(self.p).items())
        dtypes = dict(piece=torch.int32, new=torch.int64, test=torch.float64, breaks=torch.int32, new_pieces=torch.int64)
        self.out = dict((k, self.zeros(max(1, int(np.prod(s))), dtypes[k])) for k, s in self.shapes.items())

    def launch(self):
        p, t, d = self.p, self.t, self.d
        rc = self.lib.wt_split_tracks_dev(*TS.leading_args(p, t, d, False, _COLUMNS), *self.traj_args(), *TS.job_args(p, t, d, _JOB),
                                          *[d(self.out[k]) for k in _OUT], *self.tail_args())
        _lib.check(rc, self.name)

    def results(self):
        self.wait()
        o = dict((k, self.out[k].cpu().numpy()[:int(np.prod(s))].reshape(s)) for k, s in self.shapes.items())
        return _job_dicts(self.p, self.outs, *[o[k] for k in _OUT])


def split_one(packed, out, split_iou, split_gap=0, motion='linear', first_new_id=None, n_classes=4):
    """One result, one setting; the input itself when the setting splits nothing (tracking/track.py with its default flags)."""
    iou = _per_class(split_iou, n_classes, float)
    gap = _per_class(split_gap, n_classes, int)
    if max(iou) <= 0 and max(gap) == 0:
        return out
    return split_tracks(packed, [out], [{'split_iou': iou, 'split_gap': gap, 'motion': motion, 'first_new_id': first_new_id}], n_classes)[0]
