"""Refine tracking results on the GPU: drop short trajectories, fill short gaps by linear interpolation, mean track score.

    outs = refine_tracks(packed, [out], [{'max_gap': 1, 'min_len': 2}, {'max_gap': [2, 2, 0, 1], 'score_mode': 'mean'}])

DESIGN.md section 20 has the definition.  A tracker that keeps a track alive over a missed frame (``--max-age`` above 1) writes no
row for that frame: every such hole is a false negative, and a track seen in one or two frames is usually a false positive.
Every (job, segment, camera) is an independent problem and one wavefront of the HIP kernels behind ``wt_refine_tracks_*``
(include/waymotrack.h); R results are refined under J settings in one call without being copied, which is what lets the sweep of
tracking/evaluate.py try every (gap, length) pair on one tracked result.  No arithmetic of the refinement runs on the host;
without a GPU the calls fail.
"""
import ctypes as C

import numpy as np

from .. import _lib
from . import _trackset as TS
from ._trackset import COLUMNS as _COLUMNS

SCORE_MODES = {'keep': 0, 'mean': 1}
_JOB = ('job_result', 'job_max_gap', 'job_min_len', 'job_score_mode')


def _per_class(value, n_classes):
    return TS.per_class(value, n_classes, int, 'max_gap / min_len')


def _prepare(packed, outs, jobs, n_classes):
    """Everything wt_refine_tracks_* takes, as numpy arrays (include/waymotrack.h), after the checks that need names."""
    return _job_columns(TS.prepare(packed, outs, jobs, n_classes, 'refine'), jobs, n_classes)


def _job_columns(p, jobs, n_classes):
    """the job parameters of wt_refine_tracks_*, checked, added to the layout `p`"""
    J = p['J']
    p['job_max_gap'] = np.asarray([_per_class(j.get('max_gap', 0), n_classes) for j in jobs], dtype=np.int32).reshape(J, n_classes)
    p['job_min_len'] = np.asarray([_per_class(j.get('min_len', 1), n_classes) for j in jobs], dtype=np.int32).reshape(J, n_classes)
    if J and (p['job_max_gap'].min() < 0 or p['job_min_len'].min() < 1):
        raise ValueError('max_gap must be >= 0 and min_len >= 1')
    p['job_score_mode'] = np.asarray([SCORE_MODES[j.get('score_mode', 'keep')] for j in jobs], dtype=np.int32).reshape(J)
    return p


def _job_dicts(p, job_rows, frame, category, bbox, score, local, source, frame_row_offsets):
    """The J results as dicts of the form utils.track_packed returns, plus 'source' (the caller's row index of an observed row,
    -1 - the caller's row index of the gap's later observation for a filled one), 'local' and 'frame_row_offsets'."""
    results = []
    for j in range(p['J']):
        lo, hi = int(job_rows[j]), int(job_rows[j + 1])
        r = int(p['job_result'][j])
        src = source[lo:hi]
        row = np.where(src >= 0, src, -1 - src)
        caller = p['orders'][r][row] if row.size else row
        results.append(dict(frame=frame[lo:hi].copy(), category=category[lo:hi].copy(), bbox=bbox[lo:hi].copy(), score=score[lo:hi].copy(),
                            object_id=p['object_ids'][r][row] if row.size else p['object_ids'][r][:0],
                            source=np.where(src >= 0, caller, -1 - caller).astype(np.int64), local=local[lo:hi].copy(),
                            frame_row_offsets=frame_row_offsets[j].copy()))
    return results


def _host_call(p, out_cap, outputs, job_rows):
    """wt_refine_tracks_host on _prepare() output; outputs: frame, category, bbox, score, local, source, frame_row_offsets."""
    ptr = _lib.ptr
    return _lib.lib().wt_refine_tracks_host(
        *TS.leading_args(p, p, ptr, True, _COLUMNS), ptr(p['n_traj']), *TS.job_args(p, p, ptr, _JOB),
        C.c_int64(out_cap), *[ptr(x) for x in outputs], ptr(job_rows))


def refine_tracks(packed, outs, jobs, n_classes=4):
    """Refine R tracker outputs (dicts as utils.track_packed returns them, over the frame slots of `packed`) under J jobs in ONE
    wt_refine_tracks_host call (after its sizing call).  A job is a dict: 'result' (index into outs, default 0), 'max_gap' and
    'min_len' (one int, or one per class; defaults 0 and 1) and 'score_mode' ('keep' or 'mean').  Returns J dicts of the form
    track_packed returns, plus 'source'; utils.format_tracks, NativeDetFile.write_tracks and evaluate.tracks_from_packed take them
    as they are.  Rows that are not sorted by frame are stably sorted first."""
    p = _prepare(packed, outs, jobs, n_classes)
    J, nf = p['J'], p['n_frames'] + 1
    job_rows = np.zeros(J + 1, np.int64)
    _lib.check(_host_call(p, 0, [None] * 7, job_rows), 'wt_refine_tracks_host')       # the sizing call
    n = int(job_rows[-1])
    o = [np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int32), np.zeros((n + 1, 4), np.float64), np.zeros(n + 1, np.float64),
         np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int64), np.zeros((max(J, 1), nf), np.int64)]
    _lib.check(_host_call(p, n + 1, o, job_rows), 'wt_refine_tracks_host')
    return _job_dicts(p, job_rows, o[0], o[1], o[2], o[3], o[4], o[5], o[6])


class DeviceRefine(TS.DeviceStage):
    """The same refinement with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues
    wt_refine_tracks_plan_dev on the current torch stream and returns at once; ``results()`` reads the planned size, lets
    wt_refine_tracks_emit_dev write the rows and reads them back.  After results(), ``self.out`` holds the output tensors and
    ``self.job_row_offsets`` / ``self.out['frame_row_offsets']`` the offsets wt_mot_*_dev take."""
    stage = 'refine'
    name = 'wt_refine_tracks_plan_dev'

    def __init__(self, packed, outs, jobs, n_classes=4):
        """outs: the results as dicts, or a _trackset.DeviceTrackSet of results that are in HBM already (its rows are not copied)."""
        if isinstance(outs, TS.DeviceTrackSet):
            TS.DeviceStage.__init__(self, _job_columns(outs.job_params(jobs), jobs, n_classes), _COLUMNS + _JOB, trackset=outs)
        else:
            TS.DeviceStage.__init__(self, _prepare(packed, outs, jobs, n_classes), _COLUMNS + _JOB)
        self.job_row_offsets = self.zeros(self.p['J'] + 1, self.torch.int64)
        self.out = None

    def launch(self):
        p, t, d = self.p, self.t, self.d
        rc = self.lib.wt_refine_tracks_plan_dev(
            *TS.leading_args(p, t, d, False, ('score', 'category', 'local')), *self.traj_args(), *TS.job_args(p, t, d, _JOB[:3]),
            d(self.job_row_offsets), *self.tail_args())
        _lib.check(rc, self.name)

    def emit(self, out_cap=None):
        """Write the planned rows into tensors of out_cap rows (default: the planned size)."""
        torch, p, t, d = self.torch, self.p, self.t, self.d
        self.wait(self.name)
        n = int(self.job_row_offsets[-1].item()) if out_cap is None else int(out_cap)
        if self.out is None or self.out['frame'].numel() != n + 1:       # a repeated emit of the same plan writes the same buffers
            self.out = dict(frame=self.zeros(n + 1, torch.int64), category=self.zeros(n + 1, torch.int32), bbox=self.zeros((n + 1, 4), torch.float64),
                        score=self.zeros(n + 1, torch.float64), local=self.zeros(n + 1, torch.int32), source=self.zeros(n + 1, torch.int64),
                        frame_row_offsets=self.zeros((max(p['J'], 1), p['n_frames'] + 1), torch.int64))
        o = self.out
        rc = self.lib.wt_refine_tracks_emit_dev(
            *TS.leading_args(p, t, d, False, _COLUMNS), *self.traj_args(), *TS.job_args(p, t, d, _JOB),
            d(self.job_row_offsets), C.c_int64(n), d(o['frame']), d(o['category']), d(o['bbox']), d(o['score']), d(o['local']), d(o['source']),
            d(o['frame_row_offsets']), *self.tail_args())
        _lib.check(rc, 'wt_refine_tracks_emit_dev')

    def results(self):
        if self.out is None:
            self.emit()
        self.wait('wt_refine_tracks_emit_dev')
        o = dict((k, v.cpu().numpy()) for k, v in self.out.items())
        p = self.p if self.trackset is None else dict(self.p, **self.trackset.host_rows())
        return _job_dicts(p, self.job_row_offsets.cpu().numpy(), o['frame'], o['category'], o['bbox'], o['score'], o['local'], o['source'],
                          o['frame_row_offsets'])


def refine_one(packed, out, max_gap, min_len, score_mode='keep', n_classes=4):
    """One result, one setting; the input itself when the setting changes nothing (tracking/track.py with its default flags)."""
    gap, length = _per_class(max_gap, n_classes), _per_class(min_len, n_classes)
    if max(gap) == 0 and max(length) == 1 and score_mode == 'keep':
        return out
    return refine_tracks(packed, [out], [{'max_gap': gap, 'min_len': length, 'score_mode': score_mode}], n_classes)[0]
