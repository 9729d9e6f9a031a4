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
from . import refine as R

_COLUMNS = ('x', 'y', 'w', 'h', 'score', 'category', 'local')
_JOB = ('job_result', 'job_min_frames', 'job_dup_iou', 'job_dup_frac')
_OUT = ('keep', 'by', 'match', 'row_keep', 'dropped')


def _per_class(value, n_classes, kind):
    v = [kind(x) for x in value] if isinstance(value, (list, tuple, np.ndarray)) else [kind(value)] * n_classes
    if len(v) == 1:
        v = v * n_classes
    if len(v) != n_classes:
        raise ValueError('min_frames / dup_iou / dup_frac need one value, or one per class (%d)' % n_classes)
    return v


def _prepare(packed, outs, jobs, n_classes):
    """Everything wt_dedup_tracks_* takes, as numpy arrays (include/waymotrack.h): the layout refinement prepares, the jobs of the
    deduplication, and per trajectory the object id it has in the caller's rows."""
    try:
        p = R._prepare(packed, outs, [], n_classes)
    except _lib.WaymoTrackError as e:                # the duplicate in a slot, named with its image
        raise _lib.WaymoTrackError(str(e).replace('wt_refine_tracks failed', 'wt_dedup_tracks failed'))
    J = len(jobs)
    p['J'] = J
    p['job_result'] = np.asarray([int(j.get('result', 0)) for j in jobs], dtype=np.int32).reshape(J)
    if J and (p['job_result'].min() < 0 or p['job_result'].max() >= len(outs)):
        raise ValueError('a job names a result outside 0..%d' % (len(outs) - 1))
    p['job_min_frames'] = np.asarray([_per_class(j.get('min_frames', 0), n_classes, int) for j in jobs], dtype=np.int32).reshape(J, n_classes)
    p['job_dup_iou'] = np.asarray([_per_class(j.get('dup_iou', 0.7), n_classes, float) for j in jobs], dtype=np.float64).reshape(J, n_classes)
    p['job_dup_frac'] = np.asarray([_per_class(j.get('dup_frac', 0.5), n_classes, float) for j in jobs], dtype=np.float64).reshape(J, n_classes)
    if J and p['job_min_frames'].min() < 0:
        raise ValueError('min_frames must be >= 0')
    if np.isnan(p['job_dup_iou']).any():
        raise ValueError('dup_iou must not be NaN')
    if not ((p['job_dup_frac'] >= 0) & (p['job_dup_frac'] <= 1)).all():
        raise ValueError('dup_frac must be in 0..1')
    p['n_rows'] = int(p['set_row_offsets'][-1])
    p['n_traj_total'] = int(p['traj_offsets'][-1])
    # per row its trajectory's place in the (J, n_traj_total) outputs, per trajectory its object id
    sfo, S = p['stream_frame_offsets'], p['n_streams']
    ids = []
    for r in range(p['R']):
        lo, hi = int(p['set_row_offsets'][r]), int(p['set_row_offsets'][r + 1])
        frame = np.asarray(outs[r]['frame'], dtype=np.int64)[p['orders'][r]]
        stream = np.searchsorted(sfo, frame, side='right') - 1
        base = p['traj_offsets'][r * S + stream] if frame.size else np.zeros(0, np.int64)
        t0, t1 = int(p['traj_offsets'][r * S]), int(p['traj_offsets'][(r + 1) * S])
        oid = p['object_ids'][r]
        of_traj = np.zeros(t1 - t0, dtype=oid.dtype)
        of_traj[base + p['local'][lo:hi] - t0] = oid
        ids.append(of_traj)
    p['traj_ids'] = ids
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


def _leading_args(p, a, ptr, host):
    args = [C.c_int64(p['n_frames']), C.c_int32(p['n_streams']), ptr(a['stream_frame_offsets']), C.c_int32(p['R'])]
    if not host:
        args.append(C.c_int64(p['n_rows']))
    return args + [ptr(a['set_row_offsets']), ptr(a['frame_row_offsets'])] + [ptr(a[n]) for n in _COLUMNS]


def _job_args(p, a, ptr):
    return [C.c_int32(p['J'])] + [ptr(a[n]) for n in _JOB] + [C.c_int32(p['n_classes'])]


def _host_call(p, outputs):
    """wt_dedup_tracks_host on _prepare() output; outputs: keep, by, match, row_keep, dropped, each exactly (J, n) C-contiguous."""
    ptr = _lib.ptr
    return _lib.lib().wt_dedup_tracks_host(*_leading_args(p, p, ptr, True), ptr(p['n_traj']), *_job_args(p, p, ptr), *[ptr(x) for x in outputs])


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


class DeviceDedup(object):
    """The same deduplication with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues
    wt_dedup_tracks_dev on the current torch stream and returns at once - the output sizes are known up front, nothing is read
    back in between; ``results()`` synchronises and reads the outputs.  ``self.out`` holds the output tensors."""
    name = 'wt_dedup_tracks_dev'

    def __init__(self, packed, outs, jobs, n_classes=4, workspace_bytes=None):
        import torch
        self.torch = torch
        self.lib = _lib.lib()
        self.outs = outs
        self.p = p = _prepare(packed, outs, jobs, n_classes)
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.status = self.zeros(1, torch.int32)
        names = _COLUMNS + _JOB + ('stream_frame_offsets', 'set_row_offsets', 'frame_row_offsets', 'traj_offsets')
        self.t = dict((n, self.up(p[n])) for n in names)
        self.max_traj = int(p['n_traj'].max()) if p['n_traj'].size else 0
        J, nt, nr, S = p['J'], p['n_traj_total'], p['n_rows'], p['n_streams']
        self.shapes = dict(keep=(J, nt), by=(J, nt), match=(J, nt), row_keep=(J, nr), dropped=(J, S))
        self.out = dict((k, self.zeros(max(1, s[0] * s[1]), torch.int64 if k == 'dropped' else torch.int32)) for k, s in self.shapes.items())
        self.ws_bytes = int(self.lib.wt_dedup_tracks_workspace(C.c_int32(J), C.c_int32(S), C.c_int64(nr), C.c_int64(nt), C.c_int64(self.max_traj)))
        if not self.ws_bytes:
            _lib.check(4, 'wt_dedup_tracks_workspace')
        self.ws = torch.empty(self.ws_bytes if workspace_bytes is None else int(workspace_bytes), dtype=torch.uint8, device=self.device)

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a))
        return t.to(self.device) if a.size else self.zeros(1, t.dtype)

    def zeros(self, shape, dtype):
        return self.torch.zeros(shape, dtype=dtype, device=self.device)

    def d(self, t):
        return C.c_void_p(t.data_ptr())

    def launch(self):
        p, t, d, o = self.p, self.t, self.d, self.out
        rc = self.lib.wt_dedup_tracks_dev(
            *_leading_args(p, t, d, False), d(t['traj_offsets']), C.c_int64(p['n_traj_total']), C.c_int64(self.max_traj), *_job_args(p, t, d),
            *[d(o[k]) for k in _OUT], d(self.status), d(self.ws), C.c_size_t(int(self.ws.numel())),
            C.c_void_p(self.torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, self.name)

    def wait(self):
        self.torch.cuda.current_stream().synchronize()
        st = int(self.status.item())
        if st:
            raise _lib.WaymoTrackError('%s failed: %s (status reported by the kernel)' % (self.name, _lib._STATUS.get(st, st)))

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
