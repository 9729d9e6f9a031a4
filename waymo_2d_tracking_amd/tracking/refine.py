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

SCORE_MODES = {'keep': 0, 'mean': 1}
_COLUMNS = ('x', 'y', 'w', 'h', 'score', 'category', 'local')


def _per_class(value, n_classes):
    v = [int(x) for x in value] if isinstance(value, (list, tuple, np.ndarray)) else [int(value)] * n_classes
    if len(v) == 1:
        v = v * n_classes
    if len(v) != n_classes:
        raise ValueError('max_gap / min_len need one value, or one per class (%d)' % n_classes)
    return v


def _dense_local(stream, ident, n_streams):
    """Number the distinct `ident` values of every stream from 0, by first appearance.  Returns (index per row, global trajectory
    number per row, count per stream)."""
    if stream.size == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(n_streams, np.int32)
    _, inv = np.unique(ident, return_inverse=True)
    base = int(inv.max()) + 1
    u, first, traj = np.unique(stream * base + inv, return_index=True, return_inverse=True)
    t_stream = u // base
    by_appearance = np.lexsort((first, t_stream))
    rank = np.empty(u.size, np.int64)
    rank[by_appearance] = np.arange(u.size)
    counts = np.bincount(t_stream, minlength=n_streams)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    local = rank - start[t_stream]
    return local[traj].astype(np.int32), traj.astype(np.int64), counts.astype(np.int32)


def _prepare(packed, outs, jobs, n_classes):
    """Everything wt_refine_tracks_* takes, as numpy arrays (include/waymotrack.h), after the checks that need names."""
    if len(outs) < 1:
        raise ValueError('at least one result is needed')
    sfo = np.ascontiguousarray(packed['stream_frame_offsets'], dtype=np.int64)
    n_streams, n_frames = int(sfo.size - 1), int(sfo[-1])
    cols = dict((n, []) for n in _COLUMNS)
    orders, oids, fros, n_traj, set_rows = [], [], [], [], [0]
    for r, out in enumerate(outs):
        frame = np.asarray(out['frame'], dtype=np.int64)
        if frame.size and (frame.min() < 0 or frame.max() >= n_frames):
            raise ValueError('result %d: frame outside the %d frame slots of the packed set' % (r, n_frames))
        order = np.arange(frame.size) if (np.diff(frame) >= 0).all() else np.argsort(frame, kind='stable')
        frame = frame[order]
        cat = np.asarray(out['category'], dtype=np.int32)[order]
        if cat.size and (cat.min() < 1 or cat.max() > n_classes):
            raise IndexError('category_id outside 1..%d (max_gap / min_len are indexed by category_id-1)' % n_classes)
        oid = np.asarray(out['object_id'])[order]
        stream = np.searchsorted(sfo, frame, side='right') - 1
        local, traj, counts = _dense_local(stream, oid, n_streams)
        if frame.size:                               # the same trajectory twice in one slot is not a tracking result
            key, first, count = np.unique(frame * (int(traj.max()) + 1) + traj, return_index=True, return_counts=True)
            if (count > 1).any():
                i = int(first[np.argmax(count > 1)])
                segment_id, camera_id = packed['stream_keys'][int(stream[i])]
                raise _lib.WaymoTrackError('wt_refine_tracks failed: WT_ERR_INVALID (result %d: object_id %s occurs twice in image %s/%d/%s)'
                                           % (r, oid[i], segment_id, int(packed['frame_ids'][int(frame[i])]), camera_id))
        bbox = np.asarray(out['bbox'], dtype=np.float64).reshape(-1, 4)[order]
        for i, n in enumerate(('x', 'y', 'w', 'h')):
            cols[n].append(bbox[:, i])
        cols['score'].append(np.asarray(out['score'], dtype=np.float64)[order])
        cols['category'].append(cat)
        cols['local'].append(local)
        orders.append(order)
        oids.append(oid)
        fros.append(np.searchsorted(frame, np.arange(n_frames + 1)).astype(np.int64))
        n_traj.append(counts)
        set_rows.append(set_rows[-1] + int(frame.size))
    p = dict((n, np.ascontiguousarray(np.concatenate(cols[n]), dtype=np.int32 if n in ('category', 'local') else np.float64)) for n in _COLUMNS)
    p.update(stream_frame_offsets=sfo, n_streams=n_streams, n_frames=n_frames, R=len(outs), orders=orders, object_ids=oids,
             set_row_offsets=np.asarray(set_rows, dtype=np.int64), frame_row_offsets=np.ascontiguousarray(np.stack(fros), dtype=np.int64),
             n_traj=np.ascontiguousarray(np.stack(n_traj), dtype=np.int32).reshape(len(outs), n_streams), n_classes=int(n_classes))
    p['traj_offsets'] = np.concatenate([[0], np.cumsum(p['n_traj'].reshape(-1).astype(np.int64))]).astype(np.int64)
    J = len(jobs)
    p['J'] = J
    p['job_result'] = np.asarray([int(j.get('result', 0)) for j in jobs], dtype=np.int32).reshape(J)
    if J and (p['job_result'].min() < 0 or p['job_result'].max() >= len(outs)):
        raise ValueError('a job names a result outside 0..%d' % (len(outs) - 1))
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


def _leading_args(p, a, ptr, host):
    """The layout arguments every wt_refine_tracks_* call begins with.  a: the columns by name (numpy arrays or tensors)."""
    args = [C.c_int64(p['n_frames']), C.c_int32(p['n_streams']), ptr(a['stream_frame_offsets']), C.c_int32(p['R'])]
    if not host:
        args.append(C.c_int64(int(p['set_row_offsets'][-1])))
    return args + [ptr(a['set_row_offsets']), ptr(a['frame_row_offsets'])]


def _job_args(p, a, ptr, with_mode=True):
    return ([C.c_int32(p['J']), ptr(a['job_result']), ptr(a['job_max_gap']), ptr(a['job_min_len'])] +
            ([ptr(a['job_score_mode'])] if with_mode else []) + [C.c_int32(p['n_classes'])])


def _host_call(p, out_cap, outputs, job_rows):
    """wt_refine_tracks_host on _prepare() output; outputs: frame, category, bbox, score, local, source, frame_row_offsets."""
    ptr = _lib.ptr
    return _lib.lib().wt_refine_tracks_host(
        *_leading_args(p, p, ptr, True), *[ptr(p[n]) for n in _COLUMNS], ptr(p['n_traj']), *_job_args(p, p, ptr),
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


class DeviceRefine(object):
    """The same refinement with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues
    wt_refine_tracks_plan_dev on the current torch stream and returns at once; ``results()`` reads the planned size, lets
    wt_refine_tracks_emit_dev write the rows and reads them back.  After results(), ``self.out`` holds the output tensors and
    ``self.job_row_offsets`` / ``self.out['frame_row_offsets']`` the offsets wt_mot_*_dev take."""
    name = 'wt_refine_tracks_plan_dev'

    def __init__(self, packed, outs, jobs, n_classes=4):
        import torch
        self.torch = torch
        self.lib = _lib.lib()
        self.p = p = _prepare(packed, outs, jobs, n_classes)
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.status = self.zeros(1, torch.int32)
        names = _COLUMNS + ('stream_frame_offsets', 'set_row_offsets', 'frame_row_offsets', 'traj_offsets', 'job_result', 'job_max_gap',
                            'job_min_len', 'job_score_mode')
        self.t = dict((n, self.up(p[n])) for n in names)
        self.n_rows = int(p['set_row_offsets'][-1])
        self.n_traj_total = int(p['traj_offsets'][-1])
        self.max_traj = int(p['n_traj'].max()) if p['n_traj'].size else 0
        self.job_row_offsets = self.zeros(p['J'] + 1, torch.int64)
        self.ws_bytes = int(self.lib.wt_refine_tracks_workspace(C.c_int32(p['J']), C.c_int32(p['n_streams']), C.c_int64(self.n_rows),
                                                                C.c_int64(self.n_traj_total), C.c_int64(self.max_traj)))
        if not self.ws_bytes:
            _lib.check(4, 'wt_refine_tracks_workspace')
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)
        self.out = None

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a))
        return t.to(self.device) if a.size else self.zeros(1, t.dtype)

    def zeros(self, shape, dtype):
        return self.torch.zeros(shape, dtype=dtype, device=self.device)

    def d(self, t):
        return C.c_void_p(t.data_ptr())

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def _traj_args(self):
        return [self.d(self.t['traj_offsets']), C.c_int64(self.n_traj_total), C.c_int64(self.max_traj)]

    def launch(self):
        p, t, d = self.p, self.t, self.d
        rc = self.lib.wt_refine_tracks_plan_dev(
            *_leading_args(p, t, d, False), d(t['score']), d(t['category']), d(t['local']), *self._traj_args(),
            *_job_args(p, t, d, with_mode=False), d(self.job_row_offsets), d(self.status), d(self.ws), C.c_size_t(self.ws_bytes), self._stream())
        _lib.check(rc, self.name)

    def wait(self, name):
        self.torch.cuda.current_stream().synchronize()
        st = int(self.status.item())
        if st:
            raise _lib.WaymoTrackError('%s failed: %s (status reported by the kernel)' % (name, _lib._STATUS.get(st, st)))

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
            *_leading_args(p, t, d, False), *[d(t[n_]) for n_ in _COLUMNS], *self._traj_args(), *_job_args(p, t, d),
            d(self.job_row_offsets), C.c_int64(n), d(o['frame']), d(o['category']), d(o['bbox']), d(o['score']), d(o['local']), d(o['source']),
            d(o['frame_row_offsets']), d(self.status), d(self.ws), C.c_size_t(self.ws_bytes), self._stream())
        _lib.check(rc, 'wt_refine_tracks_emit_dev')

    def results(self):
        if self.out is None:
            self.emit()
        self.wait('wt_refine_tracks_emit_dev')
        o = dict((k, v.cpu().numpy()) for k, v in self.out.items())
        return _job_dicts(self.p, self.job_row_offsets.cpu().numpy(), o['frame'], o['category'], o['bbox'], o['score'], o['local'], o['source'],
                          o['frame_row_offsets'])


def refine_one(packed, out, max_gap, min_len, score_mode='keep', n_classes=4):
    """One result, one setting; the input itself when the setting changes nothing (tracking/track.py with its default flags)."""
    gap, length = _per_class(max_gap, n_classes), _per_class(min_len, n_classes)
    if max(gap) == 0 and max(length) == 1 and score_mode == 'keep':
        return out
    return refine_tracks(packed, [out], [{'max_gap': gap, 'min_len': length, 'score_mode': score_mode}], n_classes)[0]
