"""Stitch broken tracks on the GPU: link tracklets of one stream and class across gaps (the second association pass).

    outs = stitch_tracks(packed, [out], [{'max_link': 3, 'link_iou': 0.3}, {'max_link': [5, 3, 0, 3], 'motion': 'linear'}])

DESIGN.md section 21 has the definition.  A tracker drops a track that misses more than ``--max-age`` frames; when the object comes
back it is born under a new id - an identity switch, a split trajectory, lost association.  A tracklet that ends is linked to one
that begins up to max_link frame slots later when its (held or linearly extrapolated) last box overlaps the other's first box by at
least link_iou; linked pieces take the id of the earliest one.  Every (job, segment, camera) is an independent problem and one
wavefront of the HIP kernels behind ``wt_stitch_tracks_*`` (include/waymotrack.h); R results are stitched under J settings in one
call.  No arithmetic of the stitching runs on the host; without a GPU the calls fail.
"""
import numpy as np

from .. import _lib
from . import _trackset as TS

MOTIONS = {'hold': 0, 'linear': 1}
_COLUMNS = ('x', 'y', 'w', 'h', 'category', 'local')
_JOB = ('job_result', 'job_max_link', 'job_link_iou', 'job_motion')
_OUT = ('pred', 'root', 'affinity', 'row_root', 'links')


def _per_class(value, n_classes, kind):
    return TS.per_class(value, n_classes, kind, 'max_link / link_iou')


def _prepare(packed, outs, jobs, n_classes):
    """Everything wt_stitch_tracks_* takes, as numpy arrays (include/waymotrack.h): the shared layout, the jobs of the stitching,
    and per trajectory the object id it has in the caller's rows."""
    p = TS.prepare(packed, outs, jobs, n_classes, 'stitch')
    J = p['J']
    p['job_max_link'] = np.asarray([_per_class(j.get('max_link', 0), n_classes, int) for j in jobs], dtype=np.int32).reshape(J, n_classes)
    p['job_link_iou'] = np.asarray([_per_class(j.get('link_iou', 0.3), n_classes, float) for j in jobs], dtype=np.float64).reshape(J, n_classes)
    if J and (p['job_max_link'].min() < 0 or np.isnan(p['job_link_iou']).any()):
        raise ValueError('max_link must be >= 0 and link_iou must not be NaN')
    p['job_motion'] = np.asarray([MOTIONS[j.get('motion', 'hold')] for j in jobs], dtype=np.int32).reshape(J)
    p['row_stream_base'], p['traj_ids'] = TS.traj_ids(p, outs)
    return p


def _job_dicts(p, outs, pred, root, affinity, row_root, n_links):
    """The J results as dicts of the form utils.track_packed returns - the caller's rows in the caller's order, object_id replaced
    by the root's - plus 'links' (from id, to id, gap in slots, affinity per accepted link), 'n_links' per stream, and the
    per-trajectory 'pred', 'root', 'affinity' and per-row 'row_root' of the call."""
    S = p['n_streams']
    results = []
    for j in range(p['J']):
        r = int(p['job_result'][j])
        lo, hi = int(p['set_row_offsets'][r]), int(p['set_row_offsets'][r + 1])
        t0, t1 = int(p['traj_offsets'][r * S]), int(p['traj_offsets'][(r + 1) * S])
        order, ids = p['orders'][r], p['traj_ids'][r]
        out = dict((k, np.asarray(v)) for k, v in outs[r].items())
        rr = row_root[j, lo:hi]
        oid = np.asarray(out['object_id']).copy()
        oid[order] = ids[p['row_stream_base'][r] + rr - t0] if rr.size else ids[:0]
        out['object_id'] = oid
        caller_root = np.zeros(hi - lo, np.int32)
        caller_root[order] = rr
        pj, aj = pred[j, t0:t1], affinity[j, t0:t1]
        heads = np.nonzero(pj >= 0)[0]
        stream_base = p['traj_offsets'][r * S:(r + 1) * S] - t0
        base = stream_base[np.searchsorted(stream_base, heads, side='right') - 1] if heads.size else heads
        # gap: first slot of the head - last slot of the tail, read off the rows
        frame = np.asarray(outs[r]['frame'], dtype=np.int64)[order]
        flat = p['row_stream_base'][r] + p['local'][lo:hi] - t0
        first = np.full(t1 - t0, np.iinfo(np.int64).max, np.int64)
        last = np.full(t1 - t0, -1, np.int64)
        np.minimum.at(first, flat, frame)
        np.maximum.at(last, flat, frame)
        tails = base + pj[heads]
        py = lambda v: v.item() if isinstance(v, np.generic) else v
        out['links'] = [(py(ids[t]), py(ids[h]), int(first[h] - last[t]), float(aj[h])) for t, h in zip(tails, heads)]
        out.update(n_links=n_links[j].copy(), pred=pj.copy(), root=root[j, t0:t1].copy(), affinity=aj.copy(), row_root=caller_root,
                   traj_offsets=(p['traj_offsets'][r * S:(r + 1) * S + 1] - t0).astype(np.int64))
        results.append(out)
    return results


def _host_call(p, outputs):
    """wt_stitch_tracks_host on _prepare() output; outputs: pred, root, affinity, row_root, links, each exactly (J, n) C-contiguous."""
    ptr = _lib.ptr
    return _lib.lib().wt_stitch_tracks_host(*TS.leading_args(p, p, ptr, True, _COLUMNS), ptr(p['n_traj']), *TS.job_args(p, p, ptr, _JOB),
                                            *[ptr(x) for x in outputs])


def stitch_tracks(packed, outs, jobs, n_classes=4):
    """Stitch R tracker outputs (dicts as utils.track_packed returns them, over the frame slots of `packed`) under J jobs in ONE
    wt_stitch_tracks_host call.  A job is a dict: 'result' (index into outs, default 0), 'max_link' (frame slots, one int or one per
    class, default 0 = never), 'link_iou' (one float or one per class, default 0.3) and 'motion' ('hold' or 'linear').  Returns J
    dicts of the form track_packed returns, rows in the caller's order, only object_id changed, plus 'links'; utils.format_tracks,
    NativeDetFile.write_tracks, refine.refine_tracks and evaluate.tracks_from_packed take them as they are."""
    p = _prepare(packed, outs, jobs, n_classes)
    J, nt, nr, S = p['J'], p['n_traj_total'], p['n_rows'], p['n_streams']
    o = [np.zeros((J, nt), np.int32), np.zeros((J, nt), np.int32), np.zeros((J, nt), np.float64), np.zeros((J, nr), np.int32),
         np.zeros((J, S), np.int64)]
    _lib.check(_host_call(p, o), 'wt_stitch_tracks_host')
    return _job_dicts(p, outs, *o)


class DeviceStitch(TS.DeviceStage):
    """The same stitching with everything resident in HBM (torch tensors own the memory): ``launch()`` enqueues
    wt_stitch_tracks_dev on the current torch stream and returns at once - the output sizes are known up front, nothing is read
    back in between; ``results()`` synchronises and reads the outputs.  ``self.out`` holds the output tensors."""
    stage = 'stitch'
    name = 'wt_stitch_tracks_dev'

    def __init__(self, packed, outs, jobs, n_classes=4, workspace_bytes=None):
        TS.DeviceStage.__init__(self, _prepare(packed, outs, jobs, n_classes), _COLUMNS + _JOB, workspace_bytes)
        torch, p = self.torch, self.p
        self.outs = outs
        J, nt, nr, S = p['J'], p['n_traj_total'], p['n_rows'], p['n_streams']
        self.shapes = dict(pred=(J, nt), root=(J, nt), affinity=(J, nt), row_root=(J, nr), links=(J, S))
        dtypes = dict(pred=torch.int32, root=torch.int32, affinity=torch.float64, row_root=torch.int32, links=torch.int64)
        self.out = dict((k, self.zeros(max(1, s[0] * s[1]), dtypes[k])) for k, s in self.shapes.items())

    def launch(self):
        p, t, d = self.p, self.t, self.d
        rc = self.lib.wt_stitch_tracks_dev(*TS.leading_args(p, t, d, False, _COLUMNS), *self.traj_args(), *TS.job_args(p, t, d, _JOB),
                                           *[d(self.out[k]) for k in _OUT], *self.tail_args())
        _lib.check(rc, self.name)

    def results(self):
        self.wait()
        o = dict((k, self.out[k].cpu().numpy()[:s[0] * s[1]].reshape(s)) for k, s in self.shapes.items())
        return _job_dicts(self.p, self.outs, *[o[k] for k in _OUT])


def stitch_one(packed, out, max_link, link_iou=0.3, motion='hold', n_classes=4):
    """One result, one setting; the input itself when the setting links nothing (tracking/track.py with its default flags)."""
    link = _per_class(max_link, n_classes, int)
    if max(link) == 0:
        return out
    return stitch_tracks(packed, [out], [{'max_link': link, 'link_iou': _per_class(link_iou, n_classes, float), 'motion': motion}], n_classes)[0]
