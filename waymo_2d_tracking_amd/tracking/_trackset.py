"""What the seven track post-passes (refine.py, stitch.py, smooth.py, dedup.py, split.py, xclass.py, xlink.py) share: the layout every ``wt_<stage>_tracks_*`` call
takes - R results over the frame slots of `packed`, CSR offsets, the box / score / category columns, a dense per-stream trajectory
index per row, J jobs that each name a result (include/waymotrack.h; DESIGN.md section 20, "The shared layer") - the argument
lists built from it, and the device-resident form of a stage.  The layout is built on the host by prepare(), or on the GPU, for
tracker results that are in HBM already, by DeviceTrackSet (wt_tracks_layout_*)."""
import ctypes as C

import numpy as np

from .. import _lib

COLUMNS = ('x', 'y', 'w', 'h', 'score', 'category', 'local')
OFFSETS = ('stream_frame_offsets', 'set_row_offsets', 'frame_row_offsets', 'traj_offsets')


def per_class(value, n_classes, kind, names):
    v = [kind(x) for x in value] if isinstance(value, (list, tuple, np.ndarray)) else [kind(value)] * n_classes
    if len(v) == 1:
        v = v * n_classes
    if len(v) != n_classes:
        raise ValueError('%s need one value, or one per class (%d)' % (names, n_classes))
    return v


def dense_local(stream, ident, n_streams):
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


def prepare(packed, outs, jobs, n_classes, stage):
    """The layout of R results and the result each of the J jobs names, as numpy arrays, after the checks that need names;
    `stage` ('refine', ...) names the entry point in the one error text."""
    if len(outs) < 1:
        raise ValueError('at least one result is needed')
    sfo = np.ascontiguousarray(packed['stream_frame_offsets'], dtype=np.int64)
    n_streams, n_frames = int(sfo.size - 1), int(sfo[-1])
    cols = dict((n, []) for n in COLUMNS)
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
        local, traj, counts = dense_local(stream, oid, n_streams)
        if frame.size:                               # the same trajectory twice in one slot is not a tracking result
            key, first, count = np.unique(frame * (int(traj.max()) + 1) + traj, return_index=True, return_counts=True)
            if (count > 1).any():
                i = int(first[np.argmax(count > 1)])
                segment_id, camera_id = packed['stream_keys'][int(stream[i])]
                raise _lib.WaymoTrackError('wt_%s_tracks failed: WT_ERR_INVALID (result %d: object_id %s occurs twice in image %s/%d/%s)'
                                           % (stage, r, oid[i], segment_id, int(packed['frame_ids'][int(frame[i])]), camera_id))
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
    p = dict((n, np.ascontiguousarray(np.concatenate(cols[n]), dtype=np.int32 if n in ('category', 'local') else np.float64)) for n in COLUMNS)
    p.update(stream_frame_offsets=sfo, n_streams=n_streams, n_frames=n_frames, R=len(outs), orders=orders, object_ids=oids,
             set_row_offsets=np.asarray(set_rows, dtype=np.int64), frame_row_offsets=np.ascontiguousarray(np.stack(fros), dtype=np.int64),
             n_traj=np.ascontiguousarray(np.stack(n_traj), dtype=np.int32).reshape(len(outs), n_streams), n_classes=int(n_classes))
    p['traj_offsets'] = np.concatenate([[0], np.cumsum(p['n_traj'].reshape(-1).astype(np.int64))]).astype(np.int64)
    p.update(n_rows=set_rows[-1], n_traj_total=int(p['traj_offsets'][-1]), max_traj=int(p['n_traj'].max()) if p['n_traj'].size else 0)
    J = p['J'] = len(jobs)
    p['job_result'] = np.asarray([int(j.get('result', 0)) for j in jobs], dtype=np.int32).reshape(J)
    if J and (p['job_result'].min() < 0 or p['job_result'].max() >= len(outs)):
        raise ValueError('a job names a result outside 0..%d' % (len(outs) - 1))
    return p


def traj_ids(p, outs):
    """Per result: per row the first place of its stream's trajectories in the (J, n_traj_total) outputs, and per trajectory the
    object id it has in the caller's rows."""
    sfo, S = p['stream_frame_offsets'], p['n_streams']
    bases, ids = [], []
    for r in range(p['R']):
        lo, hi = int(p['set_row_offsets'][r]), int(p['set_row_offsets'][r + 1])
        frame = np.asarray(outs[r]['frame'], dtype=np.int64)[p['orders'][r]]
        stream = np.searchsorted(sfo, frame, side='right') - 1
        base = p['traj_offsets'][r * S + stream] if frame.size else np.zeros(0, np.int64)
        t0, t1 = int(p['traj_offsets'][r * S]), int(p['traj_offsets'][(r + 1) * S])
        oid = p['object_ids'][r]
        of_traj = np.zeros(t1 - t0, dtype=oid.dtype)
        of_traj[base + p['local'][lo:hi] - t0] = oid
        bases.append(base)
        ids.append(of_traj)
    return bases, ids


def leading_args(p, a, ptr, host, columns=()):
    """The layout arguments every wt_<stage>_tracks_* call begins with, then `columns`.  a: the arrays by name (numpy arrays or
    tensors); the device forms also take the row count."""
    args = [C.c_int64(p['n_frames']), C.c_int32(p['n_streams']), ptr(a['stream_frame_offsets']), C.c_int32(p['R'])]
    if not host:
        args.append(C.c_int64(p['n_rows']))
    return args + [ptr(a['set_row_offsets']), ptr(a['frame_row_offsets'])] + [ptr(a[n]) for n in columns]


def job_args(p, a, ptr, names, counts=()):
    """J, the job arrays `names`, then the p[...] of `counts` and the class count"""
    return [C.c_int32(p['J'])] + [ptr(a[n]) for n in names] + [C.c_int32(p[n]) for n in counts + ('n_classes',)]


class DeviceStage(object):
    """A stage with everything resident in HBM (torch tensors own the memory).  A subclass sets `stage`, makes `p`, names the
    arrays its calls take and allocates its outputs."""
    stage = None

    def __init__(self, p, names, workspace_bytes=None, trackset=None):
        """trackset: a DeviceTrackSet that `p` came from (its job_params()); its tensors are the layout, and only the stage's own
        arrays are uploaded."""
        import torch
        self.torch = torch
        self.lib = _lib.lib()
        self.p = p
        self.trackset = trackset
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.status = self.zeros(1, torch.int32)
        if trackset is None:
            self.t = dict((n, self.up(p[n])) for n in tuple(names) + OFFSETS)
        else:
            self.t = dict((n, trackset.t[n] if n in trackset.t else self.up(p[n])) for n in tuple(names) + OFFSETS)
        self.n_rows, self.n_traj_total, self.max_traj = p['n_rows'], p['n_traj_total'], p['max_traj']
        sizer = 'wt_%s_tracks_workspace' % self.stage
        self.ws_bytes = int(getattr(self.lib, sizer)(C.c_int32(p['J']), C.c_int32(p['n_streams']), C.c_int64(self.n_rows),
                                                     C.c_int64(self.n_traj_total), C.c_int64(self.max_traj)))
        if not self.ws_bytes:
            _lib.check(4, sizer)
        self.ws = torch.empty(self.ws_bytes if workspace_bytes is None else int(workspace_bytes), dtype=torch.uint8, device=self.device)

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a))
        return t.to(self.device) if a.size else self.zeros(1, t.dtype)

    def zeros(self, shape, dtype):
        return self.torch.zeros(shape, dtype=dtype, device=self.device)

    def d(self, t):
        return C.c_void_p(t.data_ptr())

    def traj_args(self):
        return [self.d(self.t['traj_offsets']), C.c_int64(self.n_traj_total), C.c_int64(self.max_traj)]

    def tail_args(self):
        """status, workspace, its size, the current torch stream: what every device call ends with"""
        return [self.d(self.status), self.d(self.ws), C.c_size_t(int(self.ws.numel())), C.c_void_p(self.torch.cuda.current_stream().cuda_stream)]

    def wait(self, name=None):
        self.torch.cuda.current_stream().synchronize()
        st = int(self.status.item())
        if st:
            raise _lib.WaymoTrackError('%s failed: %s (status reported by the kernel)' % (name or self.name, _lib._STATUS.get(st, st)))


# ---------------------------------------------------------------------------------------------------------------
# the layout built on the GPU (wt_tracks_layout_*): prepare() for rows that ascend by frame slot
_LAYOUT_INTS = ('set_row_offsets', 'frame_row_offsets', 'n_traj', 'traj_offsets', 'totals', 'traj_object_id')


def layout_limits():
    """(rows of one (result, stream) up to which its id table stays in LDS, the slots of that table, the rows a workgroup scans
    per step); a table in the workspace has twice its stream's rows"""
    v = [C.c_int32(0) for _ in range(3)]
    _lib.lib().wt_tracks_layout_limits(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def layout_probe(ident, capacity):
    """the first slot the id table tries for `ident` at `capacity` slots (host code: no GPU is needed)"""
    return int(_lib.lib().wt_tracks_layout_probe(C.c_int64(int(ident)), C.c_int32(int(capacity))))


def _layout_outputs(make, R, n_streams, n_frames, n):
    """the output arrays of wt_tracks_layout_*, by name, for n rows; make(shape, dtype) allocates one"""
    o = dict((k, make(max(1, n), np.float64)) for k in ('x', 'y', 'w', 'h', 'score'))
    o.update(category=make(max(1, n), np.int32), local=make(max(1, n), np.int32), set_row_offsets=make(R + 1, np.int64),
             frame_row_offsets=make((R, n_frames + 1), np.int64), n_traj=make((R, max(1, n_streams)), np.int32),
             traj_offsets=make(R * n_streams + 1, np.int64), totals=make(3, np.int64), traj_object_id=make(max(1, n), np.int64))
    return o


def layout_tracks_host(packed, outs, n_classes):
    """wt_tracks_layout_host on R results (dicts as utils.track_packed returns them, rows ascending by frame slot, integer ids): the
    fields of prepare() that the library computes, cut to their sizes, plus 'traj_object_id'."""
    sfo = np.ascontiguousarray(packed['stream_frame_offsets'], dtype=np.int64)
    n_streams, n_frames, R = int(sfo.size - 1), int(sfo[-1]), len(outs)
    rows = np.concatenate([[0], np.cumsum([len(o['frame']) for o in outs])]).astype(np.int64)
    n = int(rows[-1])
    cat = lambda k, dt, tail=(): np.ascontiguousarray(np.concatenate([np.asarray(o[k], dtype=dt).reshape((-1,) + tail) for o in outs] + [np.zeros((0,) + tail, dt)]))
    cols = [cat('frame', np.int64), cat('category', np.int32), cat('bbox', np.float64, (4,)), cat('score', np.float64), cat('object_id', np.int64)]
    o = _layout_outputs(np.zeros, R, n_streams, n_frames, n)
    ptr = _lib.ptr
    rc = _lib.lib().wt_tracks_layout_host(C.c_int64(n_frames), C.c_int32(n_streams), ptr(sfo), C.c_int32(R), ptr(rows), *[ptr(c) for c in cols],
                                          C.c_int32(n_classes), *[ptr(o[k]) for k in COLUMNS + _LAYOUT_INTS])
    _lib.check(rc, 'wt_tracks_layout_host')
    return _cut_layout(o, R, n_streams)


def _cut_layout(o, R, n_streams):
    n_rows, n_traj_total, max_traj = [int(v) for v in o['totals']]
    p = dict((k, o[k][:n_rows]) for k in COLUMNS)
    p.update(set_row_offsets=o['set_row_offsets'], frame_row_offsets=o['frame_row_offsets'], n_traj=o['n_traj'][:, :n_streams].reshape(R, n_streams),
             traj_offsets=o['traj_offsets'], n_rows=n_rows, n_traj_total=n_traj_total, max_traj=max_traj, traj_object_id=o['traj_object_id'][:n_traj_total])
    return p


class DeviceTrackSet(object):
    """The layout of R tracker results that are in HBM already, built there by wt_tracks_layout_dev: the device twin of prepare().
    `trackers`: DeviceTracker / DeviceTrackerByte after run() - anything with out_frame, out_category, out_bbox, out_score, out_id
    and counts tensors.  ``launch()`` enqueues the call on the current torch stream; ``wait()`` synchronises, raises what the
    kernels reported and reads the three scalars n_rows, n_traj_total and max_traj - all that crosses to the host.  ``t`` holds the
    tensors by the names of COLUMNS and OFFSETS; DeviceStage and its subclasses take the set in place of prepare()'s arrays."""
    name = 'wt_tracks_layout_dev'

    def __init__(self, packed, trackers, n_classes=4, workspace_bytes=None):
        import torch
        self.torch = torch
        self.lib = _lib.lib()
        self.device = torch.device('cuda', torch.cuda.current_device())
        sfo = np.ascontiguousarray(packed['stream_frame_offsets'], dtype=np.int64)
        self.n_streams, self.n_frames, self.R, self.n_classes = int(sfo.size - 1), int(sfo[-1]), len(trackers), int(n_classes)
        if self.R < 1:
            raise ValueError('at least one result is needed')
        self.trackers = list(trackers)
        caps = [int(t.out_frame.numel()) for t in self.trackers]
        self.out_cap = sum(caps)
        self.tables = torch.from_numpy(np.asarray(
            [[t.out_frame.data_ptr(), t.out_category.data_ptr(), t.out_bbox.data_ptr(), t.out_score.data_ptr(), t.out_id.data_ptr(), t.counts.data_ptr(), cap]
             for t, cap in zip(self.trackers, caps)], dtype=np.int64)).to(self.device)
        make = lambda shape, dtype: torch.zeros(shape, dtype=getattr(torch, np.dtype(dtype).name), device=self.device)
        self.t = _layout_outputs(make, self.R, self.n_streams, self.n_frames, self.out_cap)
        self.t['stream_frame_offsets'] = torch.from_numpy(sfo).to(self.device)
        self.status = make(1, np.int32)
        self.lib.wt_tracks_layout_workspace.restype = C.c_size_t
        self.ws_bytes = int(self.lib.wt_tracks_layout_workspace(C.c_int32(self.R), C.c_int32(self.n_streams), C.c_int64(self.out_cap)))
        if not self.ws_bytes:
            _lib.check(4, 'wt_tracks_layout_workspace')
        self.ws = torch.empty(self.ws_bytes if workspace_bytes is None else int(workspace_bytes), dtype=torch.uint8, device=self.device)
        self.n_rows = self.n_traj_total = self.max_traj = None

    def nbytes(self):
        """the bytes of the layout's tensors and its workspace"""
        return sum(int(v.numel()) * v.element_size() for v in self.t.values()) + int(self.ws.numel())

    def launch(self):
        d = lambda v: C.c_void_p(v.data_ptr())
        t = self.t
        rc = self.lib.wt_tracks_layout_dev(
            C.c_int64(self.n_frames), C.c_int32(self.n_streams), d(t['stream_frame_offsets']), C.c_int32(self.R), d(self.tables), C.c_int32(self.n_classes),
            C.c_int64(self.out_cap), *[d(t[k]) for k in COLUMNS + _LAYOUT_INTS], d(self.status), d(self.ws), C.c_size_t(int(self.ws.numel())),
            C.c_void_p(self.torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, self.name)
        self.n_rows = None

    def wait(self):
        if self.n_rows is None:
            self.torch.cuda.current_stream().synchronize()
            st = int(self.status.item())
            if st:
                raise _lib.WaymoTrackError('%s failed: %s (status reported by the kernel)' % (self.name, _lib._STATUS.get(st, st)))
            self.n_rows, self.n_traj_total, self.max_traj = [int(v) for v in self.t['totals'].cpu().tolist()]
        return self

    def job_params(self, jobs):
        """what prepare() gives a stage beyond the arrays: the counts, and the result every job names"""
        self.wait()
        p = dict(n_frames=self.n_frames, n_streams=self.n_streams, R=self.R, n_classes=self.n_classes, n_rows=self.n_rows,
                 n_traj_total=self.n_traj_total, max_traj=self.max_traj, J=len(jobs))
        p['job_result'] = np.asarray([int(j.get('result', 0)) for j in jobs], dtype=np.int32).reshape(p['J'])
        if p['J'] and (p['job_result'].min() < 0 or p['job_result'].max() >= self.R):
            raise ValueError('a job names a result outside 0..%d' % (self.R - 1))
        return p

    def fetch(self):
        """the layout as numpy arrays, as layout_tracks_host() returns it (tests and tools; the chain never calls it)"""
        self.wait()
        return _cut_layout(dict((k, v.cpu().numpy()) for k, v in self.t.items()), self.R, self.n_streams)

    def host_rows(self):
        """what a stage's results() needs of prepare() to give the caller's rows back: the identity order and the object ids"""
        self.wait()
        counts = [int(t.counts[0].item()) for t in self.trackers]
        return dict(orders=[np.arange(n) for n in counts], object_ids=[t.out_id[:n].cpu().numpy() for t, n in zip(self.trackers, counts)])
