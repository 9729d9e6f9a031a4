"""Adversarial inputs of the SORT assignment code (csrc/sort_device.h: munkres_wave in its register, LDS-bitmap and helper-wave forms,
the IoU association around it).  No device code: tests/test_sort_cases.py proves on the CPU oracle alone that the cases are hard (step 6
runs, augmenting paths are long, matches get rejected by the threshold) and that they land in the dispatch class they are meant for;
tests/test_gpu_sort_assignment.py feeds them to the kernels and compares exactly.

Every builder is deterministic (numpy only, fixed seeds).

Cost matrices: cost(family, n, m) -> float32 (n, m) in [-1, 0], the range of the -iou matrices the tracker builds.
Crowd streams: crowd_frames(cfg) -> one (N_f, 5) float64 array [x, y, w, h, score] per frame, one camera, one class; packed(...) puts
them, optionally next to trivial one-box streams, into the layout of tracking.utils.pack_streams.

dispatch_class(...) restates the choice the engine and the kernel make for one frame (which Munkres variant, which step 6, where the
cost matrix lives) from the sizes alone.
"""
import collections
import zlib

import numpy as np

F32 = np.float32

FAMILIES = ('product', 'dense', 'rank1_eps', 'ties', 'const_rows', 'const_cols', 'all_equal_nonzero', 'dup_cols', 'neg_zero', 'block')
# expected to be solved by step 1 and the greedy stars (or, for const_cols, exempt from the step-6 requirement for another reason:
# its rows are identical, whether step 6 runs depends on nothing but n > 1)
NO_STEP6_REQUIRED = ('const_rows', 'const_cols', 'all_equal_nonzero', 'neg_zero')
LONG_PATH_FAMILIES = ('product', 'dense', 'rank1_eps')

# rows x cols, on every dispatch and bitmap-word edge of munkres_wave (n = min, m = max after the transposition rule):
SHAPES = (
    (1, 1), (1, 70), (70, 1),                 # smallest and degenerate sizes
    (63, 64), (64, 64), (65, 64),             # transposition; the second row word
    (128, 128),                               # last shape of <2,2>
    (129, 128),                               # transposes to 128 x 129, the first shape of <2,6>
    (100, 191), (100, 192), (100, 193),       # the column word edge at 192
    (128, 384),                               # last shape of <2,6>
    (128, 385),                               # generic path by columns
    (129, 129),                               # generic path by rows
    (62, 130), (63, 130),                     # n * ld = 8122 and 8253: either side of the 8192-float LDS budget
    (200, 260),                               # generic path, more than two row words
)
SMALL_SHAPES = ((7, 7), (6, 9))               # brute-force optimality


def _rng(family, n, m):
    return np.random.default_rng([zlib.crc32(family.encode()), n, m])


def _distinct_uniform(rng, count):
    """`count` distinct float32 values k / 2^24, 0 < k < 2^24, in random order: uniform on (0, 1), no zero, no tie."""
    k = rng.choice((1 << 24) - 1, size=count, replace=False).astype(np.int64) + 1
    return (k.astype(np.float64) / float(1 << 24)).astype(F32)


def _product(n, m, rng):
    """-(i + 1)(j + 1) / (n m): the classical worst case of Munkres (every row prefers the last column, by a margin that grows with the
    row): step 6 runs O(n) times per augmentation and the augmenting paths run through most of the stars."""
    i = np.arange(1, n + 1, dtype=np.float64)[:, None]
    j = np.arange(1, m + 1, dtype=np.float64)[None, :]
    return (-(i * j) / float(n * m)).astype(F32)


def _dense(n, m, rng):
    """Unrounded uniform values, all distinct, none zero: after step 1 a row has exactly one zero, every further zero is born from an
    exact float subtraction in step 6.  Within a row the values are laid out along a column preference the rows loosely share (a
    common key per column plus as much noise per entry), as in a crowd where every detection likes the same few tracks: plain
    independent entries leave wide matrices (100 x 192) with augmenting paths of one or two stars."""
    v = -np.sort(_distinct_uniform(rng, n * m).reshape(n, m), axis=1)[:, ::-1]          # most negative first
    order = np.argsort(rng.random(m)[None, :] + rng.random((n, m)), axis=1, kind='stable')
    c = np.empty((n, m), dtype=F32)
    np.put_along_axis(c, order, v, axis=1)
    return c


def _rank1_eps(n, m, rng):
    """-(a_i + b_j) in [-1, 0], each entry moved by up to 3 ulps: step 1 leaves all rows (almost) equal, so every row wants the same
    columns in the same order and the decision rests on the last bits.  The ulp is that of the top binade [0.5, 1), 2^-24, and a_i, b_j
    are multiples of it: every entry and every difference of entries is then a float32 number, so Munkres' float32 subtractions are
    exact and its answer is the true optimum of the perturbed matrix (with perturbations of the entry's own, finer ulp the float32
    algorithm rounds them away and ends a few 1e-8 above the optimum: measured on 7 x 7)."""
    one = 1 << 24
    a = rng.integers(0, one // 2, n, dtype=np.int64)[:, None]
    b = rng.integers(0, one // 2, m, dtype=np.int64)[None, :]
    k = np.clip(a + b + rng.integers(-3, 4, size=(n, m)), 0, one)
    return (-(k.astype(np.float64) / float(one))).astype(F32)


def _ties_perms(n, m):
    rng = _rng('ties-perm', n, m)
    return rng.permutation(n), rng.permutation(m)


def ties_optimum(n, m):
    """The unique optimum of the `ties` matrix as (rows, cols) in matrix coordinates, and its total cost."""
    rho, sigma = _ties_perms(n, m)
    lo = min(n, m)
    crow, ccol, total = [], [], 0.0                  # canonical coordinates (see _ties)
    for k in range(lo // 2):
        crow += [2 * k, 2 * k + 1]
        ccol += [2 * k + 1, 2 * k]
        total += -0.75
    if lo % 2:
        crow.append(lo - 1); ccol.append(lo - 1); total += -0.5
    crow, ccol = np.asarray(crow, dtype=np.int64), np.asarray(ccol, dtype=np.int64)
    if n <= m:
        return rho[crow], sigma[ccol], total
    return rho[ccol], sigma[crow], total             # canonical rows are the matrix's columns


def _ties(n, m, rng):
    """Three values {0, -0.25, -0.5} with a unique optimum.  In canonical coordinates (rows and columns permuted afterwards), with
    lo = min(n, m) and the matrix oriented lo x hi: rows come in pairs (2k, 2k + 1) with
        C[2k, 2k] = C[2k + 1, 2k] = -0.5,  C[2k, 2k + 1] = -0.25,  C[2k, 2j] = -0.25 for some j != k (decoys),  0 elsewhere
    (an odd last row has its single -0.5 on the diagonal).  Both rows of a pair have their minimum in column 2k, so step 1 + greedy
    stars leave one of them without a zero: step 6 must run.  Uniqueness: the dual u = -0.25 for every paired row (-0.5 for the odd
    one), v = -0.25 on the even columns 2k < lo - lo % 2 and 0 elsewhere is feasible and reaches the value -0.75 per pair; its tight
    entries are (2k, 2k), (2k, 2k + 1), (2k + 1, 2k) only, row 2k + 1 has a single tight entry, which forces row 2k to column
    2k + 1."""
    lo, hi = min(n, m), max(n, m)
    c = np.zeros((lo, hi), dtype=F32)
    pairs = lo // 2
    for k in range(pairs):
        decoy = rng.random(pairs) < 0.3
        decoy[k] = False
        c[2 * k, 2 * np.nonzero(decoy)[0]] = -0.25
        c[2 * k, 2 * k] = -0.5
        c[2 * k + 1, 2 * k] = -0.5
        c[2 * k, 2 * k + 1] = -0.25
    if lo % 2:
        c[lo - 1, lo - 1] = -0.5
    rho, sigma = _ties_perms(n, m)
    if n > m:
        c = c.T                                      # canonical rows become the matrix's columns
    out = np.zeros((n, m), dtype=F32)
    out[np.ix_(rho, sigma)] = c
    return out


def _const_rows(n, m, rng):
    return np.repeat((-_distinct_uniform(rng, n))[:, None], m, axis=1)


def _const_cols(n, m, rng):
    return np.repeat((-_distinct_uniform(rng, m))[None, :], n, axis=0)


def _all_equal_nonzero(n, m, rng):
    return np.full((n, m), -0.37, dtype=F32)


def _dup_cols(n, m, rng):
    """A dense matrix whose every column appears twice, side by side (an odd m loses the twin of its last column): every zero comes
    with a tied twin, two rows can share a preferred base column, a third one cannot."""
    base = (-_distinct_uniform(rng, n * ((m + 1) // 2))).reshape(n, (m + 1) // 2)
    return np.ascontiguousarray(np.repeat(base, 2, axis=1)[:, :m])


def _neg_zero(n, m, rng):
    c = np.zeros((n, m), dtype=F32)
    c[rng.random((n, m)) < 0.5] = F32(-0.0)
    return c


def _block(n, m, rng):
    """Two dense blocks on a background of exact zeros - a crowd (more rows than columns in its block, so some of its rows must leave
    it) and a second group, the IoU matrix of two clusters that do not overlap each other."""
    c = np.zeros((n, m), dtype=F32)
    r1 = n // 2
    c1 = min(max(1, (2 * r1) // 3), max(1, m - 1))
    c2 = min(m - c1, (n - r1) + 3)
    if r1 > 0:
        c[:r1, :c1] = (-_distinct_uniform(rng, r1 * c1)).reshape(r1, c1)
    if c2 > 0:
        c[r1:, c1:c1 + c2] = (-_distinct_uniform(rng, (n - r1) * c2)).reshape(n - r1, c2)
    return c


_BUILDERS = dict(product=_product, dense=_dense, rank1_eps=_rank1_eps, ties=_ties, const_rows=_const_rows, const_cols=_const_cols,
                 all_equal_nonzero=_all_equal_nonzero, dup_cols=_dup_cols, neg_zero=_neg_zero, block=_block)


def cost(family, n, m):
    c = np.ascontiguousarray(_BUILDERS[family](n, m, _rng(family, n, m)), dtype=F32)
    assert c.shape == (n, m) and np.all(c <= 0) and np.all(c >= -1)
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# crowd streams

Crowd = collections.namedtuple('Crowd', 'name seed counts box spacing jitter move jump integer iou_thr')
# counts: detections per frame.  box: box side in pixels (each box +-20 %).  spacing: grid pitch, well below the box side, so that
# nearly every pair of boxes overlaps.  jitter: uniform offset per box and frame, in pixels.  move: drift per frame as a fraction of the
# box side.  jump: share of the objects that are re-drawn somewhere else in the region each frame.  iou_thr: the class's threshold -
# high enough that a good part of the assignment is rejected, so the rejected tracks linger (max_age = 2) next to the newborn ones and
# T grows to 2 - 3 N.
MAX_AGE, MIN_HITS, N_CLASSES, CROWD_CLASS = 2, 0, 4, 2

CROWDS = {
    # (a) N, T <= 128: munkres_wave_reg<2,2>, HELP_STEP1, row-parallel HELP_STEP6
    'a': Crowd('a', 101, (30, 38, 34, 26, 40, 31, 90, 28), 90.0, 7.0, 3.0, 0.10, 0.30, True, 0.70),
    # (b) n <= 128 < m <= 384, n * ld within the few-tracker LDS budget: <2,6>, column-parallel HELP_STEP6C, cost matrix in LDS
    'b': Crowd('b', 102, (70, 150, 80, 84, 76, 88, 82, 60), 110.5, 6.5, 2.5, 0.12, 0.35, False, 0.85),
    # (c) as (b) with n * ld above the few-tracker budget (120 x 383 = 45960 floats): cost matrix in global memory under helpers
    'c': Crowd('c', 103, (118, 124, 120, 122, 119, 121, 120), 120.0, 6.0, 3.0, 0.15, 0.45, True, 0.90),
    # (d) N > 128 (or T > 384): the generic LDS-bitmap path
    'd': Crowd('d', 104, (131, 136, 130, 134, 129, 133), 130.25, 6.0, 2.0, 0.10, 0.30, False, 0.85),
}


def crowd_frames(cfg):
    rng = np.random.default_rng(cfg.seed)
    n_max = max(cfg.counts)
    side = int(np.ceil(np.sqrt(n_max)))
    gx, gy = np.meshgrid(np.arange(side), np.arange(side))
    home = np.stack([gx.ravel(), gy.ravel()], axis=1)[rng.permutation(side * side)[:n_max]] * cfg.spacing + 200.0
    size = cfg.box * rng.uniform(0.8, 1.2, (n_max, 2))
    vel = rng.normal(0.0, cfg.move * cfg.box, (n_max, 2))
    pos = home.astype(np.float64)
    frames = []
    for count in cfg.counts:
        pos = pos + vel
        jump = rng.random(n_max) < cfg.jump
        pos[jump] = 200.0 + rng.uniform(0.0, side * cfg.spacing, (int(jump.sum()), 2))
        vel[jump] = rng.normal(0.0, cfg.move * cfg.box, (int(jump.sum()), 2))
        who = np.sort(rng.permutation(n_max)[:count])
        xy = pos[who] + rng.uniform(-cfg.jitter, cfg.jitter, (count, 2))
        wh = size[who] * rng.uniform(0.95, 1.05, (count, 2))
        if cfg.integer:
            xy, wh = np.round(xy), np.maximum(np.round(wh), 1.0)
        score = rng.uniform(0.5, 1.0, (count, 1))
        order = rng.permutation(count)
        frames.append(np.ascontiguousarray(np.concatenate([xy, wh, score], axis=1)[order]))
    return frames


def dets_xyxy(frame):
    """The float32 rows [x1, y1, x2, y2, score] the tracker builds from a frame (utils.py:33: x + w in float64, then float32)."""
    f = np.asarray(frame, dtype=np.float64)
    return np.stack([f[:, 0], f[:, 1], f[:, 0] + f[:, 2], f[:, 1] + f[:, 3], f[:, 4]], axis=1).astype(F32)


def iou_thresholds(cfg):
    thr = [0.3] * N_CLASSES
    thr[CROWD_CLASS - 1] = cfg.iou_thr
    return thr


def packed(cfg, n_trivial_streams=0):
    """The crowd stream (stream 0), then n_trivial_streams streams of one steady box per frame and class 1..4 in turn, in the layout of
    tracking.utils.pack_streams (no clipping).  64 trivial streams make 65 streams x 4 classes = 260 trackers: beyond the 256 up to
    which the engine launches helper waves and the large LDS budget."""
    frames = crowd_frames(cfg)
    rows, cats, frame_off, stream_off = [], [], [0], [0]
    n = 0
    for f in frames:
        rows.append(f); cats.append(np.full(len(f), CROWD_CLASS, np.int32)); n += len(f); frame_off.append(n)
    stream_off.append(len(frames))
    for s in range(n_trivial_streams):
        for k in range(3):
            rows.append(np.array([[50.0 + 3 * s + 2 * k, 40.0 + s, 30.0 + (s % 7), 20.0 + (s % 5), 0.9]]))
            cats.append(np.array([1 + s % N_CLASSES], np.int32)); n += 1; frame_off.append(n)
        stream_off.append(len(frame_off) - 1)
    r = np.concatenate(rows, axis=0)
    n_streams = len(stream_off) - 1
    return dict(x=np.ascontiguousarray(r[:, 0]), y=np.ascontiguousarray(r[:, 1]), w=np.ascontiguousarray(r[:, 2]),
                h=np.ascontiguousarray(r[:, 3]), score=np.ascontiguousarray(r[:, 4]), category=np.concatenate(cats).astype(np.int32),
                frame_det_offsets=np.asarray(frame_off, dtype=np.int64), stream_frame_offsets=np.asarray(stream_off, dtype=np.int64),
                frame_ids=np.arange(len(frame_off) - 1, dtype=np.int64), clip_w=np.zeros(n_streams), clip_h=np.zeros(n_streams),
                stream_keys=[('s%d' % i, 'CROWD') for i in range(n_streams)])


N_TRIVIAL = 64


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch arithmetic

LDS_COST_FLOATS = 8192            # sort_engine.hip kLdsCostFloats (and sort_single.hip: assignment_kernel, associate_kernel, Sort)
LDS_COST_FLOATS_FEW = 36864       # sort_engine.hip kLdsCostFloatsFew
HELP_LDS_BYTES = 10464            # sort_device.h help_lds_bytes(): sizeof(HelpJob) rounded up to 16
FEW_TRACKERS = 256


def munkres_lds_bytes(n_small, n_big):
    """sort_device.h munkres_lds_bytes."""
    w = (n_big + 63) // 64
    return ((2 * n_small + n_big) * 4 + 7) // 8 * 8 + n_small * w * 8 + 16


def engine_plan(max_frame_dets, n_streams, max_age=MAX_AGE, n_classes=N_CLASSES):
    """(floats of cost matrix the tracker keeps in LDS, helper waves launched) - mirrors plan_tracking of sort_engine.hip (the
    few-tracker budget: what 160 KiB leave next to the bitmaps and the helper job, clamped to [8192, 36864], with the capacities
    above it and the clamp to the full matrix below it) and the helper decision of run_tracking.  A change there must show up here as a failing
    expectation in tests/test_sort_cases.py, not as a silent loss of coverage."""
    cap_n = max(int(max_frame_dets), 1)
    cap = cap_n * (max_age + 2)
    full = cap_n * (cap | 1)
    mk = munkres_lds_bytes(cap_n, cap)
    budget = LDS_COST_FLOATS
    few = n_streams > 0 and n_streams * n_classes <= FEW_TRACKERS
    if few:
        room = (160 * 1024 - 512 - mk - HELP_LDS_BYTES - 16) // 4
        budget = min(room, LDS_COST_FLOATS_FEW)
        budget = max(budget, LDS_COST_FLOATS)
    lds_cost = min(full, budget)
    lds = (lds_cost * 4 + 15) // 16 * 16 + mk
    helpers = few and (lds + 15) // 16 * 16 + HELP_LDS_BYTES <= 160 * 1024 - 256
    return lds_cost, helpers


def dispatch_class(n_dets, n_trks, lds_cost):
    """Class of one frame's assignment: None when there is none (no tracks or no detections), else a dict with
    cls 'a' .. 'd', variant, cost ('lds' / 'global'), transposed."""
    if n_dets <= 0 or n_trks <= 0:
        return None
    n, m = min(n_dets, n_trks), max(n_dets, n_trks)
    ld = m | 1
    where = 'lds' if n * ld <= lds_cost else 'global'
    if n <= 128 and m <= 128:
        cls, variant = 'a', '<2,2>'
    elif n <= 128 and m <= 384:
        variant = '<2,6>'
        cls = 'b' if where == 'lds' else 'c'
    else:
        cls, variant = 'd', 'generic'
    return dict(cls=cls, variant=variant, cost=where, transposed=n_trks < n_dets, n=n, m=m)


def crowd_trace(oracle, cfg, n_streams=1):
    """Step oracle.Sort through the crowd stream frame by frame.  One dict per frame: dets (float32 xyxy + score), trks (predicted boxes
    the frame is associated against, read before the update), N, T, dispatch (dispatch_class under the plan of a launch with n_streams
    streams), and for frames with an assignment: cost (-iou, float32), raw (the assignment before the threshold), stats (work counters
    of the oracle), matches / unmatched_dets / unmatched_trks of oracle.associate, rejected (raw pairs the threshold removed)."""
    frames = crowd_frames(cfg)
    lds_cost, helpers = engine_plan(max(len(f) for f in frames), n_streams)
    sort = oracle.Sort(MAX_AGE, MIN_HITS)
    out = []
    for f in frames:
        dets = dets_xyxy(f)
        trks = sort.predicted()
        rec = dict(dets=dets, trks=trks, N=len(dets), T=len(trks), dispatch=dispatch_class(len(dets), len(trks), lds_cost),
                   helpers=helpers, lds_cost=lds_cost)
        if rec['dispatch'] is not None:
            rec['cost'] = oracle.iou_cost(dets, trks)
            rec['raw'], rec['stats'] = oracle.linear_assignment_stats(rec['cost'])
            rec['matches'], rec['unmatched_dets'], rec['unmatched_trks'] = oracle.associate(dets, trks, cfg.iou_thr)
            kept = set(map(tuple, rec['matches'].tolist()))
            rec['rejected'] = [p for p in map(tuple, rec['raw'].tolist()) if p not in kept]
        sort.update(dets, cfg.iou_thr)
        out.append(rec)
    return out
