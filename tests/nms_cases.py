"""Adversarial inputs of the hard-NMS kernels (csrc/det_nms.hip) with their exact answers, and a float32 reference.  No device code:
tests/test_nms_cases.py proves every closed form here on the CPU against two NMS implementations, tests/test_gpu_nms_edges.py feeds the
cases to the column sweep, the row sweep and the segmented form.

Every builder is deterministic and returns a Case: float32 boxes ALREADY IN SCORE ORDER (row 0 = best score), optional int32 group ids,
the IoU threshold and the expected keep mask.  The expected mask is a closed form of the row number, derived in the builder's docstring
from the geometry, never the output of an NMS.

The float32 contract (greedy_nms_f32 = iou_gt of the kernel = torchvision's CPU kernel, one rounded operation at a time):

    left = max(a.x1, b.x1), right = min(a.x2, b.x2), top = max(a.y1, b.y1), bottom = min(a.y2, b.y2)
    width = max(right - left, 0), height = max(bottom - top, 0), inter = width * height
    sa = (a.x2 - a.x1) * (a.y2 - a.y1), sb likewise
    suppress  <=>  inter / ((sa + sb) - inter) > thr

NaN coordinates: the kernel's fmaxf / fminf return the other operand when one is NaN, numpy's and torch's maximum / minimum return
NaN.  No decision depends on that difference: a box with a NaN coordinate has sa = NaN (the coordinate enters its own area), so the
denominator and the quotient are NaN whatever `inter` became, and NaN > thr is false for every thr.  greedy_nms_f32 therefore uses
numpy's plain maximum / minimum; test_nms_cases.py checks both NaN conventions give the same masks on every case that has a NaN.
"""
import collections
from fractions import Fraction

import numpy as np

Case = collections.namedtuple('Case', 'boxes idxs thr keep')

F32 = np.float32
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

COL_SIZES = (1, 2, 33, 64, 65, 127, 128, 129, 6143, 6144)            # column sweep (n <= 6144)
ROW_SIZES = (6145, 6160, 6161, 6208, 6209)                           # row sweep: last tile of 1, 16, 17, 64, 1 rows


def _quotient(a, b, nan_like_fmaxf=False):
    """The float32 sequence above for box a (4,) against boxes b (m, 4) -> float32 quotients (m,)."""
    if nan_like_fmaxf:
        fmax, fmin = np.fmax, np.fmin
    else:
        fmax, fmin = np.maximum, np.minimum
    zero = F32(0)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        left, right = fmax(a[0], b[:, 0]), fmin(a[2], b[:, 2])
        top, bottom = fmax(a[1], b[:, 1]), fmin(a[3], b[:, 3])
        width, height = fmax(right - left, zero), fmax(bottom - top, zero)
        inter = width * height
        sa = (a[2] - a[0]) * (a[3] - a[1])
        sb = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        q = inter / ((sa + sb) - inter)
    assert q.dtype == np.float32
    return q


def greedy_nms_f32(boxes, idxs, thr, nan_like_fmaxf=False):
    """Plain greedy NMS over rows in the given order, numpy float32, every operation rounded on its own -> bool keep (n,)."""
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    n = b.shape[0]
    g = None if idxs is None else np.asarray(idxs)
    keep = np.ones(n, dtype=bool)
    thr = F32(thr)
    for i in range(n - 1):
        if not keep[i]:
            continue
        sup = _quotient(b[i], b[i + 1:], nan_like_fmaxf) > thr
        if g is not None:
            sup &= g[i + 1:] == g[i]
        keep[i + 1:] &= ~sup
    return keep


# ---------------------------------------------------------------------------------------------------------------------------------
# ladders

# period -> (shift, width): boxes `width` wide and 10 high, box k shifted by shift * k along x.  Two boxes d steps apart overlap in
# (width - d * shift) x 10, so IoU(d) = (width - d * shift) / (width + d * shift) while d * shift < width, else 0.  Box k suppresses
# k + 1 .. k + period - 1 (IoU > 0.5) and not k + period (IoU <= 0.5): greedy keeps exactly the rows with k % period == 0 - every kept
# box rests on the decision about ALL the boxes before it (a suppressed box overlaps its successor too and must not suppress it).
LADDERS = {2: (3, 10), 3: (1, 8), 5: (1, 14)}
# the IoUs of the first `period` distances, as derived above (test_nms_cases.py recomputes them from the boxes in exact arithmetic)
LADDER_IOUS = {2: (Fraction(7, 13), Fraction(4, 16)),
               3: (Fraction(7, 9), Fraction(6, 10), Fraction(5, 11)),
               5: (Fraction(13, 15), Fraction(12, 16), Fraction(11, 17), Fraction(10, 18), Fraction(9, 19))}


def _ladder_boxes(pos, y0, period):
    shift, width = LADDERS[period]
    x0 = (np.asarray(pos, dtype=np.int64) * shift).astype(np.float32)            # integers below 2^24: exact
    y0 = np.asarray(y0, dtype=np.float32) + np.zeros_like(x0)
    return np.stack([x0, y0, x0 + F32(width), y0 + F32(10)], axis=1)


def ladder(n, period=2):
    """One chain as deep as n.  period 2: IoU(k, k+1) = 7/13 > 0.5, IoU(k, k+2) = 4/16: keep = even k, every row hangs on the row before
    it (64 rounds of the column sweep's fixed-point iteration per tile, every step across lanes 31/32 and across the tile boundary).
    periods 3 and 5 (LADDERS) are never aligned to 64."""
    k = np.arange(n)
    return Case(_ladder_boxes(k, 0, period), None, 0.5, k % period == 0)


def interleaved_ladders(n, L):
    """L independent period-2 ladders 20 apart in y (boxes are 10 high: ladders never touch); row i is position i // L of ladder i % L.
    keep = (i // L) even.  Every dependency spans L rows = L / 64 tiles: the row that decides row i was itself decided L rows earlier,
    and the suppressed rows in between overlap row i without a say."""
    i = np.arange(n)
    return Case(_ladder_boxes(i // L, 20 * (i % L), 2), None, 0.5, (i // L) % 2 == 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# uniform masks

def _identical(n):
    return np.tile(np.array([[0, 0, 10, 10]], dtype=np.float32), (n, 1))


def _disjoint(n, step=20):
    """10 x 10 boxes on a grid of pitch `step`, 100 per grid row."""
    k = np.arange(n)
    x0, y0 = (step * (k % 100)).astype(np.float32), (step * (k // 100)).astype(np.float32)
    return np.stack([x0, y0, x0 + F32(10), y0 + F32(10)], axis=1)


def identical(n):
    """n copies of one box: IoU = 100 / 100 = 1 > 0.5 for every pair, every mask word is full; only row 0 survives."""
    return Case(_identical(n), None, 0.5, np.arange(n) == 0)


def disjoint(n):
    """No two boxes overlap (inter = 0, quotient 0): all kept, the mask is all zeros."""
    return Case(_disjoint(n), None, 0.5, np.ones(n, dtype=bool))


def identical_two_groups(n):
    """Identical boxes, group = row parity: the first row of each group survives."""
    k = np.arange(n)
    return Case(_identical(n), (k % 2).astype(np.int32), 0.5, k < 2)


def ladder_two_groups(n):
    """The period-2 ladder with group = row parity: the only pairs above the threshold (neighbours) are in different groups, same-group
    pairs are 2 or more steps apart (IoU <= 4/16): all kept."""
    k = np.arange(n)
    return Case(_ladder_boxes(k, 0, 2), (k % 2).astype(np.int32), 0.5, np.ones(n, dtype=bool))


EXTREME_GROUPS = (INT32_MIN, -1, INT32_MAX, 0, INT32_MAX - 1, INT32_MIN + 1)


def extreme_groups(n):
    """Identical boxes whose group ids cycle through negative values and the ends of the int32 range: the first row of each of the six
    groups survives (ids are compared for equality only)."""
    k = np.arange(n)
    g = np.array(EXTREME_GROUPS, dtype=np.int64)[k % len(EXTREME_GROUPS)].astype(np.int32)
    return Case(_identical(n), g, 0.5, k < len(EXTREME_GROUPS))


# ---------------------------------------------------------------------------------------------------------------------------------
# thresholds

def thr0_touching(n):
    """thr = 0, boxes that share an edge (pitch 10 = width): width or height clamps to 0, inter = 0, 0 > 0 is false: all kept."""
    return Case(_disjoint(n, step=10), None, 0.0, np.ones(n, dtype=bool))


def thr0_overlap(n):
    """thr = 0, a row of 10 x 10 boxes of pitch 9: neighbours overlap in 1 x 10 (IoU 10/190 > 0), boxes 2 apart are disjoint: keep = even k."""
    k = np.arange(n)
    x0 = (9 * k).astype(np.float32)
    boxes = np.stack([x0, np.zeros(n, dtype=np.float32), x0 + F32(10), np.full(n, 10, dtype=np.float32)], axis=1)
    return Case(boxes, None, 0.0, k % 2 == 0)


def thr1_identical(n):
    """thr = 1, identical boxes: the quotient is exactly 100 / (100 + 100 - 100) = 1 and 1 > 1 is false: all kept."""
    return Case(_identical(n), None, 1.0, np.ones(n, dtype=bool))


def thr_neg_disjoint(n):
    """thr = -1, disjoint boxes in two groups (row parity), row n // 2 with a NaN coordinate: every same-group pair has the finite quotient
    0 > -1, so rows 0 and 1 suppress the rest of their groups; the NaN row's quotients are NaN: it survives and suppresses nothing."""
    k = np.arange(n)
    boxes = _disjoint(n)
    keep = k < 2
    if n > 4:
        boxes[n // 2, 1] = np.nan
        keep = keep | (k == n // 2)
    return Case(boxes, (k % 2).astype(np.int32), -1.0, keep)


# ---------------------------------------------------------------------------------------------------------------------------------
# degenerate and non-finite rows

N_DEGENERATE_KINDS = 8


def degenerate_in_ladder(n):
    """The period-2 ladder with every row i % 7 == 3 replaced by a degenerate or non-finite box that lies across the ladder (the kind
    cycles with i // 7).  By the float32 sequence each such row neither suppresses nor is suppressed at thr = 0.5:
      zero width / zero height: sa = 0 and inter = 0 against everything: quotient 0 / sb = 0, or 0 / 0 = NaN against another such row;
      x2 < x1:                  right <= x2 < x1 <= left: width clamps to 0, inter = 0: quotient 0, -0 or 0 / 0 = NaN;
      one NaN coordinate:       sa = NaN: quotient NaN (whichever way max / min treat NaN, see the module docstring);
      infinite extent(s):       sa = inf; against a finite box inter is finite: inter / inf = 0; against another infinite box inter = inf:
                                (inf + inf) - inf = NaN.
    The remaining rows are a ladder among themselves: keep = the ladder row's rank among the ladder rows is even; special rows: kept."""
    i = np.arange(n)
    special = i % 7 == 3
    rank = np.cumsum(~special) - 1
    boxes = _ladder_boxes(np.maximum(rank, 0), 0, 2)
    inf = F32(np.inf)
    for r in np.nonzero(special)[0]:
        kind = (r // 7) % N_DEGENERATE_KINDS
        x1, y1, x2, y2 = boxes[r]
        if kind == 0:
            boxes[r] = (x1 + 5, y1, x1 + 5, y2)                     # zero width, inside its neighbours
        elif kind == 1:
            boxes[r] = (x1, y1 + 5, x2, y1 + 5)                     # zero height
        elif kind == 2:
            boxes[r] = (x2, y1, x1, y2)                             # x2 < x1
        elif kind == 3:
            boxes[r, (r // (7 * N_DEGENERATE_KINDS)) % 4] = np.nan  # one NaN coordinate, each of the four in turn
        elif kind == 4:
            boxes[r] = (x1, y1, inf, y2)                            # one infinite extent
        elif kind == 5:
            boxes[r] = (x1, y1, inf, inf)                           # two infinite extents
        elif kind == 6:
            boxes[r] = (-inf, y1, inf, y2)                          # infinite to both sides
        else:
            boxes[r] = (x1, -inf, x2, y2)
    return Case(boxes, None, 0.5, special | (rank % 2 == 0))


# every (case name -> builder(n)) that runs through both single-problem sweeps at every size
CASES = collections.OrderedDict([
    ('ladder2', lambda n: ladder(n, 2)),
    ('ladder3', lambda n: ladder(n, 3)),
    ('ladder5', lambda n: ladder(n, 5)),
    ('interleaved64', lambda n: interleaved_ladders(n, 64)),
    ('interleaved256', lambda n: interleaved_ladders(n, 256)),
    ('interleaved1000', lambda n: interleaved_ladders(n, 1000)),
    ('identical', identical),
    ('disjoint', disjoint),
    ('identical_two_groups', identical_two_groups),
    ('ladder_two_groups', ladder_two_groups),
    ('extreme_groups', extreme_groups),
    ('thr0_touching', thr0_touching),
    ('thr0_overlap', thr0_overlap),
    ('thr1_identical', thr1_identical),
    ('thr_neg_disjoint', thr_neg_disjoint),
    ('degenerate_in_ladder', degenerate_in_ladder),
])
CASES_WITH_NAN = ('thr_neg_disjoint', 'degenerate_in_ladder')


# ---------------------------------------------------------------------------------------------------------------------------------
# knife-edge pairs

HALF = F32(0.5)
KNIFE_QUOTIENTS = (np.nextafter(HALF, F32(0)), HALF, np.nextafter(HALF, F32(1)))      # class 0, 1, 2; only class 2 suppresses
KNIFE_MIN_PER_CLASS = 200
KNIFE_MIN_FLIPS = 32
KNIFE_PAIRS_BELOW, KNIFE_PAIRS_ABOVE = 400, 1040       # pairs per class: 2400 rows (column sweep) and 6240 rows (row sweep)
FUSED_FORMS = ('fma(wa,ha,sb) - inter', 'fma(wb,hb,sa) - inter', 'fma(-w,h,sa+sb)', 'fma(-w,h,fma(wa,ha,sb))', 'fma(-w,h,fma(wb,hb,sa))')


def _pair_terms(a, b):
    """float32 terms of the sequence for pairs a[k], b[k]: (width, height, wa, ha, wb, hb, inter, sa, sb)."""
    left, right = np.maximum(a[:, 0], b[:, 0]), np.minimum(a[:, 2], b[:, 2])
    top, bottom = np.maximum(a[:, 1], b[:, 1]), np.minimum(a[:, 3], b[:, 3])
    width, height = np.maximum(right - left, F32(0)), np.maximum(bottom - top, F32(0))
    wa, ha, wb, hb = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    return width, height, wa, ha, wb, hb, width * height, wa * ha, wb * hb


def _fma(x, y, z):
    """float32 fused multiply-add: the product of two float32 is exact in float64, the sum is rounded there and once more to float32."""
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


def fused_quotients(a, b):
    """The quotient of each pair with the products contracted into the sums in each way a compiler may choose (FUSED_FORMS); the
    numerator stays the rounded product.  -> float32 (len(FUSED_FORMS), m)."""
    width, height, wa, ha, wb, hb, inter, sa, sb = _pair_terms(a, b)
    sum_a, sum_b = _fma(wa, ha, sb), _fma(wb, hb, sa)
    dens = (sum_a - inter, sum_b - inter, _fma(-width, height, sa + sb), _fma(-width, height, sum_a), _fma(-width, height, sum_b))
    return np.stack([inter / d for d in dens])


_knife_pool = {}


def knife_edge_pool(per_class):
    """Pairs A, B = A shifted by about a third of its width (IoU = (w - s) / (w + s) = 1/2 at s = w / 3) with fractional coordinates:
    origins up to 2000, sizes 40 .. 400, the shift and every coordinate of B jittered so that the quotient spreads over about 1e-5
    around 0.5.  Rejection sampling keeps the pairs whose float32 quotient is exactly one of KNIFE_QUOTIENTS, `per_class` of each, in
    sampling order.  -> (a (3, per_class, 4), b likewise, samples drawn).  Deterministic (fixed seed, fixed batch size); cached."""
    if per_class in _knife_pool:
        return _knife_pool[per_class]
    rng = np.random.default_rng(20240517)
    found_a, found_b = [[], [], []], [[], [], []]
    counts, drawn, m = [0, 0, 0], 0, 1 << 18
    while min(counts) < per_class:
        assert drawn < 400 * m, 'knife-edge sampler: hit rate collapsed (%r after %d samples)' % (counts, drawn)
        w, h = rng.uniform(40, 400, m), rng.uniform(40, 400, m)
        ox, oy = rng.uniform(0, 2000, m), rng.uniform(0, 2000, m)
        s = w / 3 * (1 + rng.uniform(-1.5e-5, 1.5e-5, m))
        j = rng.uniform(-1e-3, 1e-3, (4, m))
        a = np.stack([ox, oy, ox + w, oy + h], axis=1).astype(np.float32)
        b = np.stack([ox + s + j[0], oy + j[1], ox + s + w + j[2], oy + h + j[3]], axis=1).astype(np.float32)
        width, height, wa, ha, wb, hb, inter, sa, sb = _pair_terms(a, b)
        q = inter / ((sa + sb) - inter)
        drawn += m
        for c, target in enumerate(KNIFE_QUOTIENTS):
            sel = np.nonzero(q == target)[0]
            found_a[c].append(a[sel]); found_b[c].append(b[sel]); counts[c] += len(sel)
    pa = np.stack([np.concatenate(x)[:per_class] for x in found_a])
    pb = np.stack([np.concatenate(x)[:per_class] for x in found_b])
    _knife_pool[per_class] = (pa, pb, drawn)
    return _knife_pool[per_class]


def knife_edge(per_class):
    """3 * per_class pairs in adjacent rows (A above B), pair p of class p % 3 with group id p: A is always kept, B is suppressed only in
    class 2 (quotient = nextafter(0.5, 1) > 0.5; 0.5 > 0.5 and nextafter(0.5, 0) > 0.5 are false).  Also returns, per pair, whether any
    fused form of the quotient (fused_quotients) decides it differently.  -> (Case, flips bool (3 * per_class,))"""
    pa, pb, _ = knife_edge_pool(per_class)
    a = pa.transpose(1, 0, 2).reshape(-1, 4)                  # pair p = (class p % 3, sample p // 3)
    b = pb.transpose(1, 0, 2).reshape(-1, 4)
    npairs = a.shape[0]
    boxes = np.stack([a, b], axis=1).reshape(-1, 4)
    idxs = np.repeat(np.arange(npairs, dtype=np.int32), 2)
    keep = np.ones(2 * npairs, dtype=bool)
    keep[1::2] = np.arange(npairs) % 3 != 2
    flips = ((fused_quotients(a, b) > HALF) != (np.arange(npairs) % 3 == 2)[None]).any(axis=0)
    return Case(boxes, idxs, 0.5, keep), flips
