"""Adversarial inputs of the ensemble's linear soft-NMS (csrc/ensemble.hip: the dependency-free softnms_fast_kernel and the serial nms_core)
with their exact answers, and a numpy float64 restatement of the reference.  No device code: tests/test_softnms_cases.py proves every
expectation here on the CPU against the restatement and against the C oracle (oracle/softnms_oracle.c), tests/test_gpu_softnms_edges.py
feeds the cases to wt_ensemble_groups_host / wt_ensemble_groups_dev.

Every builder is deterministic and returns a Case: float64 rows [score, x, y, w, h] of all groups, the int64 group offsets, thr (the
IoU threshold), cut (soft_nms_cut), the centre flag (rows are [score, cx, cy, w, h], method | 16), and the expected output: exp_rows has
the input's row capacity, group g's kept rows start at row offsets[g] and there are exp_counts[g] of them (rows past the count are zero and
are not compared).  `closed` tells where the expectation comes from: True = a closed form of the row number, derived in the builder's
docstring and never taken from a soft-NMS run; False = the output of soft_nms_ref below.

The float64 contract (soft_nms_ref = detnet/utils/box_utils.py:307-395 nms(soft=True, conf_thresh=0) behind detnet/nn/tta.py:8-19 and
detnet/ensemble.py:19-28, one rounded operation at a time):

    cx = x + w / 2 (centre form: cx = x), x1 = cx - w * 0.5, x2 = cx + w * 0.5, likewise y;  area = (x2 - x1) * (y2 - y1)
    boxes are taken in descending score, NaN first, equal scores by the HIGHER input index first (before() of ensemble.hip = a stable
    ascending sort read from the back); the order is fixed once, scores are never sorted again
    the best remaining box i is kept with its current score; for every remaining box j
        w = max(min(x2_j, x2_i) - max(x1_j, x1_i), 0), h likewise, inter = w * h
        union = (area_j - inter) + area_i,  IoU = inter / union
        weight = min(max((cut - IoU) / (cut - thr), 0), 1)  with NaN passing through,  score_j = score_j * weight
    and j stays in the list only if score_j >= 0 (false for NaN)
    output row = [score, cxo - wd / 2 (centre form: cxo), cyo - hd / 2 (cyo), wd, hd],  wd = x2 - x1, cxo = (x1 + x2) * 0.5

NaN coordinates: numpy's maximum / minimum return NaN when an operand is NaN, the oracle's and the kernels' compare-and-select keep
the other operand.  No result depends on that difference: a NaN corner (a NaN input, or inf - inf in the corner conversion) enters the
box's own area, so the union and the weight of every pair the box is in are NaN whatever `inter` became; test_softnms_cases.py checks that
the restatement and the oracle, which differ in exactly this, agree on every case.
"""
import collections
from fractions import Fraction

import numpy as np

Case = collections.namedtuple('Case', 'rows offsets thr cut centre exp_rows exp_counts closed')

INF, NAN = float('inf'), float('nan')


def soft_nms_ref(rows, thr, cut, centre=False):
    """The contract above for one group -> the kept rows (k, 5), float64, in keep order."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    n = rows.shape[0]
    if n == 0:
        return np.zeros((0, 5))
    s, x, y, w, h = (rows[:, c] for c in range(5))
    with np.errstate(all='ignore'):
        cx = x if centre else x + w / 2
        cy = y if centre else y + h / 2
        x1, y1, x2, y2 = cx - w * 0.5, cy - h * 0.5, cx + w * 0.5, cy + h * 0.5
        area = (x2 - x1) * (y2 - y1)
        idx = np.argsort(s, kind='stable')                         # ascending, NaN last, ties in input order; read from the back
        ss = s[idx].copy()
        keep, new_scores = [], []
        while idx.size > 1:
            i = idx[-1]
            keep.append(i); new_scores.append(ss[-1])
            idx, ss = idx[:-1], ss[:-1]
            ww = np.maximum(np.minimum(x2[idx], x2[i]) - np.maximum(x1[idx], x1[i]), 0.0)
            hh = np.maximum(np.minimum(y2[idx], y2[i]) - np.maximum(y1[idx], y1[i]), 0.0)
            inter = ww * hh
            union = (area[idx] - inter) + area[i]
            iou = inter / union
            weight = np.minimum(np.maximum((cut - iou) / (cut - thr), 0.0), 1.0)
            ss = ss * weight
            high = ss >= 0.0
            idx, ss = idx[high], ss[high]
        if idx.size > 0:
            keep.append(idx[-1]); new_scores.append(ss[-1])
        k = np.asarray(keep, dtype=np.int64)
        wd, hd = x2[k] - x1[k], y2[k] - y1[k]
        cxo, cyo = (x1[k] + x2[k]) * 0.5, (y1[k] + y2[k]) * 0.5
        ox = cxo if centre else cxo - wd / 2
        oy = cyo if centre else cyo - hd / 2
    return np.stack([np.asarray(new_scores, dtype=np.float64), ox, oy, wd, hd], axis=1)


def reference(case):
    """soft_nms_ref on every group of a case -> (exp_rows, exp_counts) in the layout of Case."""
    out = np.zeros_like(case.rows)
    counts = np.zeros(len(case.offsets) - 1, dtype=np.int64)
    for g in range(len(counts)):
        a, b = int(case.offsets[g]), int(case.offsets[g + 1])
        kept = soft_nms_ref(case.rows[a:b], case.thr, case.cut, case.centre)
        out[a:a + len(kept)] = kept
        counts[g] = len(kept)
    return out, counts


def oracle_expected(oracle, case, method=2, k_inputs=2):
    """The C oracle on every group of a case, for soft-NMS (2), hard NMS (1) or weighted fusion (0, the group's rows split into k_inputs
    inputs as input_sizes() says) -> (exp_rows, exp_counts).  Corner-form rows go through wto_ensemble_groups, centre-form rows through
    the bare merge functions, as the method | 16 contract of include/waymotrack.h says."""
    sizes = input_sizes(case, k_inputs)
    if not case.centre:
        out, counts = oracle.ensemble_groups(case.rows, case.offsets, sizes, k_inputs, method, case.thr, case.cut)
        return out.copy(), counts.copy()
    out = np.zeros_like(case.rows)
    counts = np.zeros(len(case.offsets) - 1, dtype=np.int64)
    for g in range(len(counts)):
        a, b = int(case.offsets[g]), int(case.offsets[g + 1])
        if a == b:
            continue
        if method == 0:
            cuts = a + np.concatenate([[0], np.cumsum(sizes[g])])
            kept = oracle.merge_detections([case.rows[cuts[i]:cuts[i + 1]] for i in range(k_inputs)], case.thr)
        else:
            kept = oracle.nms_detections([case.rows[a:b]], case.thr, method == 2, case.cut)
        out[a:a + len(kept)] = kept
        counts[g] = len(kept)
    return out, counts


def input_sizes(case, k_inputs=2):
    """(G, k_inputs) int32: every group's rows split into k_inputs consecutive inputs, the first ones one row longer when it does not divide."""
    n = np.diff(case.offsets)
    return np.stack([n // k_inputs + (i < n % k_inputs) for i in range(k_inputs)], axis=1).astype(np.int32)


def make_case(groups, thr, cut, centre=False, expected=None):
    """Pack per-group row arrays (and, for a closed form, per-group expected kept rows) into a Case."""
    groups = [np.asarray(g, dtype=np.float64).reshape(-1, 5) for g in groups]
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    rows = np.ascontiguousarray(np.concatenate(groups + [np.zeros((0, 5))]))
    case = Case(rows, offsets, float(thr), float(cut), bool(centre), None, None, expected is not None)
    if expected is None:
        exp_rows, exp_counts = reference(case)
    else:
        exp_rows = np.zeros_like(rows)
        exp_counts = np.zeros(len(groups), dtype=np.int64)
        for g, e in enumerate(expected):
            e = np.asarray(e, dtype=np.float64).reshape(-1, 5)
            exp_rows[offsets[g]:offsets[g] + len(e)] = e
            exp_counts[g] = len(e)
    return case._replace(exp_rows=exp_rows, exp_counts=exp_counts)


def single_groups(case):
    """The groups of a case as cases of their own (same parameters, same expectation)."""
    out = []
    for g in range(len(case.offsets) - 1):
        a, b = int(case.offsets[g]), int(case.offsets[g + 1])
        out.append(case._replace(rows=np.ascontiguousarray(case.rows[a:b]), offsets=np.array([0, b - a], dtype=np.int64),
                                 exp_rows=np.ascontiguousarray(case.exp_rows[a:b]), exp_counts=case.exp_counts[g:g + 1].copy()))
    return out


def same_bits(a, b):
    """Exact equality that tells -0.0 from 0.0 (np.array_equal does not); NaN equals NaN whatever its payload."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry the dependency-free form cannot assume

ORDINARY = 7


def ordinary_boxes():
    """Seven boxes that all overlap each other with IoUs that are no dyadic fractions: box k = [0.95 - 0.1 k, 100 + 7 k, 50 + 3 k, 60 + k, 40 - k]."""
    k = np.arange(float(ORDINARY))
    return np.stack([0.95 - 0.1 * k, 100 + 7 * k, 50 + 3 * k, 60 + k, 40 - k], axis=1)


_TINY = 1e-200          # _TINY * _TINY underflows to 0; at the origin x2 - x1 = _TINY exactly (no absorption into a larger coordinate)
_HUGE = 1e200           # _HUGE * _HUGE overflows to inf
_IN = (120.0, 60.0, 30.0, 30.0)       # a box inside the ordinary cluster


def _replace(col, v):
    b = list(_IN)
    b[col] = v
    return tuple(b)


# name -> the special boxes [x, y, w, h] of the set.  Which of them the reference drops (by the contract above):
#   two zero-area boxes, wherever they lie: inter = 0, union = (0 - 0) + 0 = 0, IoU = 0 / 0 = NaN: the lower-ranked one is dropped, so of
#     m zero-area boxes only the best survives; one zero-area box alone meets unions >= the other area > 0 and survives;
#   w, h > 0 whose product underflows: two identical ones have inter = area = 0 like the above although x2 > x1 and y2 > y1;
#   a non-finite coordinate: a corner is NaN (inf - inf where the input is infinite), so the box's area is NaN: it is dropped by the
#     first box ranked above it, and when it is the best box it drops EVERY box ranked below it.  The exception is an infinite w or h in
#     the centre form: x1, x2 = -inf, +inf (or the reverse), area = +-inf, every IoU is +-0 and nothing is dropped;
#   an area that overflows to inf: against finite boxes union = inf, IoU = 0: harmless alone; two such overlapping boxes have
#     inter = inf, union = (inf - inf) + inf = NaN;
#   a negative extent: x2 < x1, so w clamps to 0 and inter = 0 against everything; area = w * h < 0 (> 0 when both are negative) and
#     union = area_j + area_i is 0 exactly when the areas cancel: IoU = 0 / 0 = NaN.
SPECIAL_SETS = collections.OrderedDict([
    ('zero2_far', [(300., 300., 0., 10.), (500., 100., 0., 30.)]),
    ('zero3_far', [(300., 300., 0., 10.), (500., 100., 0., 30.), (700., 50., 20., 0.)]),
    ('zero2_same', [(120., 60., 0., 0.)] * 2),
    ('zero3_same', [(120., 60., 0., 0.)] * 3),
    ('zero_w_vs_zero_h', [(120., 60., 0., 10.), (130., 70., 10., 0.)]),
    ('zero1', [(120., 60., 0., 10.)]),
    ('underflow1', [(0., 0., _TINY, _TINY)]),
    ('underflow2', [(0., 0., _TINY, _TINY)] * 2),
    ('overflow1', [(120., 60., _HUGE, _HUGE)]),
    ('overflow2', [(120., 60., _HUGE, _HUGE), (130., 70., _HUGE, _HUGE)]),
    ('neg_w', [(120., 60., -4., 5.)]),
    ('neg_h', [(120., 60., 4., -5.)]),
    ('neg_both', [(120., 60., -4., -5.)]),
    ('neg_cancel', [(120., 60., -4., 5.), (300., 300., 4., 5.)]),
    ('neg_cancel_reversed', [(300., 300., 4., 5.), (120., 60., -4., 5.)]),
] + [('%s_%s' % (vn, cn), [_replace(c, v)]) for vn, v in (('nan', NAN), ('pinf', INF), ('ninf', -INF))
     for c, cn in enumerate(('x', 'y', 'w', 'h'))])

POSITIONS = (0, 3, 6)        # ordinary boxes ranked above the special ones: top, middle, bottom of the ranking (one ordinary box still follows)


def special_group(name, position):
    """The seven ordinary boxes plus the special set `name`, whose scores put it right after `position` ordinary boxes (special q gets
    ordinary score[position] + 0.04 - 0.01 q: below ordinary box position - 1, above box position, tie-free)."""
    rows = ordinary_boxes()
    base = rows[position, 0]
    sp = [(base + 0.04 - 0.01 * q,) + tuple(b) for q, b in enumerate(SPECIAL_SETS[name])]
    return np.concatenate([rows, np.asarray(sp, dtype=np.float64)])


def bad_geometry(name, centre=False):
    """One special set at the top, in the middle and at the bottom of the ranking (three groups), thr 0.5, cut 0.9: ordinary boxes ranked
    after a special box change score, or leave, with it.  Expected: soft_nms_ref."""
    return make_case([special_group(name, p) for p in POSITIONS], 0.5, 0.9, centre)


ISSUE_TABLE_COUNTS = (2, 1, 1, 1, 1)


def issue_table():
    """Five tiny groups, thr 0.5, cut 0.9.  Closed form, by the rules above SPECIAL_SETS:
      [.9,10,10,20,20] [.8,100,100,0,30] [.7,300,300,0,10]: the first zero-area box meets only the ordinary one (IoU 0 / 400 = 0, weight 1)
        and stays; the second meets the first zero-area box (0 / 0): dropped.  2 rows, scores untouched.
      [.9,10,10,0,0] [.8,10,10,0,0]: 0 / 0: 1 row.
      [.9,10,10,inf,20] ...: cx = inf, x1 = inf - inf = NaN: the best box has a NaN area and drops both others: 1 row, [.9, NaN, 10, NaN, 20].
      the same with w = NaN: the same row.
      [.9,10,10,-4,5] [.8,100,100,4,5]: areas -20 and 20, inter 0: union (20 - 0) + -20 = 0: dropped.  1 row; x1 = 8 + 2, x2 = 8 - 2,
        wd = -4, cxo = 8, x = 8 - -4 / 2 = 10: the input row."""
    groups = [[[.9, 10, 10, 20, 20], [.8, 100, 100, 0, 30], [.7, 300, 300, 0, 10]],
              [[.9, 10, 10, 0, 0], [.8, 10, 10, 0, 0]],
              [[.9, 10, 10, INF, 20], [.8, 12, 12, 20, 20], [.7, 500, 500, 5, 5]],
              [[.9, 10, 10, NAN, 20], [.8, 12, 12, 20, 20], [.7, 500, 500, 5, 5]],
              [[.9, 10, 10, -4, 5], [.8, 100, 100, 4, 5]]]
    expected = [[[.9, 10, 10, 20, 20], [.8, 100, 100, 0, 30]],
                [[.9, 10, 10, 0, 0]],
                [[.9, NAN, 10, NAN, 20]],
                [[.9, NAN, 10, NAN, 20]],
                [[.9, 10, 10, -4, 5]]]
    return make_case(groups, 0.5, 0.9, False, expected)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact decay chains (thr = 0.5, cut = 1: weight = (1 - IoU) / 0.5 = 2 (1 - IoU), clamped to [0, 1])

KILLER = (0.0, 0.0, 4.0, 4.0)        # area 16
VICTIM = (0.0, 0.0, 3.0, 4.0)        # area 12, inside KILLER: inter = 12, union = (12 - 12) + 16 = 16, IoU = 3/4, weight = 0.25 / 0.5 = 1/2
CHAIN_LENGTHS = (1, 63, 64, 65, 300)


def chain(k, victim_score=0.5):
    """Row 0 is VICTIM with the lowest score, rows 1 .. k are k copies of KILLER with scores 1 - i / 1024 (i = 0 .. k - 1, all > 0.5).
    Closed form: the copies have IoU 16 / ((16 - 16) + 16) = 1 >= cut with each other: weight (1 - 1) / 0.5 = 0, so the best copy keeps
    its 1.0 and every other copy ends at exactly s * 0 = 0.0, survives (0.0 >= 0) and still halves the victim: the victim is halved k
    times, victim_score * 2^-k (exact: a power of two times the score, as long as it stays representable).  All k + 1 rows are kept,
    copies first.  All x1 are equal, so the x order is the rank order: the victim is the last lane of the last chunk (alone in it for
    k = 64), and with more than 64 equal x1 a chunk boundary falls inside the ties."""
    rows = [(victim_score,) + VICTIM] + [(1.0 - i / 1024.0,) + KILLER for i in range(k)]
    v = victim_score
    for _ in range(k):
        v = v * 0.5
    expected = [(1.0,) + KILLER] + [(0.0,) + KILLER] * (k - 1) + [(v,) + VICTIM]
    return make_case([rows], 0.5, 1.0, False, [expected])


# ---------------------------------------------------------------------------------------------------------------------------------
# group sizes, x order and the interval skip

GROUP_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
FAST_MAX_ROWS = 2048              # kFastThreads * kFastMaxPerThread of ensemble.hip: one row more and the whole call is serial
_PRIME = 1031                     # > 1024 pairs: p -> (p * stride) % _PRIME is one-to-one for every stride in 1 .. 1030


def pairs(n, stride=389):
    """n rows: row i is KILLER (i even) or VICTIM (i odd) of pair p = i // 2, moved to x = 8 * ((p * stride) % 1031): pairs are 8 apart and 4
    wide, so only the two boxes of a pair overlap.  Scores: killer 1 - p / 4096 (> 1/2), victim 1/2 - p / 4096 (> 0 for p <= 1024), tie-free.
    Closed form: rank order = the killers by p, then the victims by p; a killer meets only IoU 0 (weight 1) and keeps its score, a victim is
    halved once by its own killer: (1/2 - p / 4096) / 2, exact.  Every row is kept.  stride 389 scatters the pairs over the x-sorted chunks,
    stride 1 makes the x order the pair order: chunks of 32 whole pairs whose x ranges are pairwise disjoint."""
    i = np.arange(n)
    p = i // 2
    x = 8.0 * ((p * stride) % _PRIME)
    victim = i % 2 == 1
    rows = np.stack([np.where(victim, 0.5, 1.0) - p / 4096.0, x, np.zeros(n), np.where(victim, 3.0, 4.0), np.full(n, 4.0)], axis=1)
    order = np.concatenate([i[~victim], i[victim]])
    expected = rows[order].copy()
    expected[(n + 1) // 2:, 0] = expected[(n + 1) // 2:, 0] * 0.5
    return make_case([rows], 0.5, 1.0, False, [expected])


def touching_killer():
    """66 rows, thr 0.5, cut 1.  63 fillers [0.9 - i / 1024, -1000 + 8 i, 0, 4, 4] (disjoint), T = [1, -4, 0, 4, 4], Q = [0.375, 0, 0, 1, 4],
    V = [0.25, 0, 0, 1, 3].  x order: the fillers, T (64 rows: the first chunk), then Q and V (x1 = 0: the second chunk, its minimum x1 is 0).
    Closed form: T ends at x2 = 0 exactly: it touches Q and V without overlapping (w = 0, inter = 0, IoU = 0, weight min(2, 1) = 1 exactly).
    Q reaches 1 past the chunk's minimum and holds V: inter = 3, union = (3 - 3) + 4, IoU 3/4: V is halved once, 0.125; nothing else changes."""
    fill = [(0.9 - i / 1024.0, -1000.0 + 8 * i, 0.0, 4.0, 4.0) for i in range(63)]
    t, q = (1.0, -4.0, 0.0, 4.0, 4.0), (0.375, 0.0, 0.0, 1.0, 4.0)
    rows = [(0.25, 0.0, 0.0, 1.0, 3.0), q] + fill + [t]
    expected = [t] + fill + [q, (0.125, 0.0, 0.0, 1.0, 3.0)]
    return make_case([rows], 0.5, 1.0, False, [expected])


def far_killer():
    """102 rows, thr 0.5, cut 1.  K = [1, 0, 0, 256, 4], 100 fillers [0.9 - i / 1024, 0.5 + i / 2, 100 + 10 i, 1, 1] (1 x 1 boxes 10 apart in y,
    far below K) and V = [0.25, 64, 0, 192, 4].  x order: K, the fillers (x1 up to 50), V: the victim's only killer sits in the first chunk,
    the victim in the second.  Closed form: V lies inside K: inter = 768, union = (768 - 768) + 1024, IoU 3/4: V is halved once, 0.125;
    every other pair is disjoint in y."""
    k = (1.0, 0.0, 0.0, 256.0, 4.0)
    fill = [(0.9 - i / 1024.0, 0.5 + i / 2.0, 100.0 + 10 * i, 1.0, 1.0) for i in range(100)]
    rows = fill[:50] + [(0.25, 64.0, 0.0, 192.0, 4.0)] + fill[50:] + [k]
    expected = [k] + fill + [(0.125, 64.0, 0.0, 192.0, 4.0)]
    return make_case([rows], 0.5, 1.0, False, [expected])


def sliding_rows(m):
    """S = [1, 0, 0, 256, 4] and m windows V_i = [0.9 - i / 1024, i, 0, 192, 4] inside it (m <= 65): S overlaps every chunk with IoU exactly 3/4,
    the windows overlap each other with IoU (192 - d) / (192 + d)."""
    return [(1.0, 0.0, 0.0, 256.0, 4.0)] + [(0.9 - i / 1024.0, float(i), 0.0, 192.0, 4.0) for i in range(m)]


def spanning_killer():
    """66 rows (sliding_rows(65)), thr 0.5, cut 1: one killer spans both chunks, and the windows of the second chunk are decayed by windows
    of the first.  The weights among the windows are no dyadic fractions.  Expected: soft_nms_ref."""
    return make_case([sliding_rows(65)], 0.5, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# score ties

TIE_ROWS, TIE_BLOCK = 320, 48
TIE_DUPLICATES = ((60, 68), (250, 260))       # inclusive row ranges made identical: across lane 63 | 64 and across thread 255 | 256


def ties():
    """320 disjoint 4 x 4 boxes at x = 8 i with scores in blocks of 48 equal values, 1 - (i // 48) / 16 (blocks straddle rows 64 and 256),
    rows 60 .. 68 and 250 .. 260 made exact copies of rows 60 and 250 (each range lies inside one block).  thr 0.5, cut 1.
    Closed form: rank order = blocks by descending score, inside a block the HIGHER input index first.  Disjoint boxes keep their scores;
    among exact copies (IoU 1 >= cut, weight 0) the first ranked = the highest index keeps its score, the others end at exactly 0.0."""
    i = np.arange(TIE_ROWS)
    rows = np.stack([1.0 - (i // TIE_BLOCK) / 16.0, 8.0 * i, np.zeros(TIE_ROWS), np.full(TIE_ROWS, 4.0), np.full(TIE_ROWS, 4.0)], axis=1)
    final = rows[:, 0].copy()
    for lo, hi in TIE_DUPLICATES:
        assert lo // TIE_BLOCK == hi // TIE_BLOCK
        rows[lo:hi + 1] = rows[lo]
        final[lo:hi] = 0.0
    order = np.lexsort((-i, i // TIE_BLOCK))
    expected = rows[order].copy()
    expected[:, 0] = final[order]
    return make_case([rows], 0.5, 1.0, False, [expected])


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch edges and the mixed launch

DISPATCH_EDGES = collections.OrderedDict([          # name -> (thr, cut) at and beyond the launch condition `thr >= 0 && cut > thr`
    ('thr_zero', (0.0, 0.9)),                       # the last thr that still launches the dependency-free form
    ('thr_negative', (-0.1, 0.9)),
    ('cut_equals_thr', (0.75, 0.75)),               # weights +inf -> 1, -inf -> 0, and 0 / 0 = NaN for the pair with IoU == cut: dropped
    ('cut_below_thr', (0.9, 0.5)),
    ('cut_infinite', (0.5, INF)),                   # (inf - IoU) / (inf - thr) = NaN for every pair: only the best box of a group stays
])


def nested_pair():
    return [(0.9,) + KILLER, (0.8,) + VICTIM]


def dispatch_edge(name):
    """Three groups under the (thr, cut) of DISPATCH_EDGES: the ordinary boxes, S with 20 windows, and a KILLER / VICTIM pair (IoU exactly 3/4).
    Expected: soft_nms_ref."""
    thr, cut = DISPATCH_EDGES[name]
    return make_case([ordinary_boxes(), sliding_rows(20), nested_pair()], thr, cut)


def mixed_launch():
    """One call, thr 0.5, cut 1: empty groups, groups the dependency-free form may take, groups with a NaN or a negative score and groups with
    the geometry of SPECIAL_SETS, interleaved.  Expected: soft_nms_ref per group = each group's result when it runs alone."""
    nan_score = ordinary_boxes(); nan_score[2, 0] = NAN
    neg_score = ordinary_boxes(); neg_score[4, 0] = -0.25
    groups = [np.zeros((0, 5)), pairs(65).rows, nan_score, np.zeros((0, 5)), special_group('zero2_far', 0), chain(5).rows, neg_score,
              sliding_rows(30), special_group('nan_w', 3), np.zeros((0, 5)), touching_killer().rows, special_group('neg_cancel', 6),
              pairs(257, 1).rows, special_group('underflow2', 0), ordinary_boxes(), special_group('overflow2', 3), np.zeros((0, 5))]
    return make_case(groups, 0.5, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# registry

def _registry():
    c = collections.OrderedDict()
    for name in SPECIAL_SETS:
        c['bad_%s' % name] = (lambda name=name: bad_geometry(name, False))
        c['bad_%s_centre' % name] = (lambda name=name: bad_geometry(name, True))
    c['issue_table'] = issue_table
    for k in CHAIN_LENGTHS:
        c['chain_%d' % k] = (lambda k=k: chain(k))
    c['chain_zero_score'] = lambda: chain(3, 0.0)
    c['chain_negative_zero_score'] = lambda: chain(3, -0.0)
    c['chain_subnormal_score'] = lambda: chain(4, 2.0 ** -1070)           # ends at 2^-1074, the smallest subnormal
    c['chain_subnormal_to_zero'] = lambda: chain(5, 2.0 ** -1070)         # one more halving: 2^-1075 is a tie and rounds to even, 0.0
    for n in GROUP_SIZES:
        c['pairs_%d' % n] = (lambda n=n: pairs(n))
    c['pairs_600'] = lambda: pairs(600)
    c['pairs_65_disjoint_chunks'] = lambda: pairs(65, 1)
    c['pairs_257_disjoint_chunks'] = lambda: pairs(257, 1)
    c['touching_killer'] = touching_killer
    c['far_killer'] = far_killer
    c['spanning_killer'] = spanning_killer
    c['ties'] = ties
    for name in DISPATCH_EDGES:
        c['dispatch_%s' % name] = (lambda name=name: dispatch_edge(name))
    c['mixed_launch'] = mixed_launch
    return c


CASES = _registry()
BAD_GEOMETRY = tuple(n for n in CASES if n.startswith('bad_'))
_built = {}


def get(name):
    """The case `name`, built once per process.  Treat it as read-only."""
    if name not in _built:
        case = CASES[name]()
        for a in (case.rows, case.offsets, case.exp_rows, case.exp_counts):
            a.setflags(write=False)
        _built[name] = case
    return _built[name]


def iou_exact(a, b):
    """IoU of two [x, y, w, h] boxes with integer (or dyadic) coordinates in exact rational arithmetic."""
    ax, ay, aw, ah = (Fraction(v) for v in a)
    bx, by, bw, bh = (Fraction(v) for v in b)
    iw = max(min(ax + aw, bx + bw) - max(ax, bx), 0)
    ih = max(min(ay + ah, by + bh) - max(ay, by), 0)
    return iw * ih / (aw * ah + bw * bh - iw * ih)
