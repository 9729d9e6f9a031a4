"""Pure-Python helpers of tests/test_gpu_roi_edges.py (no device needed: tests/test_roi_cases.py runs them on the CPU).

1. The launch rules of wd_roi_pool_fpn_f32 (csrc/det_roialign.hip), restated.  If a launch rule changes, the restatement here changes with
   it (the GPU tests assert the predicted route and per-ROI paths before every launch).

     route:   pooled != 7                                  -> 'per-sample'          roi_pool_fpn_kernel alone
              C % 4 == 0 and out 16-byte aligned           -> 'workgroup'           roi_pool_wg_kernel, for 64 <= n <= 8192 behind
                                                              'workgroup+ordered'   roi_bucket_order_kernel
              otherwise                                    -> 'separable+flagged'   roi_pool_sep_kernel, then roi_pool_fpn_kernel on the
                                                                                    ROIs it flagged
     per ROI (float32 geometry of the kernels: r_lo, r_hi, q_lo, q_hi, the per-axis weight tables, first / last bin per column):
              footprint beyond the 64 x 64 tables (or empty) -> 'direct'  (the separable kernel flags exactly these ROIs)
              a column feeds bins more than 2 apart          -> 'dense'   (any_wide; the separable kernel always folds densely)
              otherwise                                      -> 'fold'    (sliding 3-bin window)

2. Dyadic ROIs.  With x1 * scale - 0.5 and the bin size dyadic - bins m / 4 <= 1 (one sample per bin) or an integer b (b samples per bin and
   axis) - every sample coordinate, bilinear weight and weighted sum of the small-integer features (|f| <= 8) is exact in float32, whatever
   the order of the operations and whatever FMA contraction does.  The expected output is then known bit for bit; where gh * gw is not a
   power of two the final division may round, and those rows are compared within one float32 ulp.  Expected values come from
   oracle/detops_ref.roi_pool_fpn on 8 channels; channel c of a wider feature map is a signed copy of base channel channel_source(c).
"""
import functools
import math
import types
from fractions import Fraction

import numpy as np
import torch

F = np.float32
STRIDES = (4, 8, 16, 32)
SCALES = tuple(1.0 / s for s in STRIDES)
MIN_LEVEL, CANONICAL_LEVEL, CANONICAL_SIZE = 2, 4, 224.0
K_MAX_FOOT = 64                    # kMaxFoot
QB = 8                             # kRoiQB
ORDER_MIN, ORDER_MAX = 64, 8192
BATCH = 2
BASE_C = 8
MAX_SAMPLES_OTHER_P = 4000         # pooled != 7: cases with more samples per ROI stay out (the reference is a Python loop per sample)


# ---------------------------------------------------------------------------------------------------------------------------------
# launch rules

def route(n, channels, pooled, out_aligned=True):
    if pooled != 7:
        return 'per-sample'
    if channels % 4 == 0 and out_aligned:
        return 'workgroup+ordered' if ORDER_MIN <= n <= ORDER_MAX else 'workgroup'
    return 'separable+flagged'


def level_index(roi, n_levels=4):
    """Index of the FPN level (0 = min_level) in the kernels' float32 arithmetic.  A negative area gives NaN, which the device's
    float -> int conversion turns into 0, below min_level."""
    x1, y1, x2, y2 = (F(v) for v in roi[1:5])
    with np.errstate(all='ignore'):
        size = np.sqrt(F((x2 - x1) * (y2 - y1)))
        v = F(CANONICAL_LEVEL) + np.log2(F(F(size / F(CANONICAL_SIZE)) + F(1e-8)))
    lvl = 0 if np.isnan(v) else int(math.floor(float(v)))
    return min(max(lvl, MIN_LEVEL), MIN_LEVEL + n_levels - 1) - MIN_LEVEL


def _low_index(v, n):
    if v <= 0:
        v = F(0)
    l = int(v)
    return n - 1 if l >= n - 1 else l


def _sample(start, bin_, g, p, i):
    return F(F(start + F(F(p) * bin_)) + F(F(F(F(i) + F(.5)) * bin_) / F(g)))


def _axis(start, bin_, g, n_pix, pooled):
    """One axis of a ROI: footprint [lo, hi], the samples of every bin and, where the footprint fits the tables, the weight rows."""
    gg = g if g > 0 else 1
    lo = _low_index(F(start + F(F(.5) * bin_) / F(gg)), n_pix)
    last = F(F(start + F(F(pooled - 1) * bin_)) + F(F(F(F(g - 1 if g > 0 else 0) + F(.5)) * bin_) / F(gg)))
    hi = min(_low_index(last, n_pix) + 1, n_pix - 1)
    n = hi - lo + 1
    samples = [[_sample(start, bin_, g, p, i) for i in range(max(g, 0))] for p in range(pooled)]
    ax = types.SimpleNamespace(lo=lo, hi=hi, n=n, samples=samples, table=None, first=None, last=None)
    if 1 <= n <= K_MAX_FOOT:
        table = [[Fraction(0)] * n for _ in range(pooled)]
        first, last_ = [K_MAX_FOOT] * pooled, [-1] * pooled
        for p in range(pooled):
            for v in samples[p]:
                if v < -1.0 or v > n_pix:
                    continue
                v = max(float(v), 0.0)
                l = int(v)
                if l >= n_pix - 1:
                    h = l = n_pix - 1
                    v = float(l)
                else:
                    h = l + 1
                assert 0 <= l - lo < n and 0 <= h - lo < n, 'weight row written outside the footprint'
                fl = Fraction(v) - l
                table[p][l - lo] += 1 - fl
                table[p][h - lo] += fl
                first[p], last_[p] = min(first[p], l - lo), max(last_[p], h - lo)
        ax.table, ax.first, ax.last = table, first, last_
    return ax


def geometry(roi, maps, pooled=7):
    """The float32 geometry the three kernels derive from a ROI, and the path it takes.  maps: (H, W) per level."""
    li = level_index(roi, len(maps))
    h, w = maps[li]
    s = F(SCALES[li])
    x1, y1, x2, y2 = (F(v) for v in roi[1:5])
    rsw, rsh = F(x1 * s - F(.5)), F(y1 * s - F(.5))
    rew, reh = F(x2 * s - F(.5)), F(y2 * s - F(.5))
    roi_w, roi_h = F(rew - rsw), F(reh - rsh)
    bin_h, bin_w = F(roi_h / F(pooled)), F(roi_w / F(pooled))
    gh, gw = int(math.ceil(float(bin_h))), int(math.ceil(float(bin_w)))
    ya, xa = _axis(rsh, bin_h, gh, h, pooled), _axis(rsw, bin_w, gw, w, pooled)
    g = types.SimpleNamespace(level=li, h=h, w=w, gh=gh, gw=gw, count=max(gh * gw, 1), bin_h=float(bin_h), bin_w=float(bin_w),
                              r_lo=ya.lo, r_hi=ya.hi, q_lo=xa.lo, q_hi=xa.hi, nrows=ya.n, ncols=xa.n, y=ya, x=xa,
                              image_ok=0 <= int(roi[0]) < BATCH)
    g.over = g.nrows > K_MAX_FOOT or g.ncols > K_MAX_FOOT or g.nrows < 1 or g.ncols < 1
    g.col_pa, g.spread = None, 0
    if not g.over:
        g.col_pa = []
        for q in range(g.ncols):
            fed = [p for p in range(pooled) if xa.table[p][q] != 0]
            g.col_pa.append(fed[0] if fed else pooled)
            if fed:
                g.spread = max(g.spread, fed[-1] - fed[0])
    g.path = 'none' if not g.image_ok else 'direct' if g.over else 'dense' if g.spread > 2 else 'fold'
    g.sep_path = 'none' if not g.image_ok else 'flagged' if g.over else 'table'
    return g


def tail_form(ncols):
    """The column block that ends a row pass of the workgroup kernel."""
    rem = ncols % QB
    return 'full' if rem == 0 else 'partial' if rem > QB // 2 else 'half'


def facts(g):
    """Tags of what a ROI's geometry makes the kernels do (derived, not intended: tests/test_roi_cases.py holds the two together)."""
    t = set()
    if not g.image_ok:
        return {'image:outside-batch'}
    t.add('path:' + g.path)
    t.add('level:%d' % g.level)
    if g.gh != g.gw:
        t.add('bins:mixed')
    for ax, n_pix, name in ((g.y, g.h, 'rows'), (g.x, g.w, 'cols')):
        flat = [v for p in ax.samples for v in p]
        if any(v == -1.0 for v in flat):
            t.add('border:sample-at-minus-one')
        if any(v < -1.0 for v in flat) and any(v >= -1.0 for v in flat):
            t.add('border:sample-below-minus-one')
        if any(v == n_pix for v in flat) and any(v > n_pix for v in flat):
            t.add('border:sample-at-limit-then-beyond')
        inside = [[v for v in p if -1.0 <= v <= n_pix] for p in ax.samples]
        if flat and any(not p for p in inside) and any(inside):
            t.add('border:empty-bins')
        if flat and not any(inside):
            t.add('border:outside')
        if n_pix <= 2:
            t.add('border:map-of-%d' % n_pix)
        if ax.n == K_MAX_FOOT:
            t.add('limit:%s-64' % name)
        if ax.n > K_MAX_FOOT:
            t.add('limit:%s-over' % name)
    if g.nrows == K_MAX_FOOT and g.ncols == K_MAX_FOOT:
        t.add('limit:both-64')
    if g.nrows > K_MAX_FOOT and g.ncols > K_MAX_FOOT:
        t.add('limit:both-over')
    if g.path in ('fold', 'dense'):
        t.add('tail:' + tail_form(g.ncols))
        if g.ncols >= QB:
            t.add('tail:after-full-blocks')
        for f, l in zip(g.y.first, g.y.last):
            if l >= f:
                t.add('rows:odd' if (l - f + 1) % 2 else 'rows:even')
        if any(pa == 7 for pa in g.col_pa):
            t.add('cols:no-weight')
        if g.path == 'fold' and g.spread == 2:
            t.add('fold:three-bins')
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes and cases

SCENES = {
    'main': ((67, 75), (80, 61), (59, 80), (80, 80)),
    'tiny': ((1, 9), (2, 2), (7, 1), (1, 1)),
}


def dyadic_roi(image, level, sy, sx, bh, bw, pooled=7):
    """The ROI whose first bin starts at feature coordinates (sy, sx) of `level` (before the half-pixel shift is undone) with bins bh x bw."""
    s = STRIDES[level]
    x1, y1 = (sx + .5) * s, (sy + .5) * s
    return (float(image), x1, y1, x1 + pooled * bw * s, y1 + pooled * bh * s)


def _pick_level(sy, sx, bh, bw, pooled, prefer):
    """The level a dyadic ROI is built for must be the level its size assigns it to: the preferred one if that is consistent."""
    for level in [prefer] + [l for l in range(4) if l != prefer]:
        if level_index(dyadic_roi(0, level, sy, sx, bh, bw, pooled)) == level:
            return level
    raise AssertionError('no consistent level for bins %s x %s, pooled %d' % (bh, bw, pooled))


def _specs():
    """(scene, name, intent tags, spec): spec = ('dyadic', level, sy, sx, bh, bw) or ('abs', x1, y1, x2, y2), image index chosen by position."""
    out = []

    def dy(scene, name, tags, level, sy, sx, bh, bw):
        out.append((scene, name, set(tags), ('dyadic', level, sy, sx, bh, bw)))

    def ab(scene, name, tags, *box):
        out.append((scene, name, set(tags), ('abs',) + box))

    # placement x bins: integer sample coordinates (start k - 0.5: the high neighbour of every sample has weight 0, the footprint ends in a
    # zero-weight column) and half-integer ones; 7 b + 1 footprint columns = 8, 15, 29, 57: tail forms full, partial (7 and 5 valid), half
    mixed = [(1, 1, 0), (1, 2, 0), (2, 1, 0), (2, 2, 1), (4, 1, 2), (1, 4, 1), (2, 4, 2), (4, 2, 0), (8, 1, 1), (1, 8, 2), (4, 4, 3), (8, 2, 3),
             (2, 8, 3), (8, 4, 3), (4, 8, 3), (8, 8, 3)]
    for i, (bh, bw, level) in enumerate(mixed):
        for place, shift in (('integer', -.5), ('half', 0.)):
            dy('main', 'bins %dx%d %s' % (bh, bw, place), ['place:' + place, 'bin:%d' % bh, 'bin:%d' % bw], level,
               1 + i % 3 + shift, 2 + i % 4 + shift, bh, bw)
    # table limit: bin 9 -> 64 footprint rows / columns (the largest the tables take), bin 10 -> 71 (direct)
    for bh, bw, level, tag in [(9, 1, 1, 'rows-64'), (10, 1, 1, 'rows-over'), (1, 9, 2, 'cols-64'), (1, 10, 2, 'cols-over'), (9, 9, 3, 'both-64'),
                               (10, 10, 3, 'both-over'), (9, 10, 3, 'cols-over'), (10, 9, 3, 'rows-over')]:
        for place, shift in (('integer', -.5), ('half', 0.)):
            dy('main', 'limit %dx%d %s' % (bh, bw, place), ['limit:' + tag, 'place:' + place], level, 3 + shift, 2 + shift, bh, bw)
    # bin 10 on a map it overhangs: the clamps shrink the footprint to 59 rows, back into the tables, with the last bin row left out
    dy('main', 'limit 10x1 clamped', ['border:empty-bins', 'path:fold'], 0, 8., 6., 10, 1)
    # narrow bins: 0.75 -> a column feeds exactly three bins (fold); 0.5 and 0.25 -> four or more (dense)
    for bh, bw, tags in [(.75, .75, ['fold:three-bins']), (.75, 2, ['path:fold']), (2, .75, ['fold:three-bins']), (.5, .5, ['path:dense']),
                         (.25, .25, ['path:dense']), (.5, 4, ['path:fold']), (4, .5, ['path:dense']), (1, .25, ['path:dense']),
                         (.25, 8, ['path:fold']), (8, .25, ['path:dense'])]:
        for k, (sy, sx) in enumerate([(10., 12.), (5.5, 7.5), (20.25, 3.125)]):
            dy('main', 'narrow %sx%s #%d' % (bh, bw, k), tags, 0, sy, sx, bh, bw)
    # borders of the level-2 map (67 x 75) and of the level-4 map (59 x 80)
    dy('main', 'first sample at -1', ['border:sample-at-minus-one'], 0, -1.5, -1.5, 1, 1)
    dy('main', 'first sample at -1, bins 2x4', ['border:sample-at-minus-one'], 2, -1.5, -1.5, 2, 4)
    dy('main', 'first sample at -1.5', ['border:sample-below-minus-one'], 1, -2., -2., 2, 2)
    dy('main', 'first bins below -1', ['border:empty-bins'], 0, -4.5, -3.5, 1, 1)
    dy('main', 'sample at W and H', ['border:sample-at-limit-then-beyond', 'border:empty-bins'], 0, 67 - 3.5, 75 - 3.5, 1, 1)
    dy('main', 'sample at W', ['border:sample-at-limit-then-beyond'], 0, 20., 75 - 4.5, 1, 2)
    dy('main', 'sample at H', ['border:sample-at-limit-then-beyond'], 2, 59 - 6.5, 30., 2, 4)
    dy('main', 'sample at W - 0.5', [], 0, 67 - 4., 75 - 4., 1, 1)
    dy('main', 'last sample at W and H, none beyond', [], 0, 67 - 6.5, 75 - 6.5, 1, 1)
    dy('main', 'outside right', ['border:outside'], 0, 10., 75 + 5., 1, 1)
    dy('main', 'outside below', ['border:outside'], 1, 80 + 1.5, 10., 2, 2)
    dy('main', 'outside left above', ['border:outside'], 0, -30., -30., 2, 1)
    dy('main', 'just outside: first sample at W + 1', ['border:outside'], 0, 10., 75 + .5, 1, 1)
    dy('main', 'covers the whole map', ['border:empty-bins'], 3, -12., -12., 8, 8)
    dy('main', 'whole map and beyond, direct', ['path:direct', 'border:empty-bins'], 3, -13., -13., 12, 12)
    # level edges: sqrt(w h) exactly 112, 224, 448 (the upper level takes the box), squares and elongated boxes
    for edge, level, boxes in [(112, 1, [(20, 28, 132, 140), (20, 12, 76, 236), (12, 20, 236, 76), (36, 4, 64, 452)]),
                               (224, 2, [(24, 32, 248, 256), (24, 8, 136, 456), (8, 24, 456, 136), (40, 8, 96, 904)]),
                               (448, 3, [(16, 48, 464, 496), (16, 16, 240, 912), (16, 16, 912, 240), (48, 16, 160, 1808)])]:
        for box in boxes:
            ab('main', 'level edge %d: %dx%d' % (edge, box[2] - box[0], box[3] - box[1]), ['edge:%d' % edge, 'level:%d' % level], *box)
    # degenerate boxes
    dy('main', 'empty box', ['degenerate:empty'], 0, 9.5, 9.5, 0, 0)
    dy('main', 'zero width', ['degenerate:empty'], 0, 9.5, 9.5, 1, 0)
    dy('main', 'negative width', ['degenerate:negative'], 0, 4.5, 14.5, 1, -1)
    dy('main', 'negative width and height', ['degenerate:negative'], 0, 11.5, 14.5, -1, -1)
    # image index (position in the list decides 0 / 1 elsewhere)
    for image in (0, 1, -1, 2):
        out.append(('main', 'image %d' % image, {'image:%d' % image}, ('dyadic', 1, 6., 9., 2, 2, image)))
    # maps with H or W of 1 and 2
    dy('tiny', 'H = 1', ['border:map-of-1', 'border:sample-at-minus-one'], 0, -1.5, 1.5, 1, 1)
    dy('tiny', 'H = 1 half', ['border:map-of-1'], 0, -1., 2., 1, 1)
    dy('tiny', 'H = 1 narrow', ['border:map-of-1'], 0, -.5, 3., .25, .75)
    dy('tiny', '2 x 2', ['border:map-of-2'], 1, -1.5, -1.5, 2, 2)
    dy('tiny', '2 x 2 half', ['border:map-of-2'], 1, -3., -2., 2, 2)
    dy('tiny', 'W = 1', ['border:map-of-1'], 2, -.5, -1.5, 2, 2)
    dy('tiny', 'W = 1 tall', ['border:map-of-1'], 2, -1., -5., 1, 4)
    dy('tiny', '1 x 1', ['border:map-of-1'], 3, -1.5, -1.5, 4, 4)
    dy('tiny', '1 x 1 around', ['border:map-of-1'], 3, -8., -8., 4, 4)
    return out


REQUIRED_INTENTS = (['place:integer', 'place:half', 'bin:1', 'bin:2', 'bin:4', 'bin:8', 'limit:rows-64', 'limit:rows-over', 'limit:cols-64',
                     'limit:cols-over', 'limit:both-64', 'limit:both-over', 'edge:112', 'edge:224', 'edge:448', 'degenerate:empty',
                     'degenerate:negative', 'image:0', 'image:1', 'image:-1', 'image:2'])
REQUIRED_FACTS = (['path:fold', 'path:dense', 'path:direct', 'bins:mixed', 'tail:full', 'tail:partial', 'tail:half', 'tail:after-full-blocks',
                   'rows:odd', 'rows:even', 'cols:no-weight', 'fold:three-bins', 'border:sample-at-minus-one', 'border:sample-below-minus-one',
                   'border:sample-at-limit-then-beyond', 'border:empty-bins', 'border:outside', 'border:map-of-1', 'border:map-of-2',
                   'limit:rows-64', 'limit:rows-over', 'limit:cols-64', 'limit:cols-over', 'limit:both-64', 'limit:both-over', 'level:0',
                   'level:1', 'level:2', 'level:3', 'image:outside-batch'])
# intents that are facts of the same name: the case's geometry must show them
CHECKED_INTENTS = ('path:', 'fold:', 'border:', 'limit:', 'level:')


def is_dyadic(roi, pooled):
    """Exact arithmetic: do the bins of this ROI stay m / 4 <= 1 or integer (or empty) with `pooled` bins per axis?"""
    li = level_index(roi)
    for a, b in ((roi[1], roi[3]), (roi[2], roi[4])):
        start = Fraction(a) / STRIDES[li] - Fraction(1, 2)
        bin_ = (Fraction(b) - Fraction(a)) / STRIDES[li] / pooled
        if (start * 8).denominator != 1:
            return False
        if bin_ > 1 and bin_.denominator != 1:
            return False
        if 0 < bin_ <= 1 and (bin_ * 4).denominator != 1:
            return False
    return True


@functools.lru_cache(maxsize=None)
def cases(scene, pooled=7):
    """The distinct ROIs of a scene -> list of namespaces (name, intents, roi, geom, facts).  pooled != 7 rebuilds the dyadic specs with
    that factor (on the level the new size assigns) and keeps the cases whose bins stay dyadic and cheap for the reference."""
    out = []
    for k, (sc, name, intents, spec) in enumerate(_specs()):
        if sc != scene:
            continue
        image = k % BATCH
        if spec[0] == 'dyadic':
            level, sy, sx, bh, bw = spec[1:6]
            if len(spec) > 6:
                image = spec[6]
            picked = _pick_level(sy, sx, bh, bw, pooled, level)
            roi = dyadic_roi(image, picked, sy, sx, bh, bw, pooled)
            if pooled == 7:
                assert picked == level, (name, picked, level)
        else:
            roi = (float(image),) + tuple(float(v) for v in spec[1:])
        if not is_dyadic(roi, pooled):
            assert pooled != 7, name
            continue
        g = geometry(roi, SCENES[scene], pooled)
        if pooled != 7 and g.gh * g.gw * pooled * pooled > MAX_SAMPLES_OTHER_P:
            continue
        out.append(types.SimpleNamespace(name=name, intents=intents, roi=roi, geom=g, facts=facts(g) if pooled == 7 else set()))
    return out


def rois_of(cs):
    return torch.tensor([c.roi for c in cs], dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# features and expected values

def channel_source(c):
    """(base channel, sign) behind channel c of a wide feature map: neighbours, channels 4, 8, 64 and 256 apart all differ, so a kernel
    that reads or writes a wrong lane, wave or 256-channel round gives a wrong value.  Channels 0..7 are the base itself."""
    return (c + c // 8 + c // 64 + c // 256) % BASE_C, -1.0 if (c // 8) % 2 else 1.0


@functools.lru_cache(maxsize=None)
def base_features(scene):
    """Per level (BATCH, 8, H, W) float32 of integers in [-8, 8]."""
    g = torch.Generator().manual_seed(sum(h * 131 + w for h, w in SCENES[scene]))
    return [torch.randint(-8, 9, (BATCH, BASE_C, h, w), generator=g).float() for h, w in SCENES[scene]]


def wide_features(scene, channels):
    """Per level (BATCH, H, W, channels) float32, contiguous: the NHWC storage the kernels read."""
    src = torch.tensor([channel_source(c)[0] for c in range(channels)])
    sign = torch.tensor([channel_source(c)[1] for c in range(channels)])
    return [(f[:, src] * sign.view(1, -1, 1, 1)).permute(0, 2, 3, 1).contiguous() for f in base_features(scene)]


def widen(exp, channels):
    """Expected (R, 8, P, P) -> (R, P, P, channels) float32, the kernels' output layout."""
    src = torch.tensor([channel_source(c)[0] for c in range(channels)])
    sign = torch.tensor([channel_source(c)[1] for c in range(channels)], dtype=exp.dtype)
    return (exp[:, src] * sign.view(1, -1, 1, 1)).permute(0, 2, 3, 1).contiguous().float()


@functools.lru_cache(maxsize=None)
def expected(scene, pooled=7):
    """-> (float64 (R, 8, P, P) from oracle/detops_ref.roi_pool_fpn, bool (R,) rows whose division by gh * gw may round).  ROIs whose image
    index lies outside the batch are zeros by the kernels' contract (the reference would index another image)."""
    from oracle import detops_ref as R
    cs = cases(scene, pooled)
    rois = rois_of(cs)
    ok = torch.tensor([c.geom.image_ok for c in cs])
    exp = torch.zeros((len(cs), BASE_C, pooled, pooled), dtype=torch.float64)
    if bool(ok.any()):
        exp[ok] = R.roi_pool_fpn(base_features(scene), rois[ok], list(SCALES), pooled, MIN_LEVEL, CANONICAL_LEVEL, CANONICAL_SIZE)[0]
    rounds = torch.tensor([c.geom.count & (c.geom.count - 1) != 0 for c in cs])
    return exp, rounds


def repeated(n_distinct, n, seed):
    """Row -> distinct ROI for an n-row launch: every distinct ROI repeated, in a fixed random order."""
    g = torch.Generator().manual_seed(seed)
    return (torch.arange(n) % n_distinct)[torch.randperm(n, generator=g)]


# ---------------------------------------------------------------------------------------------------------------------------------
# processing order (roi_bucket_order_kernel)

ORDER_BUCKETS = 2048


def bucket_key(roi, maps):
    """The counting-sort key of a ROI: 2 bits level | 6 bits row band | 3 bits column cell (serpentine)."""
    li = level_index(roi, len(maps))
    h, w = maps[li]
    s = F(SCALES[li])
    x1, y1, x2, y2 = (F(v) for v in roi[1:5])
    cx, cy = F(F(F(.5) * F(x1 + x2)) * s), F(F(F(.5) * F(y1 + y2)) * s)
    cx, cy = (cx if cx > 0 else F(0)), (cy if cy > 0 else F(0))
    band = min(int(F(F(cy * F(64)) / F(max(h, 1)))), 63)
    cell = min(int(F(F(cx * F(8)) / F(max(w, 1)))), 7)
    return ((li & 3) << 9) | (band << 3) | (7 - cell if band & 1 else cell)


def spread_rois(maps):
    """One ROI per (level, row band, column cell): 2048 boxes centred in their cell, of a size that assigns them to their level.  Not
    dyadic: the ordered launch is compared with unordered launches of the same rows, which run the same arithmetic per ROI."""
    rois = []
    for li, (h, w) in enumerate(maps):
        size = (56., 160., 320., 640.)[li]
        for band in range(64):
            for cell in range(8):
                cx, cy = (cell + .5) * w / 8 * STRIDES[li], (band + .5) * h / 64 * STRIDES[li]
                rois.append((float((band + cell) % BATCH), cx - size / 2, cy - size / 2, cx + size / 2, cy + size / 2))
    return rois
