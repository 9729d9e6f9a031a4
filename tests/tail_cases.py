"""Adversarial inputs of the detector tail (csrc/det_tail.hip: rpn_topk_stage_kernel and its host stage plan, sort_candidates_kernel<0>
and <1>, wire_kernel) with their exact answers.  No device code and no project imports: tests/test_tail_cases.py proves every closed
form here on the CPU against plain references (torch's stable float32 sort, a float64 decode, the torch sequence of the box head, the
package's CPU wire branch), tests/test_gpu_tail_edges.py feeds the cases to the kernels.  Every builder is deterministic.

The contract (include/waymodet.h): a selection is the stable descending sort of the float32 scores cut to k, i.e. score descending,
ties (and -0.0 against +0.0) by lower index first, and every NaN - whatever its sign or payload - ahead of +inf in index order,
exactly what torch.sort(descending=True, stable=True) returns.

Identification trick of the top-k: with deltas = 0, anchors[i] = (i, 0, i + 1, 1) and an image at least n + 1 wide and 1 high the
decode returns exactly (i, 0, i + 1, 1) (width (i + 1) - i = 1, centre i + 0.5 * 1, expf(0) = 1, all exact below 2^23), so the output
boxes name the anchor selected in each slot (decode_f32 below is that float32 sequence).
"""
import collections

import numpy as np

F32 = np.float32
CHUNK = 8192                 # keys one workgroup sorts
MAX_STAGES = 24              # stages the host plan of wd_rpn_topk_decode_f32 may use (include/waymodet.h)
MAX_K = 8192
MAX_LEVELS = 8
SCALE_CLAMP = F32(4.135166556742356)


def f32_bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


NANS = f32_bits(0x7fc00000, 0x7fc00001, 0xffc00000, 0xffffffff)
FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = f32_bits(0x00000001)[0]

# the nine-value vector of the issue, its torch order (every NaN first in index order) and the order of the bit-ordered keys
NINE = np.concatenate([f32_bits(0x3f800000, 0x7fc00001, 0x80000000, 0xffc00000, 0x7f800000, 0x00000000, 0x7fc00000, 0xff800000, 0x3f800000)])
NINE_TORCH_ORDER = [1, 3, 6, 4, 0, 8, 2, 5, 7]
NINE_BIT_KEY_ORDER = [1, 6, 4, 0, 8, 2, 5, 7, 3]


def stable_desc_order(x):
    """The contract in numpy: NaNs first in index order, then descending by value, equal values (-0.0 == +0.0) in index order."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    rest = np.nonzero(~nan)[0]
    return np.concatenate([np.nonzero(nan)[0], rest[np.argsort(-x[rest], kind='stable')]]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# host stage plan

def next_n(n, k):
    """Keys of a level after one selection stage: every 8192-chunk keeps its best min(len, k)."""
    chunks = (n + CHUNK - 1) // CHUNK
    last = n - (chunks - 1) * CHUNK
    return (chunks - 1) * k + min(last, k)


def stages_needed(k, n):
    """Launches until the level fits one chunk (that launch included); None when a stage stops shrinking it."""
    stages = 1
    while n > CHUNK:
        m = next_n(n, k)
        if m >= n:
            return None
        n = m
        stages += 1
    return stages


def served(k, sizes):
    """The rule of include/waymodet.h: 1 <= k <= 8192, 1..8 non-empty levels and a plan of at most MAX_STAGES stages."""
    sizes = [sizes] if isinstance(sizes, int) else list(sizes)
    if not (1 <= k <= MAX_K and 1 <= len(sizes) <= MAX_LEVELS and all(n >= 1 for n in sizes)):
        return False
    need = [stages_needed(k, n) for n in sizes]
    return all(s is not None and s <= MAX_STAGES for s in need)


STAGE_COUNTS = {(1000, 460800): 3, (4096, 460800): 7, (4097, 460800): 8, (5000, 460800): 10, (8000, 16384): 43, (8192, 8193): None}
STAGE_PLAN_CALLS = [(4096, 460800), (4097, 460800), (5000, 460800), (8000, 16384), (8192, 8193), (8192, 8192)]


def hierarchical_select(logits, k):
    """What the stages compute: keep the best min(len, k) of every chunk of 8192, repeat until one chunk is left, cut to k."""
    logits = np.asarray(logits, dtype=np.float32)
    idx = np.arange(logits.shape[0], dtype=np.int64)
    stages = 0
    while True:
        parts = [idx[lo:lo + CHUNK] for lo in range(0, idx.shape[0], CHUNK)]
        # inside a chunk positions ascend with the original index only in stage 0; later the key carries the original index, so ties
        # are decided by it: sort (value, index) lexicographically = stable order over the index-sorted chunk
        kept = []
        for p in parts:
            q = np.sort(p)
            kept.append(q[stable_desc_order(logits[q])][:k])
        stages += 1
        if len(parts) == 1:
            return kept[0], stages
        idx = np.concatenate(kept)


# ---------------------------------------------------------------------------------------------------------------------------------
# logit families: (n, k) -> (logits float32 (n,), winners int64 (min(k, n),), scores float32) ; winners are closed forms of the index

def _by_class(cls, n_classes):
    """Indices grouped by an integer class, classes ascending, indices ascending inside a class."""
    return np.concatenate([np.nonzero(cls == c)[0] for c in range(n_classes)]).astype(np.int64)


def _finish(logits, winners, k):
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    winners = np.asarray(winners, dtype=np.int64)[:min(k, logits.shape[0])]
    return logits, winners, logits[winners]


def all_equal(n, k):
    return _finish(np.full(n, 0.25, dtype=np.float32), np.arange(n), k)


def ascending(n, k):
    return _finish(np.arange(n, dtype=np.float32), n - 1 - np.arange(n), k)


def descending(n, k):
    return _finish(F32(n - 1) - np.arange(n, dtype=np.float32), np.arange(n), k)


def last_chunk(n, k):
    """Zeros, and 1, 2, 3 ... upwards through the final chunk: the final chunk wins from its end, then the zeros from index 0."""
    lo = ((n - 1) // CHUNK) * CHUNK
    m = n - lo
    logits = np.zeros(n, dtype=np.float32)
    logits[lo:] = 1 + np.arange(m, dtype=np.float32)
    return _finish(logits, np.concatenate([n - 1 - np.arange(m), np.arange(lo)]), k)


ONE_PER_CHUNK_POS = (0, 1023, 1024, 8191)


def one_per_chunk(n, k):
    """Chunk c holds 100 + c at in-chunk position 0, 1023, 1024, 8191 in rotation (where the level is long enough), 0.5 elsewhere:
    the large values win from the last chunk backwards, then the rest in index order."""
    chunks = (n + CHUNK - 1) // CHUNK
    big = [c * CHUNK + ONE_PER_CHUNK_POS[c % 4] for c in range(chunks)]
    big = [i for i in big if i < n]
    logits = np.full(n, 0.5, dtype=np.float32)
    is_big = np.zeros(n, dtype=bool)
    for i in big:
        logits[i] = 100 + i // CHUNK
        is_big[i] = True
    return _finish(logits, np.concatenate([np.array(big[::-1], dtype=np.int64), np.nonzero(~is_big)[0]]), k)


def mod7(n, k):
    i = np.arange(n)
    return _finish(-(i % 7).astype(np.float32), _by_class(i % 7, 7), k)


def signed_zero(n, k):
    """-0.0 on even and +0.0 on odd indices tie in index order behind 3.0 at index 0, 2.0 at n // 3 and 1.0 at n - 1 (later
    assignments win where the positions coincide)."""
    i = np.arange(n)
    logits = np.where(i % 2 == 0, F32(-0.0), F32(0.0)).astype(np.float32)
    cls = np.full(n, 3)
    for pos, value, c in ((n - 1, 1.0, 2), (n // 3, 2.0, 1), (0, 3.0, 0)):
        logits[pos] = value
        cls[pos] = c
    return _finish(logits, _by_class(cls, 4), k)


# (value, class in the expected order); the background -(i % 3) fills classes 4 (-0.0), 6 (-1) and 7 (-2)
_SPECIALS = [(NANS[0], 0), (F32(np.inf), 1), (NANS[2], 0), (F32(-FLT_MAX), 8), (DENORM_MIN, 3), (NANS[1], 0), (F32(-np.inf), 9),
             (NANS[3], 0), (F32(FLT_MAX), 2), (-DENORM_MIN, 5)]


def special_positions(n):
    """Ten positions over the first, the middle and the last chunk of the level (fewer when n < 30)."""
    if n < 30:
        return list(range(min(n, len(_SPECIALS))))
    return [0, 1, 5, n // 2 - 1, n // 2, n // 2 + 1, n - 4, n - 3, n - 2, n - 1]


def specials(n, k):
    """NaNs of four bit patterns, +-inf, +-FLT_MAX and the smallest denormals of both signs among -(i % 3): NaNs first in index order,
    then +inf, FLT_MAX, the denormal, the zeros, the negative denormal, -1, -2, -FLT_MAX, -inf, each class in index order."""
    i = np.arange(n)
    logits = -(i % 3).astype(np.float32)
    cls = np.array([4, 6, 7])[i % 3]
    for pos, (value, c) in zip(special_positions(n), _SPECIALS):
        logits[pos] = value
        cls[pos] = c
    return _finish(logits, _by_class(cls, 10), k)


FAMILIES = collections.OrderedDict((f.__name__, f) for f in (all_equal, ascending, descending, last_chunk, one_per_chunk, mod7,
                                                             signed_zero, specials))
NO_TIES_NO_NAN = ('ascending', 'descending')

TOPK_SIZES = (1, 2, 999, 1000, 1001, 8191, 8192, 8193, 16384, 16385, 73729, 460800)


def _topk_pairs():
    """k in 1, 2, 1000, 2000, 4096 and n - 1, n, n + 1 (up to 8192) per size; for n <= 8192 every k > n + 1 repeats k = n + 1 and is
    dropped; pairs the stage plan refuses are the business of STAGE_PLAN_CALLS."""
    pairs = []
    for n in TOPK_SIZES:
        ks = {1, 2, 1000, 2000, 4096} | {v for v in (n - 1, n, n + 1) if 1 <= v <= MAX_K}
        if n <= CHUNK:
            ks = {v for v in ks if v <= n + 1}
        pairs += [(n, v) for v in sorted(ks) if served(v, n)]
    pairs += [(n, v) for v, n in STAGE_COUNTS if served(v, n) and (n, v) not in pairs]
    return pairs


TOPK_PAIRS = _topk_pairs()

# several levels in one call: (sizes, k, family of every level)
_NAMES = list(FAMILIES)
MULTI_LEVEL = collections.OrderedDict([
    ('stages_mixed', ((73729, 1, 8192, 8193, 16385), 1000, ('mod7', 'specials', 'last_chunk', 'specials', 'one_per_chunk'))),
    ('eight_levels', ((8193, 1000, 16385, 2, 999, 8192, 73729, 1001), 1000, tuple(_NAMES))),
    ('eight_levels_k4096', ((16384, 8191, 1, 16385, 8193, 2, 8192, 1001), 4096, tuple(_NAMES[::-1]))),
    ('product_k1000', ((460800, 115200, 28800, 7200, 1800), 1000, ('specials', 'mod7', 'signed_zero', 'last_chunk', 'one_per_chunk'))),
    ('product_k2000', ((460800, 115200, 28800, 7200, 1800), 2000, ('one_per_chunk', 'specials', 'mod7', 'all_equal', 'specials'))),
])


def trick_anchors(n):
    i = np.arange(n, dtype=np.float32)
    return np.stack([i, np.zeros_like(i), i + 1, np.ones_like(i)], axis=1)


def clip_f32(b, w, h):
    """Boxes.clip as the kernel does it: o < 0 -> 0, o > limit -> limit, NaN and -0.0 stay."""
    b = np.array(b, dtype=np.float32)
    w, h = F32(w), F32(h)
    with np.errstate(invalid='ignore'):
        for cols, lim in ((slice(0, 4, 2), w), (slice(1, 4, 2), h)):
            v = b[:, cols]
            v = np.where(v < 0, F32(0), np.where(v > lim, lim, v))
            b[:, cols] = v
    return b


def decode(deltas, anchors, img_h, img_w, dtype=np.float32):
    """The op sequence of det_boxmath.h (weights 1) in numpy at the given precision."""
    T = dtype
    d, a = np.asarray(deltas).astype(T), np.asarray(anchors).astype(T)
    half, clamp = T(0.5), T(SCALE_CLAMP)
    with np.errstate(all='ignore'):
        widths, heights = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        ctr_x, ctr_y = a[:, 0] + half * widths, a[:, 1] + half * heights
        dx, dy = d[:, 0] * T(1), d[:, 1] * T(1)
        dw, dh = d[:, 2] * T(1), d[:, 3] * T(1)
        dw = np.where(dw > clamp, clamp, dw)
        dh = np.where(dh > clamp, clamp, dh)
        pcx, pcy = dx * widths + ctr_x, dy * heights + ctr_y
        pw, ph = np.exp(dw) * widths, np.exp(dh) * heights
        out = np.stack([pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph], axis=1)
        assert out.dtype == T
        lim = np.array([img_w, img_h, img_w, img_h], dtype=T)
        out = np.where(out < 0, T(0), np.where(out > lim, lim, out))
    return out


def decode_f32(deltas, anchors, img_h, img_w):
    return decode(deltas, anchors, img_h, img_w, np.float32)


def box_ok(b):
    with np.errstate(invalid='ignore'):
        return ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)


VALIDITY_IMG = (1280.0, 1920.0)          # (h, w)
# kind -> (anchor, delta); three shifted copies of every kind are used
_INF = float('inf')
_VALIDITY_KINDS = collections.OrderedDict([
    ('positive', ((10, 10, 50, 40), (0.1, -0.2, 0.3, 0.1))),
    ('positive_scale_clamp', ((100, 100, 110, 108), (0.0, 0.0, 9.0, 9.0))),
    ('positive_partly_clipped', ((-10, -10, 50, 40), (0, 0, 0, 0))),
    ('zero_width', ((10, 10, 10, 40), (0, 0, 0, 0))),
    ('zero_height', ((10, 40, 50, 40), (0, 0, 0, 0))),
    ('negative_width', ((50, 10, 10, 40), (0, 0, 0, 0))),
    ('negative_height', ((10, 40, 50, 10), (0, 0, 0, 0))),
    ('empty_at_left', ((-50, 10, -10, 40), (0, 0, 0, 0))),
    ('empty_at_right', ((1930, 10, 1970, 40), (0, 0, 0, 0))),
    ('empty_at_top', ((10, -50, 50, -10), (0, 0, 0, 0))),
    ('empty_at_bottom', ((10, 1290, 50, 1330), (0, 0, 0, 0))),
    ('nan_delta_centre', ((10, 10, 50, 40), (float('nan'), 0, 0, 0))),
    ('nan_delta_size', ((10, 10, 50, 40), (0, 0, 0, float('nan')))),
    ('nan_inf_minus_inf', ((-3e38, 10, 3e38, 40), (1, 0, 0, 0))),
])
VALIDITY_EXPECT = {'positive': True, 'positive_scale_clamp': True, 'positive_partly_clipped': True}        # every other kind: invalid


def validity_family():
    """(kinds, deltas, anchors, boxes float32-decoded, valid) - three copies of every kind, the second and third shifted by (+300, +200)
    and (+700, +500) where the kind is not tied to a border or to infinity."""
    kinds, deltas, anchors = [], [], []
    for rep, (sx, sy) in enumerate(((0, 0), (300, 200), (700, 500))):
        for kind, (a, d) in _VALIDITY_KINDS.items():
            if kind.startswith('empty_at') or kind == 'nan_inf_minus_inf':
                sx_, sy_ = 0, 0
                if kind in ('empty_at_left', 'empty_at_right'):
                    sy_ = sy
                elif kind in ('empty_at_top', 'empty_at_bottom'):
                    sx_ = sx
            else:
                sx_, sy_ = sx, sy
            kinds.append(kind)
            anchors.append((a[0] + sx_, a[1] + sy_, a[2] + sx_, a[3] + sy_))
            deltas.append(d)
    deltas, anchors = np.array(deltas, dtype=np.float32), np.array(anchors, dtype=np.float32)
    boxes = decode_f32(deltas, anchors, *VALIDITY_IMG)
    return kinds, deltas, anchors, boxes, box_ok(boxes)


# ---------------------------------------------------------------------------------------------------------------------------------
# RPN candidate sort (n <= 8192)

SORT_SIZES = (1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192)
VALID_PATTERNS = ('all', 'none', 'mod3', 'absent')


def sort_payload(n, pattern):
    """Row r: box (r, r + .25, r + .5, r + .75), group r % 5 - 1, (valid, valid2) of the pattern; valid2 None = not passed."""
    r = np.arange(n)
    boxes = (r[:, None] + np.array([0, 0.25, 0.5, 0.75])).astype(np.float32)
    group = (r % 5 - 1).astype(np.int32)
    ones, zeros = np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    valid, valid2 = {'all': (ones, ones), 'none': (zeros, ones), 'mod3': ((r % 3 != 0).astype(np.uint8), (r % 3 != 1).astype(np.uint8)),
                     'absent': ((r % 3 != 0).astype(np.uint8), None)}[pattern]
    return boxes, group, valid, valid2


def sort_case(family, n, pattern):
    """-> dict of inputs and expected outputs of wd_sort_candidates_f32."""
    scores, order, sorted_scores = FAMILIES[family](n, n)
    boxes, group, valid, valid2 = sort_payload(n, pattern)
    both = valid if valid2 is None else valid & valid2
    return dict(scores=scores, boxes=boxes, group=group, valid=valid, valid2=valid2, order=order, out_scores=sorted_scores,
                out_boxes=boxes[order], out_group=group[order], out_valid=both[order])


# ---------------------------------------------------------------------------------------------------------------------------------
# box-head candidates (rows x nc)

THIRD = F32(1.0 / 3)
THRESH = F32(0.05)
BOX_SHAPES = ((1, 1), (1, 4), (37, 4), (1000, 4), (2048, 4), (2730, 3), (8192, 1))
BOX_REFUSED_SHAPES = ((2731, 3), (2049, 4), (8193, 1))
BOX_IMG = (1280.0, 1920.0)               # (h, w)
KNIFE_MIN = 1000                         # pairs per class and per kind of "another evaluation decides differently", over the whole set
KNIFE_SEEDS = (0, 1, 2)                  # the set: one (2048, 4) block of knife_edge_scores per seed


def mean3_f32(s0, s1, s2):
    """((s0 + s1) + s2) * float32(1 / 3), every operation rounded to float32: the kernel's and torch's sequence."""
    s0, s1, s2 = (np.asarray(v, dtype=np.float32) for v in (s0, s1, s2))
    with np.errstate(invalid='ignore', over='ignore'):
        out = ((s0 + s1) + s2) * THIRD
    assert out.dtype == np.float32
    return out


def sums_landing_on(target):
    """Every float32 sum S with S * float32(1/3) == target (the product is monotone in S: a window around target * 3 is exhaustive)."""
    s = F32(F32(target) * F32(3))
    lo = s
    for _ in range(16):
        lo = np.nextafter(lo, F32(0))
    out, v = [], lo
    for _ in range(33):
        if F32(v * THIRD) == F32(target):
            out.append(v)
        v = np.nextafter(v, F32(1))
    return out


def knife_edge_scores(rows=2048, nc=4, seed=0):
    """Three (rows, nc + 1) matrices whose class columns all lie on the threshold's edge: the float32 sum (s0 + s1) + s2 of pair
    (row, cls) is, in rotation, one of the float32 sums that the multiplication by float32(1/3) takes to nextafter(thresh, 0), to thresh
    itself or to nextafter(thresh, 1) (sums_landing_on: for thresh = float32(0.05) one sum each for the two neighbours and none for the
    threshold, which no float32 sum reaches).  s0 and s1 are random, s2 is chosen among the float32 values that make the sum come out
    as planned.  Background columns hold 0.5.
    -> (s0, s1, s2, info): info['mean'] the float32 means (rows, nc), info['real'] = mean > thresh, info['cls'] 0 below / 1 at / 2 above, info['flip_f64' | 'flip_div' | 'flip_assoc'] the pairs that the float64 mean, the division by 3.0f and the other
    association s0 + (s1 + s2) decide differently."""
    rng = np.random.default_rng(seed)
    m = rows * nc
    below, above = np.nextafter(THRESH, F32(0)), np.nextafter(THRESH, F32(1))
    window = np.array(sums_landing_on(below) + sums_landing_on(THRESH) + sums_landing_on(above), dtype=np.float32)
    s0 = np.empty(m, dtype=np.float32)
    s1 = np.empty(m, dtype=np.float32)
    s2 = np.empty(m, dtype=np.float32)
    todo = np.arange(m)
    want = window[np.arange(m) % len(window)]
    while todo.size:
        a = rng.uniform(0.01, 0.07, todo.size).astype(np.float32)
        b = rng.uniform(0.01, 0.07, todo.size).astype(np.float32)
        p = a + b
        c = (want[todo] - p).astype(np.float32)
        c = (c.view(np.int32) + rng.integers(-3, 4, todo.size).astype(np.int32)).view(np.float32)       # a few ulps either way
        ok = ((p + c) == want[todo]) & (c > 0)
        s0[todo[ok]], s1[todo[ok]], s2[todo[ok]] = a[ok], b[ok], c[ok]
        todo = todo[~ok]
    mean = mean3_f32(s0, s1, s2)
    cls = np.where(mean == below, 0, np.where(mean == THRESH, 1, np.where(mean == above, 2, 3)))
    real = mean > THRESH
    d0, d1, d2 = s0.astype(np.float64), s1.astype(np.float64), s2.astype(np.float64)
    info = dict(mean=mean.reshape(rows, nc), real=real.reshape(rows, nc), cls=cls.reshape(rows, nc),
                flip_f64=(((d0 + d1 + d2) / 3.0 > np.float64(THRESH)) != real).reshape(rows, nc),
                flip_div=((((s0 + s1) + s2) / F32(3) > THRESH) != real).reshape(rows, nc),
                flip_assoc=(((s0 + (s1 + s2)) * THIRD > THRESH) != real).reshape(rows, nc))

    def full(v):
        out = np.full((rows, nc + 1), 0.5, dtype=np.float32)
        out[:, :nc] = v.reshape(rows, nc)
        return out
    return full(s0), full(s1), full(s2), info


def poison_kinds(nc):
    """(target, column, value): target 0 = the box, 1..3 = a stage's score matrix (columns 0..nc, the last is the background)."""
    bad = (float('nan'), float('inf'), float('-inf'))
    return [(0, c, v) for c in range(4) for v in bad] + [(t, c, v) for t in (1, 2, 3) for c in range(nc + 1) for v in bad]


BOX_FAMILIES = ('equal', 'poison_odd', 'poison_even', 'clip', 'at_thresh', 'nv_none', 'nv_0', 'nv_1', 'nv_rows_m1', 'nv_rows',
                'nv_rows_p7', 'nv_m3')


def _plain_boxes(rows):
    r = np.arange(rows, dtype=np.float32)
    return np.stack([r % 1500 + 1, r % 900 + 2, r % 1500 + 41, r % 900 + 32], axis=1).astype(np.float32)


def box_case(family, rows, nc):
    """-> dict: inputs of wd_box_candidates_f32 (boxes, s0, s1, s2, n_valid, thresh) and the expected outputs.  Every real pair of a
    case has the same score, so the expected order is the flat index among the real pairs, then the flat index among the rest."""
    boxes = _plain_boxes(rows)
    s = [np.full((rows, nc + 1), 0.3, dtype=np.float32) for _ in range(3)]
    thresh, n_valid = THRESH, None
    real = np.ones((rows, nc), dtype=bool)
    flat = np.arange(rows * nc).reshape(rows, nc)
    if family.startswith('poison'):
        kinds = poison_kinds(nc)
        first = 1 if family == 'poison_odd' else 0
        for j, row in enumerate(range(first, rows, 2)):
            target, col, value = kinds[j % len(kinds)]
            (boxes if target == 0 else s[target - 1])[row, col] = value
            real[row] = False
    elif family == 'clip':
        h, w = BOX_IMG
        pats = np.array([(-3e38, -3e38, 3e38, 3e38), (-0.0, -0.0, 5.0, 6.0), (-7.5, -0.25, 30.0, 20.0), (1900.0, 1270.0, 1921.0, 1281.0),
                         (3e38, 3e38, 3e38, 3e38), (-3e38, 5.0, -1.0, 9.0), (w, h, w + 1, h + 1), (5.0, 6.0, -0.0, -0.0)], dtype=np.float32)
        boxes = pats[np.arange(rows) % len(pats)].copy()
    elif family == 'at_thresh':
        thresh = F32(0.25)                                      # (0.25 + 0.25 + 0.25) * float32(1/3) is exactly 0.25: not real
        at = flat % 2 == 0
        for m in s:
            m[:, :nc] = np.where(at, F32(0.25), F32(0.5))
        real = ~at
    elif family.startswith('nv_'):
        n_valid = {'nv_none': None, 'nv_0': 0, 'nv_1': 1, 'nv_rows_m1': rows - 1, 'nv_rows': rows, 'nv_rows_p7': rows + 7,
                   'nv_m3': -3}[family]
        if n_valid is not None:
            real = np.broadcast_to((np.arange(rows) < n_valid)[:, None], (rows, nc)).copy()
    else:
        assert family == 'equal', family
    mean = mean3_f32(s[0][:, :nc], s[1][:, :nc], s[2][:, :nc])
    flat_real = real.reshape(-1)
    order = np.concatenate([np.nonzero(flat_real)[0], np.nonzero(~flat_real)[0]]).astype(np.int64)
    n_real = int(flat_real.sum())
    scores = np.full(rows * nc, -1.0, dtype=np.float32)
    scores[:n_real] = mean.reshape(-1)[order[:n_real]]
    return dict(boxes=boxes, s0=s[0], s1=s[1], s2=s[2], n_valid=n_valid, thresh=thresh, real=real, n_real=n_real, order=order,
                out_scores=scores, out_boxes=clip_f32(boxes, BOX_IMG[1], BOX_IMG[0])[order // nc],
                out_group=np.where(np.arange(rows * nc) < n_real, order % nc, -1).astype(np.int32),
                out_valid=(np.arange(rows * nc) < n_real).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------------------
# wire rows

WIRE_N = (0, 1, 127, 128, 129, 300)
WIRE_SIZES = ((1920, 1280, 1920, 1280), (2880, 1920, 1920, 1280), (1920, 886, 1920, 886), (1237, 713, 1920, 1280))   # in_w, in_h, out_w, out_h


def wire_counts(n):
    """None (every slot real), 0, 1, n - 1, n, n + 5, without repeats or negatives."""
    out = [None]
    for c in (0, 1, n - 1, n, n + 5):
        if c >= 0 and c not in out:
            out.append(c)
    return out


def wire_scores(n):
    ties = [F32(m) / F32(64) for m in range(1, 64, 2)]                  # score * 1e5 ends in .5 exactly
    fixed = [F32(0), F32(1), F32(0.999995), f32_bits(0x00000003)[0]]
    near = []
    for j in (0, 1, 12345, 50000, 99999):
        v = F32(j / 1e5 + 0.5e-5)
        near += [np.nextafter(v, F32(0)), v, np.nextafter(v, F32(1))]
    pool = np.array(ties + fixed + near, dtype=np.float32)
    return pool[np.arange(n) % len(pool)]


def wire_boxes(n, in_w, in_h, out_w, out_h):
    """Row r takes pattern r % 8 at a position that moves with r: input coordinates that scale to whole output pixels, their float32
    neighbours, negative, zero-size, x2 < x1 and far outside (up to 1e7)."""
    out = np.zeros((n, 4), dtype=np.float32)
    fx, fy = in_w / out_w, in_h / out_h
    for r in range(n):
        px, py = (37 * r) % out_w, (23 * r) % out_h                    # whole output pixels
        pw, ph = 1 + (11 * r) % 200, 1 + (7 * r) % 150
        x1, y1, x2, y2 = F32(px * fx), F32(py * fy), F32((px + pw) * fx), F32((py + ph) * fy)
        pat = r % 8
        if pat == 1:
            x1, y1, x2, y2 = (np.nextafter(v, F32(-1e9)) for v in (x1, y1, x2, y2))
        elif pat == 2:
            x1, y1, x2, y2 = (np.nextafter(v, F32(1e9)) for v in (x1, y1, x2, y2))
        elif pat == 3:
            x1, y1 = F32(-x2 - F32(0.75)), F32(-y2 - F32(0.5))           # truncation goes toward zero, not down
            x2, y2 = F32(x1 + F32(0.5)), F32(y1 + F32(0.25))
        elif pat == 4:
            x2, y2 = x1, y1
        elif pat == 5:
            x1, x2 = x2, x1
        elif pat == 6:
            x1, y1, x2, y2 = F32(-1e7 + r), F32(-3e6 - r), F32(1e7 - 3 * r), F32(9999999.0)
        elif pat == 7:
            x1, y1, x2, y2 = F32(x1 + F32(0.5)), F32(y1 + F32(0.25)), F32(x2 + F32(0.125)), F32(y2 + F32(0.0625))
        out[r] = (x1, y1, x2, y2)
    return out


def wire_classes(n):
    return (np.arange(n) * 3 % 4).astype(np.int64)


def wire_ref(boxes, scores, classes, count, in_w, in_h, out_w, out_h, hflip):
    """Detectron2Det.predict + COCODetection.load_prediction restated: float32 box steps, then Python floats, int() truncation,
    Python's round(score, 5).  -> (xywh list of int 4-lists, scores list of float, category list of int; 0 for slots >= count)."""
    b = np.array(boxes, dtype=np.float32).reshape(-1, 4)
    if hflip:
        w = F32(in_w)
        b = np.stack([w - b[:, 2], b[:, 1], w - b[:, 0], b[:, 3]], axis=1)
    iw, ih = F32(1.0 / in_w), F32(1.0 / in_h)
    x1, y1, x2, y2 = b[:, 0] * iw, b[:, 1] * ih, b[:, 2] * iw, b[:, 3] * ih
    cx, cy = (x1 + x2) * F32(0.5), (y1 + y2) * F32(0.5)
    w, h = x2 - x1, y2 - y1
    assert cx.dtype == np.float32 and w.dtype == np.float32
    xywh, out_scores, cat = [], [], []
    for i in range(b.shape[0]):
        bx, by, bw, bh = float(cx[i]) * out_w, float(cy[i]) * out_h, float(w[i]) * out_w, float(h[i]) * out_h
        bx -= bw / 2
        by -= bh / 2
        xywh.append([int(bx), int(by), int(bw), int(bh)])
        out_scores.append(round(float(scores[i]), 5))
        cat.append(int(classes[i]) + 1 if count is None or i < count else 0)
    return xywh, out_scores, cat


def wire_cases():
    """Every (n, count, sizes, hflip) of the set -> (id, dict of inputs)."""
    for n in WIRE_N:
        for count in wire_counts(n):
            for sizes in WIRE_SIZES:
                for hflip in (False, True):
                    yield ('n%d-count%s-%dx%d_to_%dx%d-%s' % ((n, count) + sizes + ('hflip' if hflip else 'plain',)),
                           dict(n=n, count=count, sizes=sizes, hflip=hflip, boxes=wire_boxes(n, *sizes), scores=wire_scores(n),
                                classes=wire_classes(n)))
