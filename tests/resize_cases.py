"""Shapes and contents for the PIL-exact bilinear resize (csrc/resize_host.h, csrc/det_resize.hip), shared by the CPU and the GPU
tests, together with a Python restatement of the coefficient tables and the checks that put every shape into its class.

A shape is ((in_h, in_w), (out_h, out_w)).  The class says which path of the code the shape is there for; class_facts(shape)
computes the facts that test_resize_cases.py holds against CLASS_CHECKS, so that a shape cannot drift out of its class unnoticed.
"""
import math

import numpy as np

MAX_SIZE = 16384
PRECISION_BITS = 22

# class -> shapes
CLASSES = {
    'smallest': [((1, 1), (1, 1)), ((1, 1), (5, 7)), ((7, 5), (1, 1))],
    'long_kernel': [((3, 300), (2, 2)), ((300, 3), (2, 2))],
    'large_upscale': [((2, 2), (3, 300))],
    'copy': [((64, 64), (64, 64))],
    'horizontal_only': [((40, 63), (40, 31)), ((40, 64), (40, 32)), ((40, 65), (40, 33)), ((40, 257), (40, 129))],
    'vertical_only': [((63, 40), (31, 40)), ((65, 40), (97, 40))],
    'ratio_1_5': [((48, 72), (32, 48)), ((48, 72), (72, 108))],
    'non_integer': [((61, 91), (30, 45)), ((96, 130), (37, 50))],
    'ksize_35': [((33, 1025), (33, 64)), ((1025, 33), (64, 33))],
    'off_by_one': [((20, 30), (19, 29)), ((20, 30), (21, 31))],
    'row_sum': [((128, 192), (80, 120))],
}
SHAPES = [s for shapes in CLASSES.values() for s in shapes]
CONTENTS = ('random', 'zeros', 'full', 'checker')


def shape_id(shape):
    (h, w), (oh, ow) = shape
    return '%dx%d-%dx%d' % (h, w, oh, ow)


def make_image(shape, content, seed=0):
    """(in_h, in_w, 3) uint8."""
    h, w = shape[0]
    if content == 'random':
        return np.random.default_rng(seed + 7919 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == 'zeros':
        return np.zeros((h, w, 3), np.uint8)
    if content == 'full':
        return np.full((h, w, 3), 255, np.uint8)
    if content == 'checker':
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    raise ValueError(content)


def pil_resize(img, out_h, out_w):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((out_w, out_h), Image.BILINEAR))


def ksize(in_size, out_size):
    scale = in_size / out_size
    support = 1.0 * max(scale, 1.0)
    return int(math.ceil(support)) * 2 + 1


def tables(in_size, out_size):
    """The tables of one axis in Python floats (IEEE double, one rounding per operation): bounds (out_size, 2) int32 and coeffs
    (out_size, ksize) int32."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ks), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
            ww = ww + w[-1]
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            coeffs[xx, x] = int(v * 4194304.0 + 0.5)
        bounds[xx] = (xmin, xmax)
    return bounds, coeffs


def resize_ref(img, out_h, out_w):
    """The two passes in numpy from tables(): horizontal first, rounded to uint8, then vertical."""
    h, w = img.shape[:2]
    cur = img
    for axis, (n_in, n_out) in ((1, (w, out_w)), (0, (h, out_h))):
        if n_in == n_out:
            continue
        bounds, coeffs = tables(n_in, n_out)
        src = np.moveaxis(cur, axis, 0).astype(np.int64)
        out = np.zeros((n_out,) + src.shape[1:], np.int64)
        for xx in range(n_out):
            first, count = bounds[xx]
            acc = np.tensordot(coeffs[xx, :count].astype(np.int64), src[first:first + count], axes=(0, 0))
            assert np.all(acc < 2 ** 31)
            out[xx] = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
        cur = np.moveaxis(out.astype(np.uint8), 0, axis)
    return np.ascontiguousarray(cur)


def class_facts(shape):
    """What the class checks look at: per axis ('x' = width, 'y' = height) skipped / ksize / whether a window was clamped at 0 and at
    in_size / the set of row sums minus 2^22."""
    (h, w), (oh, ow) = shape
    facts = {}
    for name, n_in, n_out in (('x', w, ow), ('y', h, oh)):
        if n_in == n_out:
            facts[name] = dict(skipped=True, ksize=None, clamped_low=False, clamped_high=False, sum_offsets=set())
            continue
        scale = n_in / n_out
        support = max(scale, 1.0)
        bounds, coeffs = tables(n_in, n_out)
        centers = (np.arange(n_out) + 0.5) * scale
        low = any(int(c - support + 0.5) < 0 for c in centers)
        high = any(int(c + support + 0.5) > n_in for c in centers)
        facts[name] = dict(skipped=False, ksize=ksize(n_in, n_out), clamped_low=low, clamped_high=high,
                           sum_offsets=set((coeffs.sum(1).astype(np.int64) - (1 << PRECISION_BITS)).tolist()))
    return facts


# class -> predicate over class_facts(shape)
CLASS_CHECKS = {
    'smallest': lambda f, s: min(s[0] + s[1]) == 1,
    'long_kernel': lambda f, s: sorted((f['x']['ksize'], f['y']['ksize'])) == [5, 301],
    'large_upscale': lambda f, s: f['x']['ksize'] == 3 and s[1][1] >= 100 * s[0][1],
    'copy': lambda f, s: f['x']['skipped'] and f['y']['skipped'],
    'horizontal_only': lambda f, s: f['y']['skipped'] and not f['x']['skipped'],
    'vertical_only': lambda f, s: f['x']['skipped'] and not f['y']['skipped'],
    'ratio_1_5': lambda f, s: {s[0][0] / s[1][0], s[0][1] / s[1][1]} in ({1.5}, {1 / 1.5}),
    'non_integer': lambda f, s: not any(float(a / b).is_integer() or float(2 * a / b).is_integer() for a, b in zip(s[0], s[1])),
    'ksize_35': lambda f, s: 35 in (f['x']['ksize'], f['y']['ksize']),
    'off_by_one': lambda f, s: all(abs(a - b) == 1 for a, b in zip(s[0], s[1])),
    'row_sum': lambda f, s: bool((f['x']['sum_offsets'] | f['y']['sum_offsets']) - {0}),
}
