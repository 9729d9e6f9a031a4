"""Track smoothing restated in plain Python: per-trajectory dicts keyed by slot, Python floats, one operation
per statement.  Built differently from csrc/track_smooth.hip on purpose - the kernel walks two linked chains of rows with two
pointers; here a trajectory is a dict and "is there a row at slot f - d" is a lookup.

Definition.  A tracking result = the rows utils.track_packed returns.  A trajectory = the rows of one stream with the same
object_id; its class is the category of its first observation (lowest slot).  A job = window[class - 1] in 0..32 and a weight table
weights[class - 1][0 ..] per class, finite, >= 0, the first > 0, longer than the window.  For the row of trajectory T at slot f, W the
window and k the weights of T's class, and each of x, y, w, h on its own:
    acc = k[0] * v(f);  den = k[0];  pairs = 0
    for d = 1 .. W ascending, only when T has a row at slot f - d AND a row at slot f + d:
        pair = v(f - d) + v(f + d);  term = k[d] * pair;  acc = acc + term
        two = k[d] + k[d];           den = den + two;     pairs += 1
    out = acc / den if pairs > 0, else v(f) itself
All reads are of input values.  Score, category, identity, row count and row order are untouched.

`variant` swaps one step for a plausible other implementation, for the tests that prove a case can tell them apart: 'fused' (acc =
fma(k[d], pair, acc), rounded once), 'descending' (d = W .. 1) and 'split' (k[d] * v(f - d) + k[d] * v(f + d))."""
import math
from fractions import Fraction

MAX_WINDOW = 32
VARIANTS = ('definition', 'fused', 'descending', 'split')


def stream_of_slot(stream_frame_offsets, slot):
    for s in range(len(stream_frame_offsets) - 1):
        if stream_frame_offsets[s] <= slot < stream_frame_offsets[s + 1]:
            return s
    raise ValueError('slot %d is in no stream' % slot)


def divide(a, b):
    """C division of doubles, b > 0 or +inf or NaN"""
    if a != a or b != b:
        return float('nan')
    if math.isinf(a) and math.isinf(b):
        return float('nan')
    return a / b


def smooth_value(values, f, window, k, variant='definition'):
    """values: {slot: v} of one trajectory and column.  Returns (out, pairs)."""
    v = values[f]
    acc = k[0] * v
    den = k[0]
    pairs = 0
    distances = range(1, window + 1) if variant != 'descending' else range(window, 0, -1)
    for d in distances:
        if f - d not in values or f + d not in values:
            continue
        a, b = values[f - d], values[f + d]
        if variant == 'split':
            left = k[d] * a
            right = k[d] * b
            term = left + right
            acc = acc + term
        elif variant == 'fused':
            pair = a + b
            acc = float(Fraction(k[d]) * Fraction(pair) + Fraction(acc))        # exact, rounded once
        else:
            pair = a + b
            term = k[d] * pair
            acc = acc + term
        two = k[d] + k[d]
        den = den + two
        pairs += 1
    if pairs == 0:
        return v, 0
    return divide(acc, den), pairs


def trajectories(stream_frame_offsets, out):
    """[(class, {slot: caller's row})] of every (stream, object_id)"""
    offsets = [int(v) for v in stream_frame_offsets]
    found = {}
    for i in range(len(out['frame'])):
        slot = int(out['frame'][i])
        key = (stream_of_slot(offsets, slot), int(out['object_id'][i]))
        rows = found.setdefault(key, {})
        if slot in rows:
            raise ValueError('object_id %d occurs twice in slot %d' % (key[1], slot))
        rows[slot] = i
    result = []
    for rows in found.values():
        first = min(rows)                                  # the category of the first observation
        result.append((int(out['category'][rows[first]]), rows))
    return result


def check_job(job, n_classes):
    assert len(job['window']) == n_classes and len(job['weights']) == n_classes
    for W, k in zip(job['window'], job['weights']):
        assert 0 <= W <= MAX_WINDOW and len(k) > W
        assert all(math.isfinite(x) and x >= 0.0 for x in k) and k[0] > 0.0


def smooth(stream_frame_offsets, out, job, variant='definition'):
    """out: dict of sequences frame, category, bbox, object_id; job: {'window': [per class], 'weights': [[k0, k1, ..] per class]}.
    Returns {'bbox': [[x, y, w, h]], 'pairs': [n]} per row in the caller's order."""
    assert variant in VARIANTS
    check_job(job, len(job['window']))
    bbox = [[float(v) for v in row] for row in out['bbox']]
    pairs = [0] * len(bbox)
    source = [list(row) for row in bbox]
    for cls, rows in trajectories(stream_frame_offsets, out):
        W = int(job['window'][cls - 1])
        k = [float(x) for x in job['weights'][cls - 1]]
        if W == 0:
            continue
        for col in range(4):
            values = dict((slot, source[i][col]) for slot, i in rows.items())
            for slot, i in rows.items():
                bbox[i][col], pairs[i] = smooth_value(values, slot, W, k, variant)
    return {'bbox': bbox, 'pairs': pairs}


def gaussian(sigma, n):
    return [math.exp(-(d * d) / (2.0 * sigma * sigma)) for d in range(n)]


def box(n):
    return [1.0] * n
