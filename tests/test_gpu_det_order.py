"""The ordering unit the two detection metrics share (csrc/det_order.hip: the two radix sorts, the segment offsets and the
one-entry cache of the sorts' temporary storage, keyed on (rows, segment bits)): calls of wt_det_eval_host and wt_det_coco_host
take turns, so each finds the cache filled by the other.

Input A (section 16): K = 2 results, 3 classes = 7 segments, 3 segment bits.  Input B (section 28): K = 3 results, 5 categories =
16 segments, 4 bits, another row count.  B2 is B with as many rows as A: the same row count, other bits.  In each, one (image,
class) problem has 70 rows, more than one 64-lane tile, and the scores take few values, so the stable order decides.
Every output of every call equals the first call on that input (bit for bit) and the restatement, by the equality rules of
tests/test_gpu_det_eval.py and tests/test_gpu_det_coco.py."""
import numpy as np
import pytest

import coco_ap_ref as RC
import coco_cases as CC
import det_ap_ref as R
from test_gpu_det_coco import assert_equal
from test_gpu_det_eval import assert_equals_restatement

pytestmark = pytest.mark.gpu

IMAGES = ['a', 'b', 'c']
GRID = [[100.0 * (j % 5), 100.0 * (j // 5), 60.0, 80.0] for j in range(10)]


def input_a():
    """(annotations, [result 0, result 1]) in the forms of tests/test_gpu_det_eval.py: 70 + 9 + 4 and 70 + 6 + 5 rows."""
    annotations = {'images': [{'id': k, 'width': 1000, 'height': 1000} for k in IMAGES], 'categories': R.CATEGORIES[:3],
                   'annotations': [{'image_id': 'a', 'category_id': 1, 'bbox': b} for b in GRID[:6]] +
                                  [{'image_id': k, 'category_id': c, 'bbox': b} for k, c, b in (('a', 2, GRID[7]), ('c', 2, GRID[1]), ('c', 3, GRID[2]))]}
    rng = np.random.default_rng(11)

    def rows(n, boxes):                          # shifted copies of the boxes, confidences of one decimal
        b = np.asarray([boxes[i] for i in rng.integers(0, len(boxes), n)]).reshape(-1, 4) + rng.integers(0, 9, (n, 1))
        conf = rng.integers(2, 10, n) / 10
        return np.stack([conf, (b[:, 0] + b[:, 2] / 2) / 1000, (b[:, 1] + b[:, 3] / 2) / 1000, b[:, 2] / 1000, b[:, 3] / 1000], axis=1).astype(np.float32)

    sets = [{'a': [rows(70, GRID[:6]), rows(9, GRID[6:8]), rows(0, GRID)], 'c': [rows(0, GRID), rows(2, GRID[1:2]), rows(2, GRID[2:4])]},
            {'a': [rows(70, GRID[:8]), rows(0, GRID), rows(6, GRID[:3])], 'b': [rows(3, GRID), rows(2, GRID), rows(0, GRID)]}]
    return annotations, sets


def input_b(n_rows=None):
    """(annotations, [three results]) in the forms of tests/coco_cases.py; n_rows: rows in all (filler on image 'c')."""
    cats = CC.CATS4 + [{'id': 5, 'name': 'other'}]
    boxes = [('a', 2, b, {'iscrowd': 1} if j == 3 else {}) for j, b in enumerate(GRID[:7])] + [('a', 5, GRID[8]), ('b', 1, GRID[0]), ('c', 4, GRID[9])]
    rng = np.random.default_rng(12)
    row = lambda k, c, boxes: CC.det(k, c, [v + float(rng.integers(0, 9)) for v in boxes[int(rng.integers(0, len(boxes)))][:2]] + [60.0, 80.0],
                                     float(rng.integers(2, 10)) / 10)
    sets = [[row('a', 2, GRID[:7]) for _ in range(70)] + [row('a', 5, GRID[8:9]) for _ in range(3)],
            [row('b', 1, GRID[:2]) for _ in range(4)] + [row('a', 2, GRID[:3]) for _ in range(5)],
            [row('c', 4, GRID[8:]) for _ in range(6)]]
    n = sum(len(s) for s in sets)
    sets[2] += [row('c', 3, GRID) for _ in range(7 if n_rows is None else n_rows - n)]
    sets = [[s[i] for i in rng.permutation(len(s))] for s in sets]
    return CC.ann(IMAGES, boxes, cats), sets


@pytest.fixture(scope='module')
def inputs():
    """name -> (call, restatement): call() makes one host call and returns its outputs, the restatement is computed once."""
    from waymo_2d_tracking_amd.detnet import evaluate as E
    from waymo_2d_tracking_amd.detnet.data import metric as M
    annotations, sets = input_a()
    gt = E.pack_ground_truth(annotations)
    p = E.pack_detections(gt, sets)
    image_ids, sizes, boxes, names = M.load_ground_truth(annotations)
    thr = [R.THRESHOLDS['voc'](n) for n in names[1:]]
    refs = []
    for k in range(2):
        g, d = R.columns(image_ids, sizes, boxes, sets[k], [1, 2, 3])
        lo, hi = p['set_row_offsets'][k:k + 2]
        assert np.array_equal(p['conf'][lo:hi], d['conf']) and np.array_equal(p['category'][lo:hi], d['label'])
        assert np.bincount(d['image'][d['label'] == 1])[0] == 70 and len(np.unique(d['conf'])) <= 8
        refs.append((d, R.evaluate(g, d, 3, thr)))
    out = {'A': (lambda: E.evaluate_detection_sets(gt, p, metric='voc', per_row=True), refs)}
    n_a = int(p['set_row_offsets'][-1])
    for name, n_rows in (('B', None), ('B2', n_a)):
        annotations, sets = input_b(n_rows)
        cgt = E.pack_coco_ground_truth(annotations)
        cp = E.pack_coco_detections(cgt, sets)
        n_b = int(cp['set_row_offsets'][-1])
        assert cgt['n_cats'] == 5 and len(cp['set_row_offsets']) == 4 and (n_b == n_a) == (name == 'B2')
        assert ((cp['cat'][:int(cp['image_det_offsets'][0, 1])] == 1).sum()) == 70 and len(np.unique(cp['score'])) <= 8
        out[name] = (lambda cgt=cgt, cp=cp: E._coco_call_host(cgt, cp, None, True), RC.call_from_packed(cgt, cp))
    return out


def flat(results):
    """Every output of the K DetResult of one call, by name."""
    out = {}
    for k, r in enumerate(results):
        out.update({(n, k): getattr(r, n) for n in ('ap', 'ar', 'npos', 'tp', 'fp', 'tp_flag', 'match_gt')})
        out.update({(n, k, c): getattr(r, n)[c] for n in ('order', 'ctp', 'cfp') for c in (1, 2, 3)})
    return out


def test_alternating_calls_of_the_two_metrics_share_the_ordering_unit(inputs):
    first = {}
    for name in ('A', 'B', 'A', 'B', 'B2', 'A', 'B2'):
        call, ref = inputs[name]
        got = call()
        if name == 'A':
            for k, (d, exp) in enumerate(ref):
                assert_equals_restatement(got[k], exp, d, 2, labels=[1, 2, 3])
            got = flat(got)
        else:
            assert_equal(got, ref)
            assert (got['rank'] >= 64).any() and (got['precision'] > 0).any()
        for n, v in first.setdefault(name, got).items():
            assert np.array_equal(v, got[n], equal_nan=n[0] == 'ar'), (name, n)
