"""HIP detection metric (csrc/det_eval.hip through detnet/evaluate.py) against the reference-run fixture, detnet/data/metric.py on
tie-free input, and the plain-numpy restatement tests/det_ap_ref.py where confidences tie.

Equality rules: (i) tp_flag, match_gt, order, ctp, cfp, npos, tp, fp, T are EQUAL; (ii) recall / precision rebuilt from ctp / cfp
are equal and ar is bit-equal (one correctly rounded division of the same integers on both sides); (iii) ap is within
(T + 1) * 2^-52 of the reference value: the AP terms are bit-identical by (ii), non-negative, at most T + 1 in number and sum to
<= 1, and any two summation orders of n such terms differ by at most 2 (n - 1) 2^-53 times their sum (numpy sums pairwise, the
kernel by tree; neither order is part of the definition).  Against the G8 fixture, whose values went through JSON: 1e-12."""
import json
import os
import shlex

import numpy as np
import pytest

import det_ap_ref as R

pytestmark = pytest.mark.gpu

LABELS = [1, 2, 3, 4]
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope='module')
def g8(golden_dir):
    return json.load(open(os.path.join(golden_dir, 'metric_g8.json')))


def _preds(g8):
    return {k: [np.asarray(d, np.float32).reshape(-1, 5) for d in v] for k, v in g8['predictions'].items()}


def same(a, b):
    return a == b or (a != a and b != b)


def reference(annotations, detections, metric, min_conf=0.01):
    from waymo_2d_tracking_amd.detnet.data import metric as M
    image_ids, sizes, gt, names = M.load_ground_truth(annotations)
    g, d = R.columns(image_ids, sizes, gt, detections, LABELS)
    return g, d, R.evaluate(g, d, 4, [R.THRESHOLDS[metric](n) for n in names[1:]], min_conf)


def assert_equals_restatement(got, ref, d, n_thr, labels=LABELS):
    """DetResult (per_row=True) against det_ap_ref.evaluate() on the same rows, by the three rules."""
    assert np.array_equal(got.tp_flag, ref['tp_flag'])
    assert np.array_equal(got.match_gt, ref['match_gt'])
    for c in labels:
        assert np.array_equal(got.order[c], ref['order'][c]), c
        for t in range(n_thr):
            for bi, b in enumerate(('', 'S', 'M', 'L')):
                exp = ref['curves'][(c, t, b)]
                print('class %d thr %d bucket %r: T %d tp %d fp %d ap %.17g (ref %.17g, diff %.3g, bound %.3g) ar %r'
                      % (c, t, b, exp['T'], exp['tp'], exp['fp'], got.ap[c - 1, t, bi], exp['ap'], abs(got.ap[c - 1, t, bi] - exp['ap']),
                         (exp['T'] + 1) * 2.0 ** -52, got.ar[c - 1, t, bi]))
                assert got.npos[c - 1, t, bi] == exp['T'] and got.tp[c - 1, t, bi] == exp['tp'] and got.fp[c - 1, t, bi] == exp['fp'], (c, t, b)
                assert same(float(got.ar[c - 1, t, bi]), exp['ar']), (c, t, b)
                assert abs(got.ap[c - 1, t, bi] - exp['ap']) <= (exp['T'] + 1) * 2.0 ** -52, (c, t, b)
            exp = ref['curves'][(c, t, '')]
            ctp, cfp = got.ctp[c][:, t], got.cfp[c][:, t]
            assert np.array_equal(ctp, exp['ctp']) and np.array_equal(cfp, exp['cfp']), (c, t)
            assert np.array_equal(ctp / max(exp['T'], EPS), exp['rec']) and np.array_equal(ctp / np.maximum(ctp + cfp, EPS), exp['prec'])


@pytest.mark.parametrize('metric', ['waymo', 'voc'])
def test_g8_matches_the_numbers_of_the_reference_run(g8, metric):
    from waymo_2d_tracking_amd.detnet import evaluate as E
    r = E.evaluate_detection_sets(g8['annotations'], [_preds(g8)], metric=metric, min_conf=g8['threshold'])[0]
    got = r.summary()
    for cls, exp in g8['expected_' + metric].items():
        for k, v in exp.items():
            if k == 'by_size':
                continue
            print(cls, k, got[cls][k], v)
            if v is None:
                assert got[cls][k] is None or np.isnan(got[cls][k]), (cls, k)
            else:
                assert got[cls][k] == pytest.approx(v, abs=1e-12), (cls, k)
    if metric == 'waymo':
        assert got['vehicle']['T'] == 20 and got['sign']['T'] == 0
        assert any('mean AP' in line for line in r.lines())
    else:
        assert got['score'] == pytest.approx(np.mean([g8['expected_voc'][c]['ap@0.5'] for c in g8['classnames']]), abs=1e-12)


def as_restatement(got, thr_count):
    """DetResult (per_row=True) -> the dict det_ap_ref.evaluate() returns, with what the device has: rec / prec / ctp / cfp for the
    all-sizes bucket (rebuilt from the device's ctp / cfp), ap / ar / T for every bucket."""
    curves = {}
    for c in LABELS:
        for t in range(thr_count):
            for bi, b in enumerate(('', 'S', 'M', 'L')):
                curves[(c, t, b)] = dict(ap=float(got.ap[c - 1, t, bi]), ar=float(got.ar[c - 1, t, bi]), T=int(got.npos[c - 1, t, bi]))
            ctp, cfp = got.ctp[c][:, t], got.cfp[c][:, t]
            curves[(c, t, '')].update(ctp=ctp, cfp=cfp, rec=ctp / max(int(got.npos[c - 1, t, 0]), EPS), prec=ctp / np.maximum(ctp + cfp, EPS))
    return dict(tp_flag=got.tp_flag, match_gt=got.match_gt, order=got.order, curves=curves)


@pytest.fixture(scope='module')
def tie_free():
    from test_det_ap_ref import assert_tie_free
    annotations, detections = R.synthetic(5, n_images=220)
    assert_tie_free(detections)
    return annotations, detections


@pytest.mark.parametrize('metric', ['waymo', 'voc'])
def test_tie_free_synthetic_set_equals_metric_py(tie_free, metric):
    from test_det_ap_ref import compare_with_metric_py
    from waymo_2d_tracking_amd.detnet import evaluate as E
    from waymo_2d_tracking_amd.detnet.data import metric as M
    annotations, detections = tie_free
    gt = E.pack_ground_truth(annotations)
    p = E.pack_detections(gt, [detections])
    got = E.evaluate_detection_sets(gt, p, metric=metric, per_row=True)[0]
    assert np.array_equal(got.source_row, np.arange(len(p['conf'])))      # one dict set: packed rows = rows of det_ap_ref.columns
    compare_with_metric_py(annotations, detections, as_restatement(got, thr_count=E.thresholds(gt, metric).shape[1]), None, p, metric)
    ev = M.evaluate_detections(detections, annotations, metric=metric)
    s = got.summary()
    assert list(s) == list(ev)
    lines = []
    M.evaluate_detections(detections, annotations, metric=metric, print_fn=lines.append)
    assert got.lines() == lines                              # the printed figures (4 decimals) agree


def test_many_ties_equal_the_restatement():
    from waymo_2d_tracking_amd.detnet import evaluate as E
    annotations, detections = R.synthetic(5, n_images=220, decimals=2)
    g, d, ref = reference(annotations, detections, 'voc')
    conf = d['conf'][(d['label'] == 1) & (d['conf'] > 0.01)]
    assert len(np.unique(conf)) < len(conf) / 10             # at most 100 different values
    gt = E.pack_ground_truth(annotations)
    p = E.pack_detections(gt, [detections])
    assert np.array_equal(p['conf'], d['conf']) and np.array_equal(p['category'], d['label'])
    got = E.evaluate_detection_sets(gt, p, metric='voc', per_row=True)[0]
    assert_equals_restatement(got, ref, d, 2)


def test_three_sets_with_their_own_min_conf_in_one_call_equal_three_calls(tie_free):
    from waymo_2d_tracking_amd.detnet import evaluate as E
    annotations, detections = tie_free
    _, other = R.synthetic(6, n_images=220)
    half = {k: v for i, (k, v) in enumerate(detections.items()) if i % 2}
    sets, minc = [detections, other, half], [0.01, 0.3, 0.6]
    gt = E.pack_ground_truth(annotations)
    together = E.evaluate_detection_sets(gt, sets, min_conf=minc, per_row=True)
    assert len(together) == 3
    for k in range(3):
        alone = E.evaluate_detection_sets(gt, [sets[k]], min_conf=minc[k], per_row=True)[0]
        for name in ('ap', 'ar', 'npos', 'tp', 'fp', 'tp_flag', 'match_gt'):
            assert np.array_equal(getattr(together[k], name), getattr(alone, name), equal_nan=name == 'ar'), (k, name)
        for c in LABELS:
            for name in ('order', 'ctp', 'cfp'):
                assert np.array_equal(getattr(together[k], name)[c], getattr(alone, name)[c]), (k, c, name)
    assert together[0].tp[0, 0, 0] > together[2].tp[0, 0, 0] > 0 and (together[1].tp_flag == 2).sum() > (together[0].tp_flag == 2).sum()
    g, d, ref = reference(annotations, other, 'waymo', 0.3)
    assert_equals_restatement(together[1], ref, d, 1)


def test_host_form_equals_device_form(tie_free):
    import torch
    from waymo_2d_tracking_amd.detnet import evaluate as E
    annotations, detections = tie_free
    gt = E.pack_ground_truth(annotations)
    _, other = R.synthetic(6, n_images=220, decimals=2)
    host = E.evaluate_detection_sets(gt, [detections, other], metric='voc', min_conf=[0.01, 0.2], per_row=True)
    dev = E.DeviceDetEvaluation(gt, [detections, other], metric='voc', min_conf=[0.01, 0.2])
    torch.cuda.synchronize()                                 # the buffers were filled on the default stream
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev.launch()
        dev.launch()                                         # a second launch on the same buffers gives the same result
        device = dev.results(per_row=True)
    for h, v in zip(host, device):
        for name in ('ap', 'ar', 'npos', 'tp', 'fp', 'tp_flag', 'match_gt'):
            assert np.array_equal(getattr(h, name), getattr(v, name), equal_nan=name == 'ar'), name
        for c in LABELS:
            for name in ('order', 'ctp', 'cfp'):
                assert np.array_equal(getattr(h, name)[c], getattr(v, name)[c]), (c, name)


def _ann(images, boxes):
    return {'images': [{'id': k, 'width': 1000, 'height': 1000} for k in images], 'categories': R.CATEGORIES,
            'annotations': [{'image_id': k, 'category_id': c, 'bbox': b} for k, c, b in boxes]}


def test_edge_problems():
    from waymo_2d_tracking_amd.detnet import evaluate as E
    f = lambda rows: np.asarray(rows, np.float32).reshape(-1, 5)
    # vehicle: one box, one detection on it; pedestrian: ground truth but no detection; sign: detections but no ground truth;
    # cyclist: neither.  Image 'b' has no detections at all, image 'c' no ground truth.
    annotations = _ann(['a', 'b', 'c'], [('a', 1, [100, 100, 200, 200]), ('a', 2, [500, 500, 50, 100]), ('b', 2, [10, 10, 20, 20])])
    detections = {'a': [f([[0.9, 0.2, 0.2, 0.2, 0.2]]), f([]), f([[0.8, 0.5, 0.5, 0.1, 0.1], [0.4, 0.1, 0.1, 0.01, 0.01]]), f([])],
                  'c': [f([[0.7, 0.5, 0.5, 0.1, 0.1]]), f([]), f([]), f([])]}
    got = E.evaluate_detection_sets(annotations, [detections], per_row=True)[0]
    g, d, ref = reference(annotations, detections, 'waymo')
    assert_equals_restatement(got, ref, d, 1)
    s = got.summary()
    assert s['vehicle']['T'] == 1 and s['vehicle']['ar'] == 1.0 and s['vehicle']['ap'] == 1.0
    assert got.tp[0, 0].tolist() == [1, 0, 0, 1] and got.fp[0, 0].tolist() == [1, 0, 0, 1]          # 200 x 200 px is L; so is the false positive
    assert s['pedestrian']['T'] == 2 and s['pedestrian']['ap'] == 0.0 and np.isnan(s['pedestrian']['ar'])
    assert s['sign']['T'] == 0 and s['sign']['ap'] == 0.0 and s['sign']['ar'] == 0.0 and got.fp[2, 0, 0] == 2
    assert s['cyclist']['T'] == 0 and s['cyclist']['ap'] == 0.0 and np.isnan(s['cyclist']['ar'])
    assert got.match_gt.tolist() == [0, -1, -1, -1] and got.tp_flag[:, 0].tolist() == [1, 0, 0, 0]
    assert got.mean_ap() == 0.5
    # no detection anywhere
    empty = E.evaluate_detection_sets(annotations, [{}], per_row=True)[0]
    assert empty.tp.sum() == 0 and empty.fp.sum() == 0 and np.isnan(empty.ar).all() and (empty.ap == 0).all() and empty.npos[1, 0, 0] == 2


def test_two_sets_without_rows_and_two_whose_rows_all_take_no_part():
    """n_det = 0 with K = 2: only the offsets and curve kernels run.  Every confidence at or under min_conf: all rows sort into the
    last segment, the one no curve reads."""
    from waymo_2d_tracking_amd.detnet import evaluate as E
    f = lambda rows: np.asarray(rows, np.float32).reshape(-1, 5)
    annotations = _ann(['a', 'b'], [('a', 1, [100, 100, 200, 200]), ('a', 2, [500, 500, 50, 100]), ('b', 2, [10, 10, 20, 20])])
    detections = {'a': [f([[0.9, 0.2, 0.2, 0.2, 0.2], [0.9, 0.2, 0.2, 0.2, 0.2]]), f([[0.5, 0.5, 0.5, 0.1, 0.1]]), f([]), f([])],
                  'b': [f([]), f([[0.7, 0.5, 0.5, 0.1, 0.1]]), f([[0.9, 0.5, 0.5, 0.1, 0.1]]), f([])]}
    for sets, min_conf in (([{}, {}], [0.01, 0.01]), ([detections, detections], [0.9, 2.0])):
        got = E.evaluate_detection_sets(annotations, sets, min_conf=min_conf, per_row=True)
        assert len(got) == 2
        for k in range(2):
            g, d, ref = reference(annotations, sets[k], 'waymo', min_conf[k])
            assert_equals_restatement(got[k], ref, d, 1)
            assert got[k].tp.sum() == 0 and got[k].fp.sum() == 0 and (got[k].tp_flag == 2).all() and len(got[k].tp_flag) == len(d['conf'])
            assert np.isnan(got[k].ar).all() and (got[k].ap == 0).all() and got[k].npos[1, 0, 0] == 2
            assert all(len(got[k].order[c]) == 0 for c in LABELS)


def test_shuffled_input_rows_give_the_sorted_result(g8):
    """As test_unsorted_input_gives_the_sorted_result_not_defect_d10 checks for metric.py: the flags follow the confidence order."""
    from waymo_2d_tracking_amd.detnet import evaluate as E
    rng = np.random.default_rng(0)
    preds = _preds(g8)
    shuffled = {k: [d[rng.permutation(len(d))] for d in v] for k, v in preds.items()}
    a, b = E.evaluate_detection_sets(g8['annotations'], [preds, shuffled], min_conf=g8['threshold'])
    assert np.array_equal(a.ap, b.ap) and np.array_equal(a.ar, b.ar, equal_nan=True) and np.array_equal(a.tp, b.tp)
    for cls, exp in g8['expected_waymo'].items():
        assert b.summary()[cls]['ap'] == pytest.approx(exp['ap'], abs=1e-12)


def test_problems_beyond_one_tile():
    """More than 64 and more than 1024 rows on both sides of one problem: several LDS tiles of ground truth, several chunks of
    detections; and a class with more rows than one tile of the curve kernel."""
    from waymo_2d_tracking_amd.detnet import evaluate as E
    annotations, detections = R.synthetic(9, n_images=12, crowd=(3, 1500), clutter=400)
    g, d, ref = reference(annotations, detections, 'voc')
    per_problem = np.bincount(d['image'][(d['label'] == 1) & (d['conf'] > 0.01)])
    assert per_problem.max() > 1024 and ((per_problem > 64) & (per_problem < 1024)).any()
    assert np.bincount(g['image'][g['label'] == 1]).max() == 1500 and len(ref['order'][1]) > 2048
    got = E.evaluate_detection_sets(annotations, [detections], metric='voc', per_row=True)[0]
    assert_equals_restatement(got, ref, d, 2)


def test_sweep_ranks_what_the_ensemble_cli_writes(tmp_path):
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.detnet import ensemble, evaluate as E
    subs = syn.ensemble_inputs_json(3, n_images=6, k_inputs=2, n_objects=40)
    ids = sorted(set(r['image_id'] for r in subs[0]))
    boxes = [(r['image_id'], r['category_id'], r['bbox']) for i, r in enumerate(subs[0]) if i % 5]      # every fifth object is unlabelled
    annotations = {'images': [{'id': k, 'width': 1920, 'height': 1280} for k in ids], 'categories': R.CATEGORIES,
                   'annotations': [{'image_id': k, 'category_id': c, 'bbox': b} for k, c, b in boxes]}
    paths = []
    for k, rows in enumerate(subs):
        paths.append(str(tmp_path / ('in%d.json' % k)))
        json.dump(rows, open(paths[-1], 'w'))
    grid = {'method': ['soft_nms', 'nms'], 'iou_thresh': [0.5, 0.7], 'soft_nms_cut': [0.9], 'min_score': [0.0, 0.3]}
    res = E.sweep(paths, annotations, grid)
    assert len(res.settings) == 8 and sorted(res.ranked) == list(range(8)) and res.settings[0] == {
        'method': 'soft_nms', 'iou_thresh': 0.5, 'soft_nms_cut': 0.9, 'min_score': 0.0}
    aps = [res.mean_ap[i] for i in res.ranked]
    assert all(a >= b for a, b in zip(aps, aps[1:])) and aps[0] > 0.3 and len(set(aps)) > 1
    gt = E.pack_ground_truth(annotations)
    for i in res.ranked:
        s = res.settings[i]
        out = tmp_path / ('out%d.json' % i)
        ensemble.main(paths + ['-o', str(out)] + shlex.split(E.flag_line(s)))
        scored = E.evaluate_detection_sets(gt, [str(out)])[0]
        assert np.array_equal(scored.ap, res.results[i].ap) and np.array_equal(scored.tp, res.results[i].tp), s
        assert scored.mean_ap() == res.mean_ap[i]
    assert res.best == res.settings[res.ranked[0]]
    out = tmp_path / 'winner.json'
    ensemble.main(paths + ['-o', str(out)] + shlex.split(res.flag_line()))
    assert E.evaluate_detection_sets(gt, [str(out)])[0].mean_ap() == max(res.mean_ap)
    # per-input weights reach the merge normalised like the ensemble's own: a weight changes the merged scores and the ranking input
    weighted = E.sweep(paths, gt, {'method': ['weighted_fusion'], 'iou_thresh': [0.5], 'soft_nms_cut': [1.0], 'min_score': [0.0]}, weights=[2, 1])
    same = E.sweep(paths, gt, {'method': ['weighted_fusion'], 'iou_thresh': [0.5], 'soft_nms_cut': [1.0], 'min_score': [0.0]}, weights=[1, 0.5])
    assert np.array_equal(weighted.results[0].ap, same.results[0].ap)
