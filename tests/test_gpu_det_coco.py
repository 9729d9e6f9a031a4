"""HIP COCO metric (csrc/det_coco_eval.hip through detnet/evaluate.py) against the plain restatement tests/coco_ap_ref.py.

Equality rule: both tables, npig and every per-row output are EQUAL, the tables bit for bit.  Every table entry is one chain of
individually rounded float64 operations on the same integers on both sides (ctp / npig, ctp / ((cfp + ctp) + 2^-52), comparisons and
maxima, which are exact), the unit is compiled without FMA contraction, and neither side sums floating-point values: no tolerance."""
import ctypes as C
import json
import shlex

import numpy as np
import pytest

import coco_ap_ref as R
import coco_cases as CC

pytestmark = pytest.mark.gpu

TABLES = ('precision', 'recall', 'npig')
ROWS = ('rank', 'match_gt', 'ignore')


def evaluate():
    from waymo_2d_tracking_amd.detnet import evaluate as E
    return E


def expected(name, build):
    """The restatement on its own packing of the case (shared with tests/test_coco_ap_ref.py), rows of the K sets concatenated."""
    _, _, _, gt, packed, out = R.case_reference(name, build)
    A, T = len(R.AREAS), len(R.THR)
    exp = {k: out[k] for k in TABLES}
    exp['rank'] = np.concatenate(out['rank'])
    exp['match_gt'] = np.concatenate(out['match_gt']).reshape(-1, A, T)
    exp['ignore'] = np.concatenate(out['ignore']).reshape(-1, A, T)
    return exp


def assert_equal(got, exp, names=TABLES + ROWS):
    for k in names:
        assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, (k, got[k].shape, exp[k].shape, got[k].dtype, exp[k].dtype)
        same = got[k] == exp[k]
        assert same.all(), (k, int((~same).sum()), np.argwhere(~same)[:5].tolist(), got[k][~same][:5], exp[k][~same][:5])


def run_case(name, build):
    E = evaluate()
    annotations, sets, dt_images = build()
    gt = E.pack_coco_ground_truth(annotations)
    p = E.pack_coco_detections(gt, sets)
    got = E._coco_call_host(gt, p, p['has_rows'] if dt_images else None, True)
    assert_equal(got, expected(name, build))
    return gt, p, got


@pytest.mark.parametrize('name', sorted(CC.hand_cases()))
def test_hand_worked_cases(name):
    run_case(name, lambda: CC.hand_cases()[name])


def test_problem_sizes_around_the_tile_the_cap_and_the_lds_limit():
    gt, p, got = run_case('shapes', CC.shapes_case)
    assert (got['rank'] == -1).sum() == 65 + 1 + 65 and got['rank'].max() == 99
    assert np.diff(gt['image_gt_offsets']).max() == 300                        # above 256 rows: the taken words live in the workspace


@pytest.mark.parametrize('k_sets', [1, 2, 3])
def test_random_sets(k_sets):
    gt, p, got = run_case('random%d' % k_sets, lambda: CC.random_case(k_sets, k_sets))
    assert (got['precision'] > 0).any() and (got['ignore'] == 1).any() and (got['rank'] == -1).any()
    # the tables alone (per-row outputs NULL) are the same
    E = evaluate()
    assert_equal(E._coco_call_host(gt, p, None, False), got, TABLES)


def test_three_hundred_categories():
    gt, p, got = run_case('many_categories', CC.many_categories_case)
    assert gt['n_cats'] == 300 and got['npig'][0, [0, 149, 299], 0].tolist() == [1, 2, 1] and got['npig'].sum() == 2 * (1 + 1 + 2 + 2 + 1 + 1)
    assert (got['precision'][:, :, :, 298] == -1).all() and (got['precision'][:, 0, :, 299, 0, 2] > 0.99).all()


def test_two_sets_without_rows():
    """n_det = 0 with K = 2: only the offsets and curve kernels run."""
    gt, p, got = run_case('two_empty_sets', lambda: (CC.hand_cases()['j_three_step_curve'][0], [[], []], False))
    assert p['set_row_offsets'].tolist() == [0, 0, 0] and got['npig'][:, 0, 0].tolist() == [3, 3]
    assert (got['precision'][:, :, :, 0, 0] == 0).all() and (got['recall'][:, :, 0, 0] == 0).all()


def test_every_row_takes_no_part():
    """Category indices outside 0..n_cats - 1, which only the device form lets through: all rows sort into the last segment, the
    one no curve reads, and the tables are those of a result without rows."""
    E = evaluate()
    annotations, sets, _ = CC.random_case(2, 2)
    gt = E.pack_coco_ground_truth(annotations)
    p = E.pack_coco_detections(gt, sets)
    p['cat'][:] = np.where(np.arange(len(p['cat'])) % 2, gt['n_cats'], -1).astype(np.int32)
    dev = E.DeviceCocoEvaluation(gt, p)
    dev.launch()
    res = dev.results()
    exp = R.call_from_packed(gt, p)
    assert (exp['rank'] == -1).all() and (exp['npig'] > 0).any() and exp['precision'].max() == 0
    got = dict(precision=np.stack([r.precision for r in res]), recall=np.stack([r.recall for r in res]), npig=np.stack([r.npig for r in res]),
               rank=np.concatenate([r.rank for r in res]), match_gt=np.concatenate([r.match_gt for r in res]), ignore=np.concatenate([r.ignore for r in res]))
    assert_equal(got, exp)


def half_case():
    annotations, sets, _ = CC.random_case(2, 2)
    return annotations, [[r for r in sets[0] if r['image_id'] < 'img020'], [r for r in sets[1] if r['image_id'] >= 'img030']], True


def test_image_mask():
    gt, p, got = run_case('random2_dt_images', half_case)
    assert p['has_rows'][0, :20].sum() > 10 and p['has_rows'][0, 20:].sum() == 0 and p['has_rows'][1, 30:].sum() > 5 and p['has_rows'][1, :30].sum() == 0
    full = expected('random2', lambda: CC.random_case(2, 2))
    assert (got['npig'] < full['npig']).any() and got['npig'][0].sum() > got['npig'][1].sum() > 0


def test_k_results_in_one_call_equal_k_calls_of_one():
    E = evaluate()
    annotations, sets, _ = CC.random_case(3, 3)
    gt = E.pack_coco_ground_truth(annotations)
    together = E.evaluate_coco_sets(gt, sets, per_row=True)
    exp = R.case_reference('random3', lambda: CC.random_case(3, 3))[5]
    for k in range(3):
        alone = E.evaluate_coco_sets(gt, [sets[k]], per_row=True)[0]
        for name in TABLES + ROWS + ('source_row', 'stats'):
            assert np.array_equal(getattr(together[k], name), getattr(alone, name)), (k, name)
        assert np.array_equal(alone.stats, R.summarize(exp['precision'][k], exp['recall'][k]))
    assert len(set(float(r.stats[0]) for r in together)) == 3


def test_device_form_equals_host_form():
    import torch
    E = evaluate()
    annotations, sets, _ = CC.random_case(2, 2)
    exp = expected('random2', lambda: CC.random_case(2, 2))
    for per_row in (True, False):
        dev = E.DeviceCocoEvaluation(annotations, sets, per_row=per_row)
        torch.cuda.synchronize()                                 # the buffers were filled on the default stream
        with torch.cuda.stream(torch.cuda.Stream()):
            dev.launch()
            dev.launch()                                         # a second launch on the same buffers gives the same result
            res = dev.results()
        for k, r in enumerate(res):
            assert np.array_equal(r.precision, exp['precision'][k]) and np.array_equal(r.recall, exp['recall'][k]) and np.array_equal(r.npig, exp['npig'][k])
        if per_row:
            assert np.array_equal(np.concatenate([r.rank for r in res]), exp['rank'])
            assert np.array_equal(np.concatenate([r.match_gt for r in res]), exp['match_gt'])
            assert np.array_equal(np.concatenate([r.ignore for r in res]), exp['ignore'])


def host_call(lib, gt, p, out, **over):
    from waymo_2d_tracking_amd import _lib
    E = evaluate()
    a = dict(thr=np.ascontiguousarray(E.COCO_THR), rec=np.ascontiguousarray(E.COCO_REC), areas=np.ascontiguousarray(E.COCO_AREAS),
             md=np.ascontiguousarray(E.COCO_MAX_DETS), n_thr=10, n_rec=101, n_area=4, n_md=3, k_sets=len(p['set_row_offsets']) - 1, n_cats=gt['n_cats'])
    cols = dict(p)
    for k, v in over.items():
        if k in a:
            a[k] = v
        else:
            cols[k] = v
    ptr = lambda v: _lib.ptr(v) if v is not None else None
    return lib.wt_det_coco_host(
        C.c_int64(gt['x'].size), ptr(gt['x']), ptr(gt['y']), ptr(gt['w']), ptr(gt['h']), ptr(gt['area']), ptr(gt['cat']), ptr(gt['crowd']),
        C.c_int64(len(gt['image_ids'])), ptr(gt['image_gt_offsets']), C.c_int32(a['k_sets']), ptr(cols['set_row_offsets']), ptr(cols['image_det_offsets']),
        ptr(cols['score']), ptr(cols['x']), ptr(cols['y']), ptr(cols['w']), ptr(cols['h']), ptr(cols['cat']), None,
        C.c_int32(a['n_cats']), C.c_int32(a['n_thr']), ptr(a['thr']), C.c_int32(a['n_rec']), ptr(a['rec']), C.c_int32(a['n_area']), ptr(a['areas']),
        C.c_int32(a['n_md']), ptr(a['md']), ptr(out.get('precision')), ptr(out.get('recall')), ptr(out.get('npig')), ptr(out.get('rank')),
        ptr(out.get('match_gt')), ptr(out.get('ignore')))


def test_every_refusal_leaves_the_outputs_untouched():
    import torch
    from waymo_2d_tracking_amd import _lib
    E = evaluate()
    lib = _lib.lib()
    annotations, sets, _ = CC.hand_cases()['h_category_without_ground_truth']
    gt = E.pack_coco_ground_truth(annotations)
    p = E.pack_coco_detections(gt, sets)
    n = len(p['score'])

    def fresh():
        return dict(precision=np.full((1, 10, 101, 2, 4, 3), 7.0), recall=np.full((1, 10, 2, 4, 3), 7.0), npig=np.full((1, 2, 4), 7, np.int64),
                    rank=np.full(n, 7, np.int32), match_gt=np.full((n, 4, 10), 7, np.int64), ignore=np.full((n, 4, 10), 7, np.uint8))

    def refused(rc, out, code, text):
        assert rc == code, (rc, lib.wt_last_error())
        assert text in lib.wt_last_error().decode(), lib.wt_last_error()
        for k, v in out.items():
            assert (v == 7).all(), k

    INVALID, CAPACITY = 1, 4
    assert _lib._STATUS[INVALID] == 'WT_ERR_INVALID' and _lib._STATUS[CAPACITY] == 'WT_ERR_CAPACITY'
    out = fresh()
    assert host_call(lib, gt, p, out) == 0 and not any((v == 7).all() for v in out.values())           # the call itself works
    out = fresh()
    refused(host_call(lib, gt, p, dict(out, precision=None)), out, INVALID, 'bad argument')              # null pointer
    refused(host_call(lib, gt, p, dict(out, ignore=None)), out, INVALID, 'come together')
    refused(host_call(lib, gt, p, out, thr=None), out, INVALID, 'bad argument')
    refused(host_call(lib, gt, p, out, n_thr=0), out, INVALID, 'n_thr')                                   # bad shapes
    refused(host_call(lib, gt, p, out, n_thr=17), out, INVALID, 'n_thr')
    refused(host_call(lib, gt, p, out, n_rec=129), out, INVALID, 'n_rec')
    refused(host_call(lib, gt, p, out, n_cats=0), out, INVALID, 'bad argument')
    refused(host_call(lib, gt, p, out, n_cats=1), out, INVALID, 'category index 1 outside 0..0')
    refused(host_call(lib, gt, p, out, md=np.asarray([1, 10, 200], np.int32)), out, CAPACITY, 'max_dets 200 above 128')
    refused(host_call(lib, gt, p, out, md=np.asarray([10, 1, 100], np.int32)), out, INVALID, 'ascend')
    refused(host_call(lib, gt, p, out, rec=np.ascontiguousarray(E.COCO_REC[::-1])), out, INVALID, 'recall thresholds must ascend')
    bad = p['w'].copy()
    bad[2] = np.nan
    refused(host_call(lib, gt, p, out, w=bad), out, INVALID, 'result set 0, row 2')                      # non-finite row
    bad = p['score'].copy()
    bad[1] = np.inf
    refused(host_call(lib, gt, p, out, score=bad), out, INVALID, 'result set 0, row 1')
    refused(host_call(lib, gt, p, out, image_det_offsets=np.asarray([[0, n + 1]], np.int64)), out, INVALID, 'do not cover')
    with pytest.raises(_lib.WaymoTrackError, match='image zz, which the ground truth does not list'):   # unlisted image: refused by the packer
        E.evaluate_coco_sets(gt, [[CC.det('zz', 1, [0, 0, 1, 1], .5)]])
    # sizer: 0 for a bad shape; short workspace: refused before any launch
    size = lambda *a: lib.wt_det_coco_workspace(C.c_int32(a[0]), C.c_int64(a[1]), C.c_int32(a[2]), C.c_int32(a[3]), C.c_int32(a[4]), C.c_int32(a[5]), C.c_int32(a[6]),
                                                C.c_int64(a[7]), C.c_int64(a[8]))
    assert size(1, 1, 2, 10, 101, 4, 3, 2, n) > 0
    assert size(0, 1, 2, 10, 101, 4, 3, 2, n) == 0 and size(1, 1, 2, 10, 101, 5, 3, 2, n) == 0 and size(1, 1, 2, 10, 101, 4, 3, -1, n) == 0
    assert size(1, 1, 2, 16, 101, 4, 3, 2, n) > 0 and size(1, 1, 2, 10, 101, 4, 5, 2, n) == 0 and size(1 << 20, 1 << 20, 2, 10, 101, 4, 3, 2, n) == 0
    dev = E.DeviceCocoEvaluation(gt, p)
    for t in dev.out.values():
        t.fill_(7)
    dev.ws_bytes -= 1
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY.*workspace too small'):
        dev.launch()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in dev.out.values())
    dev.ws_bytes += 1
    dev.launch()
    assert np.array_equal(dev.results()[0].precision, out_ok(E, gt, p))


def out_ok(E, gt, p):
    return E._coco_call_host(gt, p, None, False)['precision'][0]


def test_non_finite_rows_stay_in_bounds_in_the_device_form():
    """The device form does not check the numbers: NaN / inf rows must not fault or hang; what they score is not defined."""
    E = evaluate()
    annotations, sets, _ = CC.hand_cases()['c_crowd_absorbs']
    gt = E.pack_coco_ground_truth(annotations)
    p = E.pack_coco_detections(gt, sets)
    p['score'][0], p['w'][1], p['x'][2] = np.nan, np.inf, -np.inf
    dev = E.DeviceCocoEvaluation(gt, p)
    dev.launch()
    r = dev.results()[0]
    assert r.rank.min() >= 0 and r.rank.max() == 4 and sorted(r.rank.tolist()) == list(range(5)) and r.match_gt.max() <= 1 and r.match_gt.min() >= -1


def test_eval_command_line_on_the_gpu(tmp_path):
    from waymo_2d_tracking_amd.detnet import eval as coco_cli
    annotations, sets, _ = CC.random_case(1, 1)
    json.dump(annotations, open(tmp_path / 'gt.json', 'w'))
    json.dump(sets[0], open(tmp_path / 'dt.json', 'w'))
    lines = []
    r = coco_cli.main(['--gt', str(tmp_path / 'gt.json'), '--dt', str(tmp_path / 'dt.json'), '--each-category'], print_fn=lines.append)
    exp = R.case_reference('random1', lambda: CC.random_case(1, 1))[5]
    assert np.array_equal(r.stats, R.summarize(exp['precision'][0], exp['recall'][0])) and len(lines) == 17
    assert lines[0].endswith('= %0.3f' % r.stats[0])


def test_sweep_ranks_by_coco_map(tmp_path):
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.detnet import ensemble
    E = evaluate()
    subs = syn.ensemble_inputs_json(3, n_images=6, k_inputs=2, n_objects=40)
    ids = sorted(set(r['image_id'] for r in subs[0]))
    boxes = [(r['image_id'], r['category_id'], r['bbox']) for i, r in enumerate(subs[0]) if i % 5]      # every fifth object is unlabelled
    annotations = CC.ann(ids, boxes, CC.CATS4)
    paths = []
    for k, rows in enumerate(subs):
        paths.append(str(tmp_path / ('in%d.json' % k)))
        json.dump(rows, open(paths[-1], 'w'))
    grid = {'method': ['soft_nms', 'nms'], 'iou_thresh': [0.5, 0.7], 'soft_nms_cut': [0.9], 'min_score': [0.0]}
    res = E.sweep(paths, annotations, grid, metric='coco')
    assert len(res.settings) == 4 and sorted(res.ranked) == [0, 1, 2, 3] and all(isinstance(r, E.CocoResult) for r in res.results)
    assert res.mean_ap == [float(r.stats[0]) for r in res.results] and res.mean_ap[res.ranked[0]] == max(res.mean_ap) > 0.2
    assert [res.mean_ap[i] for i in res.ranked] == sorted(res.mean_ap, reverse=True)
    out = tmp_path / 'winner.json'
    ensemble.main(paths + ['-o', str(out)] + shlex.split(res.flag_line()))
    scored = E.evaluate_coco_sets(annotations, [str(out)])[0]
    assert np.array_equal(scored.stats, res.results[res.ranked[0]].stats)
    gt = R.ground_truth(annotations)
    ref = R.evaluate(gt, [R.result(gt, json.load(open(out)))])
    assert np.array_equal(scored.precision, ref['precision'][0]) and np.array_equal(scored.recall, ref['recall'][0])
