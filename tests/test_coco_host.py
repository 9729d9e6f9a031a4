"""Host side of the COCO metric (detnet/evaluate.py, detnet/eval.py; no GPU): the packers against the restatement's own, the three
result forms, the refusals made before any launch, the summary numbers, and both command lines end to end with
tests/coco_ap_ref.py injected in place of the HIP call."""
import json

import numpy as np
import pytest

import coco_ap_ref as R
import coco_cases as CC
from waymo_2d_tracking_amd import _lib
from waymo_2d_tracking_amd.detnet import eval as coco_cli
from waymo_2d_tracking_amd.detnet import evaluate as E


def test_constants_are_the_restatements():
    assert np.array_equal(E.COCO_THR, R.THR) and np.array_equal(E.COCO_REC, R.REC) and np.array_equal(E.COCO_AREAS, R.AREAS)
    assert np.array_equal(E.COCO_MAX_DETS, R.MAX_DETS) and E.COCO_MAX_DETS.dtype == np.int32 and E.COCO_STATS == R.STAT_NAMES


def test_ground_truth_and_wire_rows_pack_like_the_restatement():
    annotations, sets, _ = CC.random_case(2, 2)
    gt, ref = E.pack_coco_ground_truth(annotations), R.ground_truth(annotations)
    assert gt['image_ids'] == ref['image_ids'] and gt['cat_ids'] == ref['cat_ids'] == [1, 2, 3, 4] and gt['names'] == ref['names']
    for k in ('x', 'y', 'w', 'h', 'area', 'cat', 'crowd', 'image_gt_offsets'):
        assert np.array_equal(gt[k], ref[k]) and gt[k].dtype == ref[k].dtype, k
    assert gt['crowd'].sum() > 0 and (gt['area'] != gt['w'] * gt['h']).any() and E.pack_coco_ground_truth(gt) is gt
    p = E.pack_coco_detections(gt, sets)
    for k, rows in enumerate(sets):
        r = R.result(ref, rows)
        lo, hi = p['set_row_offsets'][k], p['set_row_offsets'][k + 1]
        for name in ('score', 'x', 'y', 'w', 'h', 'cat', 'source_row'):
            assert np.array_equal(p[name][lo:hi], r[name]), name
        assert np.array_equal(p['image_det_offsets'][k], r['image_det_offsets']) and np.array_equal(p['has_rows'][k], r['has_rows'])
        assert len(r['score']) < len(rows)                                   # rows of the undefined category 5 took no part


def test_image_ids_sort_as_given_and_float_coordinates_are_kept():
    annotations = {'images': [{'id': 10, 'width': 100, 'height': 50}, {'id': 9, 'width': 100, 'height': 50}], 'categories': [{'id': 7, 'name': 'x'}, {'id': 3, 'name': 'y'}],
                   'annotations': [{'image_id': 10, 'category_id': 7, 'bbox': [0.1, 0.2, 0.3, 16777217.0]}, {'image_id': 9, 'category_id': 3, 'bbox': [1, 2, 3, 4], 'ignore': 1},
                                   {'image_id': 10, 'category_id': 7, 'bbox': [0.1, 0.2, 0.3, 16777217.0]}]}
    gt = E.pack_coco_ground_truth(annotations)
    assert gt['image_ids'] == [9, 10] and gt['cat_ids'] == [3, 7] and gt['cat'].tolist() == [0, 1, 1]          # 9 before 10: not as strings
    assert gt['h'].tolist() == [4.0, 16777217.0, 16777217.0] and gt['x'].tolist() == [1.0, 0.1, 0.1]             # no float32 rounding, duplicates stay
    assert gt['crowd'].tolist() == [0, 0, 0] and gt['image_gt_offsets'].tolist() == [0, 1, 3]


def test_the_three_result_forms_give_the_same_columns(tmp_path):
    from waymo_2d_tracking_amd.detnet.trainer import Predictions
    annotations = CC.ann(['a', 'b'], [('a', 1, [0, 0, 50, 50]), ('b', 2, [10, 10, 20, 20])])
    gt = E.pack_coco_ground_truth(annotations)
    f = lambda rows: np.asarray(rows, np.float64).reshape(-1, 5)
    per_image = {'b': [f([[.875, .5, .5, .25, .25]]), f([[.75, .25, .5, .125, .0625], [.625, .75, .25, .5, .5]])], 'a': [f([]), f([[.5, .5, .25, .25, .125]])]}
    wire = []
    for k in ('a', 'b'):                                                        # the dict form goes class by class inside an image
        for ci, rows in enumerate(per_image[k]):
            for conf, cx, cy, w, h in rows.tolist():
                wire.append(CC.det(k, ci + 1, [(cx - w / 2) * 1920, (cy - h / 2) * 1280, w * 1920, h * 1280], conf))
    path = tmp_path / 'dets.json'
    json.dump(wire, open(path, 'w'))
    store = Predictions(['vehicle', 'pedestrian'])
    for k, v in per_image.items():
        store[k] = [a.astype(np.float32) for a in v]                            # these values are exact in float32
    forms = [E.pack_coco_detections(gt, [s]) for s in (wire, str(path), per_image, store)]
    assert forms[0]['score'].tolist() == [.5, .875, .75, .625] and forms[0]['cat'].tolist() == [1, 0, 1, 1] and forms[0]['x'][1] == (.5 - .25 / 2) * 1920
    for other in forms[1:]:
        for name in E.COCO_DET_COLUMNS + ('cat', 'set_row_offsets', 'image_det_offsets', 'has_rows'):
            assert np.array_equal(forms[0][name], other[name]), name


def test_refusals_name_the_image_or_the_row():
    annotations = CC.hand_cases()['k_all_images'][0]
    gt = E.pack_coco_ground_truth(annotations)
    with pytest.raises(_lib.WaymoTrackError, match=r'WT_ERR_INVALID.*row 1 is on image zz'):
        E.pack_coco_detections(gt, [[CC.det('a', 1, [0, 0, 1, 1], .5), CC.det('zz', 1, [0, 0, 1, 1], .5)]])
    with pytest.raises(_lib.WaymoTrackError, match=r'WT_ERR_INVALID.*result 1, row 2'):
        E.pack_coco_detections(gt, [[], [CC.det('a', 1, [0, 0, 1, 1], .5)] * 2 + [CC.det('b', 1, [0, 0, 1, float('inf')], .5)]])
    with pytest.raises(_lib.WaymoTrackError, match=r'WT_ERR_INVALID.*result 0, row 0'):
        E.pack_coco_detections(gt, [[CC.det('a', 1, [0, 0, 1, 1], float('nan'))]])
    with pytest.raises(_lib.WaymoTrackError, match=r'annotation 0 is on image q'):
        E.pack_coco_ground_truth(CC.ann(['a'], [('q', 1, [0, 0, 1, 1])]))
    with pytest.raises(_lib.WaymoTrackError, match=r'annotation 0 has category_id 9'):
        E.pack_coco_ground_truth(CC.ann(['a'], [('a', 9, [0, 0, 1, 1])]))
    with pytest.raises(ValueError, match='at least one'):
        E.pack_coco_detections(gt, [])
    with pytest.raises(TypeError):
        E.pack_coco_detections(gt, [42])
    with pytest.raises(ValueError, match='waymo'):                              # 'coco' is no threshold preset: it is another algorithm
        E.thresholds({'classnames': ['background', 'vehicle'], 'n_classes': 1}, 'coco')


def test_results_from_the_injected_restatement_and_the_summary():
    annotations, sets, _ = CC.hand_cases()['h_category_without_ground_truth']
    r = E.evaluate_coco_sets(annotations, sets, per_row=True, call=R.call_from_packed)[0]
    ref = R.case_reference('h_category_without_ground_truth', lambda: CC.hand_cases()['h_category_without_ground_truth'])[5]
    assert np.array_equal(r.precision, ref['precision'][0]) and np.array_equal(r.recall, ref['recall'][0]) and np.array_equal(r.npig, ref['npig'][0])
    assert np.array_equal(r.stats, R.summarize(ref['precision'][0], ref['recall'][0])) and len(r.stats) == 12
    assert np.array_equal(r.rank, ref['rank'][0]) and np.array_equal(r.match_gt, ref['match_gt'][0]) and np.array_equal(r.ignore, ref['ignore'][0])
    cats = r.per_category()
    assert [(c[0], c[1], c[2]) for c in cats] == [(1, 'vehicle', 1), (2, 'pedestrian', 1)] and (cats[1][3] == -1).all()
    table = r.table()
    assert len(table) == 2 and table[1].endswith('vehicle') and ' 1  ' in table[1]          # pedestrian has no value >= 0: no row
    only2 = E.evaluate_coco_sets(annotations, sets, cat_ids=[2], call=R.call_from_packed)[0]
    assert only2.stats.tolist() == [-1.0] * 12 and np.array_equal(only2.precision, r.precision)
    dt = [E.evaluate_coco_sets(*CC.hand_cases()[n][:2], dt_images=CC.hand_cases()[n][2], call=R.call_from_packed)[0] for n in ('k_all_images', 'k_dt_images')]
    assert dt[0].npig[0, 0] == 2 and dt[1].npig[0, 0] == 1 and dt[0].stats[8] == 0.5 and dt[1].stats[8] == 1.0


def test_eval_command_line_end_to_end(tmp_path):
    annotations, sets, _ = CC.random_case(1, 1)
    gt_path, dt_path = tmp_path / 'gt.json', tmp_path / 'dt.json'
    json.dump(annotations, open(gt_path, 'w'))
    json.dump(sets[0], open(dt_path, 'w'))
    lines = []
    r = coco_cli.main(['--gt', str(gt_path), '--dt', str(dt_path), '--each-category'], coco_call=R.call_from_packed, print_fn=lines.append)
    ref = R.case_reference('random1', lambda: CC.random_case(1, 1))[5]
    stats = R.summarize(ref['precision'][0], ref['recall'][0])
    assert np.array_equal(r.stats, stats) and 0 < stats[0] < 1
    assert lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %0.3f' % stats[0]
    assert lines[1] == ' Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = %0.3f' % stats[1]
    assert lines[6] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = %0.3f' % stats[6]
    assert lines[11] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = %0.3f' % stats[11]
    assert len(lines) == 12 + 1 + 4 and lines[12].split() == list(E.COCO_STATS) + ['T', 'name']
    maps = [float(l.split()[0]) for l in lines[13:]]
    assert maps == sorted(maps, reverse=True) and sorted(l.split()[-1] for l in lines[13:]) == ['cyclist', 'pedestrian', 'sign', 'vehicle']
    counts = np.bincount(R.ground_truth(annotations)['cat'])
    assert sorted(int(l.split()[-2]) for l in lines[13:]) == sorted(counts.tolist())
    # --catId selects the categories of the summary, --dt-images the images
    lines2 = []
    half = [r for r in sets[0] if r['image_id'] < 'img020']
    json.dump(half, open(dt_path, 'w'))
    r2 = coco_cli.main(['--gt', str(gt_path), '--dt', str(dt_path), '--catId', '2,3', '--dt-images'], coco_call=R.call_from_packed, print_fn=lines2.append)
    gt = R.ground_truth(annotations)
    ref2 = R.evaluate(gt, [R.result(gt, half)], dt_images=True)
    assert np.array_equal(r2.stats, R.summarize(ref2['precision'][0][:, :, 1:3], ref2['recall'][0][:, 1:3])) and len(lines2) == 12
    assert np.array_equal(r2.npig, ref2['npig'][0]) and (ref2['npig'] < ref['npig']).any()
    with pytest.raises(SystemExit, match='--catId 9'):
        coco_cli.main(['--gt', str(gt_path), '--dt', str(dt_path), '--catId', '9'], coco_call=R.call_from_packed)
    args = coco_cli.build_parser().parse_args(['--gt', 'G.json'])
    assert args.dt == 'submission.json' and args.catId == [] and not args.dt_images and not args.each_category


def test_evaluate_command_line_with_coco(tmp_path, capsys):
    annotations, sets, _ = CC.hand_cases()['j_three_step_curve']
    gt_path, dt_path, out_path = tmp_path / 'gt.json', tmp_path / 'dt.json', tmp_path / 'out.json'
    json.dump(annotations, open(gt_path, 'w'))
    json.dump(sets[0], open(dt_path, 'w'))
    assert E.main(['--annotations', str(gt_path), '--coco', str(dt_path), '--json', str(out_path)], coco_call=R.call_from_packed) == 0
    printed = capsys.readouterr().out.splitlines()
    assert printed[0] == str(dt_path) and len(printed) == 13 and printed[1].startswith(' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.7')
    saved = json.load(open(out_path))[str(dt_path)]
    assert list(saved) == list(E.COCO_STATS) and saved['mAP'] == pytest.approx((34 + 33 * 2 / 3 + 34 * .6) / 101, abs=1e-12)
    args = E.build_parser().parse_args(['--annotations', 'GT.json', '--coco', '--sweep', 'A.json', 'B.json'])
    assert args.coco and args.sweep == ['A.json', 'B.json'] and args.metric == 'waymo'
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(['--annotations', 'GT.json', '--metric', 'coco', 'A.json'])      # --metric keeps its two choices


def test_without_a_gpu_the_call_fails_loudly():
    import torch
    annotations, sets, _ = CC.hand_cases()['k_all_images']
    if torch.cuda.is_available():
        assert E.evaluate_coco_sets(annotations, sets)[0].stats[8] == 0.5
    else:
        with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_NO_DEVICE'):
            E.evaluate_coco_sets(annotations, sets)


def test_the_modules_do_not_import_the_restatement():
    for mod in (E, coco_cli):
        src = open(mod.__file__).read()
        assert 'coco_ap_ref' not in src and 'oracle' not in src and 'pycocotools' not in src
