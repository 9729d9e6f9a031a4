"""Host side of detnet/evaluate.py (no GPU): ground truth and results in their three forms -> the columns and offsets the kernels
walk, the checks made before the launch, and the two command lines."""
import json
import re

import numpy as np
import pytest

from waymo_2d_tracking_amd import _lib
from waymo_2d_tracking_amd.detnet import evaluate as E

CATS = [{'id': 1, 'name': 'vehicle'}, {'id': 2, 'name': 'pedestrian'}, {'id': 3, 'name': 'sign'}, {'id': 4, 'name': 'cyclist'}]


def annotations():
    images = [{'id': 'b/2/FRONT', 'width': 200, 'height': 100}, {'id': 'a/1/FRONT', 'width': 400, 'height': 200},
              {'id': 'c/3/SIDE_LEFT', 'width': 100, 'height': 100}]
    anns = [{'image_id': 'b/2/FRONT', 'category_id': 2, 'bbox': [20, 10, 40, 30]}, {'image_id': 'a/1/FRONT', 'category_id': 1, 'bbox': [40, 20, 100, 50]},
            {'image_id': 'b/2/FRONT', 'category_id': 1, 'bbox': [100, 50, 50, 25]}, {'image_id': 'a/1/FRONT', 'category_id': 1, 'bbox': [40, 20, 100, 50]}]
    return {'images': images, 'annotations': anns, 'categories': CATS}


def dict_set():
    f = lambda rows: np.asarray(rows, np.float32).reshape(-1, 5)
    return {'c/3/SIDE_LEFT': [f([]), f([]), f([[0.3, 0.5, 0.5, 0.25, 0.5]]), f([])],
            'a/1/FRONT': [f([[0.9, 0.25, 0.25, 0.25, 0.25], [0.005, 0.5, 0.5, 0.125, 0.125]]), f([]), f([]), f([[0.5, 0.5, 0.5, 0.5, 0.5]])],
            'b/2/FRONT': [f([[0.7, 0.625, 0.625, 0.25, 0.25]]), f([[0.6, 0.25, 0.25, 0.25, 0.5], [0.8, 0.75, 0.5, 0.125, 0.25]]), f([]), f([])],
            'unknown/9/FRONT': [f([[0.9, 0.5, 0.5, 0.5, 0.5]]), f([]), f([]), f([])]}


def test_ground_truth_columns_follow_load_ground_truth():
    gt = E.pack_ground_truth(annotations())
    assert gt['image_ids'] == ['a/1/FRONT', 'b/2/FRONT', 'c/3/SIDE_LEFT'] and gt['n_classes'] == 4
    assert gt['image_gt_offsets'].tolist() == [0, 1, 3, 3]                    # the duplicated box of a/1 is gone
    assert gt['image_area'].tolist() == [80000.0, 20000.0, 10000.0]
    assert gt['label'].tolist() == [1, 2, 1] and gt['label'].dtype == np.int32   # inside an image: np.unique's row order
    f32 = lambda vals: [float(np.float32(v)) for v in vals]                   # float32-rounded like COCOAnnotationTransform
    assert gt['x1'].tolist() == f32([0.1, 0.1, 0.5]) and gt['y2'].tolist() == [float(np.float32(70) / np.float32(200)), f32([0.4])[0], 0.75]
    assert E.pack_ground_truth(gt) is gt
    assert E.thresholds(gt, 'waymo').tolist() == [[0.7], [0.5], [0.5], [0.5]] and E.thresholds(gt, 'voc').shape == (4, 2)
    with pytest.raises(ValueError, match='waymo'):
        E.thresholds(gt, 'coco')


def test_dict_and_prediction_store_give_the_same_columns():
    from waymo_2d_tracking_amd.detnet.trainer import Predictions
    gt = E.pack_ground_truth(annotations())
    store = Predictions(['vehicle', 'pedestrian', 'sign', 'cyclist'])
    for k, v in dict_set().items():
        store[k] = v
    a, b = E.pack_detections(gt, [dict_set()]), E.pack_detections(gt, [store, dict_set()])
    assert a['set_row_offsets'].tolist() == [0, 7] and b['set_row_offsets'].tolist() == [0, 7, 14]
    assert a['image_det_offsets'].tolist() == [[0, 3, 6, 7]] and b['image_det_offsets'].tolist() == [[0, 3, 6, 7]] * 2
    assert a['category'].tolist() == [1, 1, 4, 1, 2, 2, 3]                     # image order, class by class, stored order
    assert a['conf'].tolist() == [float(np.float32(v)) for v in (0.9, 0.005, 0.5, 0.7, 0.6, 0.8, 0.3)]
    for k in E.DET_COLUMNS + ('category',):
        assert a[k].dtype == (np.int32 if k == 'category' else np.float64)
        assert np.array_equal(b[k][:7], a[k]) and np.array_equal(b[k][7:], a[k]), k
    assert a['classes'] == [[('vehicle', 1), ('pedestrian', 2), ('sign', 3), ('cyclist', 4)]]
    # a store with other class names: only the classes the ground truth knows are evaluated
    other = Predictions(['cyclist', 'tram'])
    other['a/1/FRONT'] = [np.asarray([[0.5, 0.5, 0.5, 0.5, 0.5]], np.float32), np.asarray([[0.9, 0.5, 0.5, 0.5, 0.5]], np.float32)]
    c = E.pack_detections(gt, [other])
    assert c['category'].tolist() == [4] and c['classes'] == [[('cyclist', 4)]] and c['source_row'].tolist() == [0]


def wire_rows():
    return [{'image_id': 'b/2/FRONT', 'category_id': 1, 'bbox': [100, 50, 51, 25], 'score': 0.7},       # classes ascend inside an image, as
            {'image_id': 'a/1/FRONT', 'category_id': 1, 'bbox': [41, 19, 99, 51], 'score': 0.91234},     # load_prediction writes them
            {'image_id': 'b/2/FRONT', 'category_id': 2, 'bbox': [25, 12, 50, 25], 'score': 0.8},
            {'image_id': 'a/1/FRONT', 'category_id': 4, 'bbox': [3, 7, 11, 13], 'score': 0.5}]


def test_wire_rows_are_the_inverse_of_load_prediction_in_the_stated_operation_order():
    gt = E.pack_ground_truth(annotations())
    p = E.pack_detections(gt, [wire_rows()])
    assert p['image_det_offsets'].tolist() == [[0, 2, 4, 4]] and p['source_row'].tolist() == [1, 3, 0, 2]     # image order, file order inside
    built = {}
    for r in wire_rows():
        W, H = gt['sizes'][r['image_id']]
        x, y, w, h = (float(v) for v in r['bbox'])
        per_class = built.setdefault(r['image_id'], [[], [], [], []])
        per_class[r['category_id'] - 1].append([r['score'], (x + w / 2) / W, (y + h / 2) / H, w / W, h / H])
    q = E.pack_detections(gt, [{k: [np.asarray(c, np.float64).reshape(-1, 5) for c in v] for k, v in built.items()}])
    for k in E.DET_COLUMNS + ('category', 'image_det_offsets'):
        assert np.array_equal(p[k], q[k]), k


def test_json_form_round_trips_through_the_export_writer(tmp_path):
    from waymo_2d_tracking_amd.detnet.export import write_detections_json
    gt = E.pack_ground_truth(annotations())
    rows = wire_rows()
    ids = ['b/2/FRONT', 'a/1/FRONT']
    cols = dict(image=np.asarray([ids.index(r['image_id']) for r in rows], np.int32), category=np.asarray([r['category_id'] for r in rows], np.int32),
                bbox=np.asarray([r['bbox'] for r in rows], np.int64), score=np.asarray([r['score'] for r in rows]))
    path = tmp_path / 'dets.json'
    write_detections_json(path, ids, cols)
    assert json.load(open(path)) == rows
    a, b = E.pack_detections(gt, [str(path)]), E.pack_detections(gt, [rows])
    for k in E.DET_COLUMNS + ('category', 'image_det_offsets', 'source_row'):
        assert np.array_equal(a[k], b[k]), k
    c = E.pack_detections(gt, [path])                                           # a pathlib.Path works too
    assert np.array_equal(c['conf'], a['conf'])


def test_layout_errors_name_the_image():
    gt = E.pack_ground_truth(annotations())
    with pytest.raises(_lib.WaymoTrackError, match=r'WT_ERR_INVALID.*image q/1/FRONT'):
        E.pack_detections(gt, [wire_rows() + [{'image_id': 'q/1/FRONT', 'category_id': 1, 'bbox': [0, 0, 5, 5], 'score': 0.5}]])
    with pytest.raises(_lib.WaymoTrackError, match=r'WT_ERR_INVALID.*category_id 7 outside 1\.\.4 in image a/1/FRONT'):
        E.pack_detections(gt, [wire_rows() + [{'image_id': 'a/1/FRONT', 'category_id': 7, 'bbox': [0, 0, 5, 5], 'score': 0.5}]])
    bad = dict_set()
    bad['b/2/FRONT'] = bad['b/2/FRONT'][:3]
    with pytest.raises(_lib.WaymoTrackError, match=r'image b/2/FRONT has 3 class arrays'):
        E.pack_detections(gt, [bad])
    bad = dict_set()
    bad['a/1/FRONT'][3] = np.zeros((2, 4))
    with pytest.raises(_lib.WaymoTrackError, match=r'image a/1/FRONT, class cyclist'):
        E.pack_detections(gt, [bad])
    with pytest.raises(ValueError, match='at least one'):
        E.pack_detections(gt, [])
    with pytest.raises(TypeError):
        E.pack_detections(gt, [42])
    with pytest.raises(ValueError, match='2 min_conf values for 3 results'):
        E._min_conf([0.1, 0.2], 3)
    assert E._min_conf(0.01, 3).tolist() == [0.01] * 3


def test_command_lines():
    args = E.build_parser().parse_args(['--annotations', 'GT.json', 'A.json', 'B.json', '--metric', 'voc', '--min-conf', '0.05', '--json', 'o.json'])
    assert args.detections == ['A.json', 'B.json'] and args.metric == 'voc' and args.min_conf == 0.05 and args.json == 'o.json' and not args.sweep
    assert E.build_parser().parse_args(['--annotations', 'GT.json', 'A.json']).min_conf == 0.01
    args = E.build_parser().parse_args(['--annotations', 'GT.json', '--sweep', 'A.json', 'B.json', '--method', 'soft_nms,nms', '--iou-grid', '0.4:0.8:0.05',
                                        '--cut-grid', '0.9,1.0', '--min-score-grid', '0,0.01', '--weights', '1,1'])
    assert args.sweep == ['A.json', 'B.json'] and args.detections == [] and args.weights == '1,1'
    grid = E.grid_from_args(args)
    assert grid == {'method': ['soft_nms', 'nms'], 'iou_thresh': [0.4, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8], 'soft_nms_cut': [0.9, 1.0],
                    'min_score': [0.0, 0.01]}
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(['A.json'])                                 # --annotations is required
    with pytest.raises(SystemExit):
        E.main(['--annotations', 'GT.json'])
    with pytest.raises(SystemExit):
        E.main(['--annotations', 'GT.json', '--sweep', 'A.json'])
    line = E.flag_line({'method': 'soft_nms', 'iou_thresh': 0.55, 'soft_nms_cut': 0.9, 'min_score': 0.01})
    assert line == '-m soft_nms --iou-thresh=0.55 --soft-nms-cut=0.9 --min-score=0.01'
    from waymo_2d_tracking_amd.detnet import ensemble
    back = ensemble.build_parser().parse_args(['A.json', 'B.json', '-o', 'O.json'] + line.split())
    assert (back.method, back.iou_thresh, back.soft_nms_cut, back.min_score) == ('soft_nms', 0.55, 0.9, 0.01)


def test_eval_gpu_is_opt_in_and_needs_eval():
    from waymo_2d_tracking_amd.detnet import inference
    parser = inference.build_parser()
    assert parser.parse_args(['--eval', '--annotations', 'GT.json']).eval_gpu is False
    with pytest.raises(ValueError, match='--eval-gpu'):
        inference.check_supported(parser.parse_args(['--eval-gpu', '--export', 'x.json']))
    inference.check_supported(parser.parse_args(['--eval-gpu', '--eval', '--annotations', 'GT.json']))


def test_summary_has_the_keys_and_nesting_of_evaluate_detections():
    from waymo_2d_tracking_amd.detnet.data import metric as M
    gt = E.pack_ground_truth(annotations())
    p = E.pack_detections(gt, [dict_set()])
    for metric in ('waymo', 'voc'):
        thr = E.thresholds(gt, metric)
        z = np.zeros((4, thr.shape[1], 4))
        r = E.DetResult(metric, thr, p['classes'][0], z, z, z.astype(np.int64), z.astype(np.int64), z.astype(np.int64))
        ev = M.evaluate_detections(dict_set(), annotations(), metric=metric)
        s = r.summary()
        assert list(s) == list(ev)
        for k, v in ev.items():
            if isinstance(v, dict):
                assert list(s[k]) == list(v), k
                assert [type(x) for x in s[k].values()] == [type(x) for x in v.values()], k
        assert len(r.lines()) == 5 and r.lines()[-1].startswith('* mean AP over classes with ground truth')


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason='a GPU is present: tests/test_gpu_det_eval.py covers that case')
def test_without_a_gpu_the_calls_fail_loudly():
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_NO_DEVICE'):
        E.evaluate_detection_sets(annotations(), [dict_set()])


def test_the_module_does_not_import_the_oracle():
    import sys
    src = open(E.__file__).read()
    assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M)
    assert 'oracle' not in src and 'det_ap_ref' not in src
    assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules if sys.modules[m] is not None and
                   getattr(sys.modules[m], '__file__', None) == E.__file__)
