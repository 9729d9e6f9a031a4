"""Device ensemble of several TTA views' wire slots (wt_ensemble_slots_dev / devpath.SlotEnsemble) against the host
composition of the file route (tests/view_ensemble_ref.py), the reference fixture G2, numpy's rounding, graph capture and
the multi-view DetectTrackPipeline."""
import json
import os

import numpy as np
import pytest
import torch

from view_ensemble_ref import host_merge_slots, random_view_slots

pytestmark = pytest.mark.gpu

METHODS = ('weighted_fusion', 'nms', 'soft_nms')


def _device_merge(xywhs, cat, n_frames, slots, weights, n_categories, method, thr, cut, min_score):
    from waymo_2d_tracking_amd.devpath import SlotEnsemble
    ens = SlotEnsemble(n_frames, slots, weights, n_categories, method, thr, cut, min_score)
    ox, oc, on = ens.run(torch.from_numpy(np.ascontiguousarray(xywhs)).cuda(), torch.from_numpy(np.ascontiguousarray(cat)).cuda())
    torch.cuda.synchronize()
    return ox.cpu().numpy(), oc.cpu().numpy(), on.cpu().numpy()


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('K', [2, 3, 5])
def test_slots_match_host_composition(oracle, method, K):
    rng = np.random.default_rng(100 * K + len(method))
    F, S, C = 12, 100, 4
    xywhs, cat = random_view_slots(rng, K, F, S, C)
    weights = [1.0, 0.8, 0.55, 0.9, 0.7][:K]
    thr, cut, min_score = 0.5, 0.9, 0.01
    got = _device_merge(xywhs, cat, F, S, weights, C, method, thr, cut, min_score)
    exp = host_merge_slots(oracle, xywhs, cat, F, S, weights, method, thr, cut, min_score)
    assert np.array_equal(got[2], exp[2])
    assert np.array_equal(got[1], exp[1])
    assert np.array_equal(got[0], exp[0])
    assert exp[2].sum() > 0


def test_eight_views_global_scratch_path(oracle):
    """K = 8 at S = 100: the fusion group memory exceeds 64 KiB of LDS and runs on the global scratch."""
    rng = np.random.default_rng(8)
    F, S, C, K = 3, 100, 4, 8
    xywhs, cat = random_view_slots(rng, K, F, S, C)
    weights = [1.0 - 0.05 * k for k in range(K)]
    for method in METHODS:
        got = _device_merge(xywhs, cat, F, S, weights, C, method, 0.55, 0.95, 0.0)
        exp = host_merge_slots(oracle, xywhs, cat, F, S, weights, method, 0.55, 0.95, 0.0)
        for a, b in zip(got, exp):
            assert np.array_equal(a, b), method


@pytest.mark.parametrize('method', ['soft_nms', 'weighted_fusion'])
def test_reference_fixture_g2(golden_dir, method):
    exp = json.load(open(os.path.join(golden_dir, 'ensemble_g2_expected.json')))
    subs = [json.load(open(os.path.join(golden_dir, 'ensemble_g2_input%d.json' % i))) for i in range(3)]
    images = sorted({r['image_id'] for s in subs for r in s})
    frame = {name: f for f, name in enumerate(images)}
    F, S, C, K = len(images), 40, 4, 3
    xywhs, cat = np.zeros((K, 5, F * S)), np.zeros((K, F * S), np.int32)
    for k, s in enumerate(subs):
        used = np.zeros(F, np.int64)
        for r in s:
            f = frame[r['image_id']]
            i = f * S + int(used[f])
            used[f] += 1
            assert used[f] <= S
            xywhs[k, 0:4, i] = r['bbox']
            xywhs[k, 4, i] = r['score']
            cat[k, i] = r['category_id']
    ox, oc, on = _device_merge(xywhs, cat, F, S, exp['weights'], C, method, exp['iou_thresh'], exp['soft_nms_cut'], exp['min_score'])
    rows = []
    for f in range(F):
        for j in range(f * K * S, f * K * S + int(on[f])):
            rows.append({'image_id': images[f], 'category_id': int(oc[j]), 'bbox': [int(v) for v in ox[0:4, j]], 'score': float(ox[4, j])})
    want = exp['outputs'][method]
    assert len(rows) == len(want)
    assert rows == want


def test_scores_round_like_numpy():
    """Single-row nms groups with scores at and beside 5-decimal halfway points: the output is round(np.float64(s), 5)."""
    rng = np.random.default_rng(5)
    halves = (rng.integers(0, 100000, 1000) + 0.5) / 1e5
    s = [0.649415, np.nextafter(0.649415, 0.0), np.nextafter(0.649415, 1.0), 0.000015, 0.5, 0.999995]
    s += halves.tolist() + np.nextafter(halves, 0.0).tolist() + np.nextafter(halves, 1.0).tolist()
    s += rng.uniform(0.0, 1.0, 500).tolist()
    s = np.asarray([v for v in s if v > 0], np.float64)
    F, S = len(s), 1
    xywhs = np.zeros((1, 5, F))
    xywhs[0, 0:4] = np.array([[10.0], [20.0], [30.0], [40.0]])
    xywhs[0, 4] = s
    cat = np.ones((1, F), np.int32)
    ox, oc, on = _device_merge(xywhs, cat, F, S, [1.0], 1, 'nms', 0.5, 1.0, 0.0)
    assert np.array_equal(on, np.ones(F, np.int64))
    want = np.asarray([round(np.float64(v), 5) for v in s], np.float64)
    assert np.array_equal(ox[4], want)
    assert ox[4][0] == 0.64942                                   # numpy's around; CPython's round gives 0.64941
    assert np.array_equal(ox[0:4, 0], [10.0, 20.0, 30.0, 40.0])


def test_graph_capture_replay_equals_eager():
    from waymo_2d_tracking_amd.devpath import SlotEnsemble
    F, S, C, K = 6, 100, 4, 2
    ens = SlotEnsemble(F, S, [1.0, 0.7], C, 'soft_nms', 0.5, 0.9, 0.01)
    sx = torch.zeros((K, 5, F * S), dtype=torch.float64, device='cuda')
    sc = torch.zeros((K, F * S), dtype=torch.int32, device='cuda')
    out = ens.outputs()
    ens.run(sx, sc, out=out)                                      # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ens.run(sx, sc, out=out)
    for seed in (1, 2, 3):
        x, c = random_view_slots(np.random.default_rng(seed), K, F, S, C)
        sx.copy_(torch.from_numpy(x))
        sc.copy_(torch.from_numpy(c))
        g.replay()
        torch.cuda.synchronize()
        got = [t.cpu().numpy().copy() for t in out]
        eager = ens.run(sx.clone(), sc.clone())
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert np.array_equal(a, b.cpu().numpy()), seed
        assert got[2].sum() > 0


VIEWS = ('orig', 'x1.5,hflip')
VIEW_ENS = dict(method='soft_nms', iou_thresh=0.5, soft_nms_cut=0.9, min_score=0.01, weights=[1.0, 0.8])


@pytest.fixture(scope='module')
def view_model():
    from waymo_2d_tracking_amd.detnet.nn.detectron2_det import Detectron2Det
    return Detectron2Det(seed=0).cuda().eval()


def _run_views_pipeline(model, n_inflight, defer, steps):
    from waymo_2d_tracking_amd.bench_e2e import DetectTrackPipeline
    pipe = DetectTrackPipeline(5, 2, height=256, width=384, seed=0, model=model, segment_frames=6, n_inflight=n_inflight,
                               deterministic=True, defer_tracking=defer, views=VIEWS, view_ensemble=VIEW_ENS)
    for _ in range(steps):
        pipe.step()
    pipe.flush()
    return pipe


def test_pipeline_views_merge_track_and_lanes(oracle, view_model):
    """3 steps per segment (segment_frames 6 = 3 chunks of 2 frames), then a 4th step wraps into a new segment."""
    from waymo_2d_tracking_amd.bench_e2e import check_against
    results = {}
    for n_inflight, defer in ((1, False), (2, False), (2, True), (1, True)):
        pipe = _run_views_pipeline(view_model, n_inflight, defer, 3)
        assert pipe.slots == 2 * 100 and pipe.tracker.max_frame == 200
        h = pipe.view_history()
        assert h['xywhs'].shape == (3, 2, 5, 10 * 100)
        for c in range(3):
            exp = host_merge_slots(oracle, h['xywhs'][c], h['category'][c], 10, 100, VIEW_ENS['weights'], 'soft_nms', 0.5, 0.9, 0.01)
            assert np.array_equal(h['merged_counts'][c], exp[2]), (n_inflight, defer, c)
            assert np.array_equal(h['merged_category'][c], exp[1]), (n_inflight, defer, c)
            assert np.array_equal(h['merged_xywhs'][c], exp[0]), (n_inflight, defer, c)
        rep = check_against(pipe, oracle.track_streams)
        assert rep['ok'], rep
        assert rep['dets'] > 0 and rep['rows'] > 0
        results[(n_inflight, defer)] = (h, pipe.history()[1])
        pipe.step()                                              # segment wrap: fresh trackers, ring slot 0 reused
        pipe.flush()
        assert pipe.segments_done == 1 and pipe.chunk == 1
        rep = check_against(pipe, oracle.track_streams)
        assert rep['ok'], rep
        h1 = pipe.view_history()
        exp = host_merge_slots(oracle, h1['xywhs'][0], h1['category'][0], 10, 100, VIEW_ENS['weights'], 'soft_nms', 0.5, 0.9, 0.01)
        assert np.array_equal(h1['merged_xywhs'][0], exp[0]) and np.array_equal(h1['merged_category'][0], exp[1])
        del pipe
        torch.cuda.empty_cache()
    ref_h, ref_rows = results[(1, False)]
    for key, (h, rows) in results.items():
        for k in ('xywhs', 'category', 'merged_xywhs', 'merged_category', 'merged_counts'):
            assert np.array_equal(h[k], ref_h[k]), (key, k)
        for k in ref_rows:
            assert np.array_equal(rows[k], ref_rows[k]), (key, k)


def _synthetic_view_rows(rng, n_images, K):
    """Export-shaped rows of K views (images in data-set order, int boxes, 5-decimal scores).  Image 0 and image 3 have rows
    in view 1 only, image 5 has none at all: the merged file's image order is not the data-set order."""
    views = []
    for k in range(K):
        cols = dict(image=[], category=[], bbox=[], score=[])
        for i in range(n_images):
            if i == 5 or (i in (0, 3) and k == 0):
                continue
            n = int(rng.integers(1, 30))
            base = np.stack([rng.integers(0, 600, n), rng.integers(0, 400, n), rng.integers(0, 90, n), rng.integers(1, 90, n)], 1)
            for j in range(n):
                cols['image'].append(i); cols['category'].append(int(rng.integers(1, 5)))
                cols['bbox'].append(base[j] + rng.integers(-3, 4, 4) * (rng.random() < 0.7))
                cols['score'].append(round(float(rng.uniform(0, 1)), 5))
        views.append(dict(image=np.asarray(cols['image'], np.int32), category=np.asarray(cols['category'], np.int32),
                          bbox=np.asarray(cols['bbox'], np.int64).reshape(-1, 4), score=np.asarray(cols['score'], np.float64)))
    return views


@pytest.mark.parametrize('method', METHODS)
def test_merged_view_rows_are_byte_identical_to_the_ensemble_cli(tmp_path, method):
    from waymo_2d_tracking_amd.detnet import ensemble as E
    from waymo_2d_tracking_amd.detnet.export import write_detections_json
    from waymo_2d_tracking_amd.detnet.inference import merge_view_rows
    image_ids = ['seg/%d/FRONT' % (100 + i) for i in range(8)]
    views = _synthetic_view_rows(np.random.default_rng(len(method)), len(image_ids), 2)
    files = []
    for k, r in enumerate(views):
        files.append(str(tmp_path / ('view%d.json' % k)))
        write_detections_json(files[-1], image_ids, r)
    E.main(files + ['-o', str(tmp_path / 'file_route.json'), '-m', method, '--iou-thresh', '0.55', '--soft-nms-cut', '0.9',
                    '--min-score', '0.05'])
    rows = merge_view_rows(image_ids, views, [1.0, 1.0], method, 0.55, 0.9, 0.05, batch_frames=3)
    write_detections_json(tmp_path / 'device.json', image_ids, rows)
    got, want = (tmp_path / 'device.json').read_bytes(), (tmp_path / 'file_route.json').read_bytes()
    order = list(dict.fromkeys(rows['image'].tolist()))
    assert order[0] == 1 and order[-2:] == [0, 3]                      # images 0 and 3 (view 1 only) come after view 0's images
    if method != 'weighted_fusion':
        assert got == want
        return
    # fusion averages 5-decimal scores, so half-way points are common: the device rounds them like the reference (numpy's around),
    # the host route with Python's round - those rows differ by one unit of the 5th decimal, nothing else does
    g, w = json.loads(got), json.loads(want)
    assert [(r['image_id'], r['category_id'], r['bbox']) for r in g] == [(r['image_id'], r['category_id'], r['bbox']) for r in w]
    diff = [(a['score'], b['score']) for a, b in zip(g, w) if a['score'] != b['score']]
    assert all(abs(a - b) <= 1.0000001e-5 for a, b in diff)


def test_inference_cli_views_equal_the_file_route(tmp_path):
    """inference.py --views against the route it replaces: --export-views files, detnet.ensemble over them, --tta per view."""
    from PIL import Image
    from test_gpu_detector import _random_model_file, _rows_match
    from waymo_2d_tracking_amd.detnet import ensemble as E
    from waymo_2d_tracking_amd.detnet import inference as I
    rng = np.random.default_rng(1)
    root = tmp_path / 'images'
    for i in range(7):
        cam = ('FRONT', 'SIDE_LEFT')[i % 2]
        d = root / 'seg' / str(100 + i)
        d.mkdir(parents=True, exist_ok=True)
        arr = rng.integers(30, 200, ((96, 64)[i % 2], 160, 3), dtype=np.uint8)
        Image.fromarray(arr).save(d / (cam + '.jpg'), quality=92)
    model = _random_model_file(tmp_path)
    flags = ['--views-method', 'soft_nms', '--views-soft-nms-cut', '0.9', '--views-min-score', '0.01']
    merged, vdir = tmp_path / 'M.json', tmp_path / 'V'
    I.main(['-m', model, '-i', str(root), '--batch-size=1', '--views', 'orig;x1.5,hflip', '--export', str(merged),
            '--export-views', str(vdir)] + flags)
    E.main([str(vdir / 'view0.json'), str(vdir / 'view1.json'), '-o', str(tmp_path / 'F.json'), '-m', 'soft_nms',
            '--soft-nms-cut', '0.9', '--min-score', '0.01'])
    assert len(json.load(open(merged))) > 0
    assert merged.read_bytes() == (tmp_path / 'F.json').read_bytes()
    for k, spec in enumerate(('orig', 'x1.5,hflip')):
        single = tmp_path / ('tta%d.json' % k)
        I.main(['-m', model, '-i', str(root), '--batch-size=1', '--tta', spec, '--export', str(single)])
        _rows_match(json.load(open(vdir / ('view%d.json' % k))), json.load(open(single)))
