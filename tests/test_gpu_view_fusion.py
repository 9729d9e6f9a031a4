"""Weighted boxes fusion / NMW of several TTA views' wire slots on the device (wt_fuse_slots_dev, devpath.SlotEnsemble with method
'weighted_fusion_b' / 'nmw') against the host composition of the ensemble_b file route (tests/view_fusion_ref.py: plain-Python
merge, compared with ==), numpy's rounding, graph capture, the error returns, the multi-view DetectTrackPipeline, and
inference.merge_view_rows / `inference.py --views` against `python -m detnet.ensemble_b`."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from view_ensemble_ref import random_view_slots
from view_fusion_ref import WSUM_MIN_SCORE, WSUM_WEIGHTS, host_fuse_slots, wsum_case

pytestmark = pytest.mark.gpu

METHODS = ('weighted_fusion_b', 'nmw')
EB_NAME = {'weighted_fusion_b': 'weighted_fusion', 'nmw': 'nmw'}          # the -m of detnet.ensemble_b
WEIGHTS = [1.0, 0.8, 0.55, 0.9, 0.7, 0.95, 0.6, 0.85, 0.75, 0.65, 0.5, 0.45, 0.4, 0.35, 0.3, 0.25]


def _device_merge(xywhs, cat, n_frames, slots, weights, n_categories, method, thr, min_score):
    from waymo_2d_tracking_amd.devpath import SlotEnsemble
    ens = SlotEnsemble(n_frames, slots, weights, n_categories, method, thr, 1.0, min_score)
    ox, oc, on = ens.run(torch.from_numpy(np.ascontiguousarray(xywhs)).cuda(), torch.from_numpy(np.ascontiguousarray(cat)).cuda())
    torch.cuda.synchronize()
    return ox.cpu().numpy(), oc.cpu().numpy(), on.cpu().numpy()


def _assert_same(got, exp, what=None):
    assert np.array_equal(got[2], exp[2]), what
    assert np.array_equal(got[1], exp[1]), what
    assert np.array_equal(got[0], exp[0]), what


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('K', [1, 2, 3])
def test_slots_match_host_composition(method, K):
    """F = 4, S = 20 (LDS path); three thresholds, min_score 0.01 and -inf, unequal weights."""
    rng = np.random.default_rng(100 * K + len(method))
    F, S, Cn = 4, 20, 4
    xywhs, cat = random_view_slots(rng, K, F, S, Cn)
    rows = 0
    for thr in (0.3, 0.55, 0.75):
        for min_score in (0.01, -np.inf):
            got = _device_merge(xywhs, cat, F, S, WEIGHTS[:K], Cn, method, thr, min_score)
            exp = host_fuse_slots(xywhs, cat, F, S, WEIGHTS[:K], Cn, method, thr, min_score)
            _assert_same(got, exp, (thr, min_score))
            rows += int(exp[2].sum())
    assert rows > 0


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('K,S', [(13, 37), (2, 241), (16, 31)])
def test_capacity_edge_and_scratch_path(method, K, S):
    """K * S = 481 is the last shape whose group state fits LDS, 482 the first on the workspace slice; K = 16 is the most views.
    Frame 1 is dense: every one of its K * S slots holds a kept row of category 2, so that group fills its arrays to the end."""
    from waymo_2d_tracking_amd import _lib
    lds_rows = int(_lib.lib().wt_fuse_groups_lds_rows())
    assert lds_rows == 481 and (K * S <= lds_rows) == ((K, S) == (13, 37))
    rng = np.random.default_rng(K * S)
    F, Cn = 2, 4
    xywhs, cat = random_view_slots(rng, K, F, S, Cn)
    objects = np.stack([rng.integers(0, 1800, 40), rng.integers(0, 1200, 40), rng.integers(20, 300, 40), rng.integers(20, 200, 40)], 0)
    for k in range(K):
        pick = rng.integers(0, 40, S)
        xywhs[k, 0:4, S:2 * S] = objects[:, pick] + rng.integers(-4, 5, (4, S))
        xywhs[k, 4, S:2 * S] = np.round(rng.uniform(0.05, 1.0, S), 5)
        cat[k, S:2 * S] = 2
    got = _device_merge(xywhs, cat, F, S, WEIGHTS[:K], Cn, method, 0.5, 0.01)
    exp = host_fuse_slots(xywhs, cat, F, S, WEIGHTS[:K], Cn, method, 0.5, 0.01)
    _assert_same(got, exp)
    assert 0 < exp[2][1] < K * S and exp[2][0] > 0


def _edge_frames(K, S):
    """Frames: 0 no kept row (zero width, negative height, score below min_score, category out of range); 1 one category only;
    2, 4, 6, 7 one group of exactly 1, 63, 64, 65 identical boxes spread over the views; 3 and 5 empty."""
    F, Cn = 8, 3
    xywhs, cat = np.zeros((K, 5, F * S)), np.zeros((K, F * S), np.int32)
    rng = np.random.default_rng(7)
    bad = [([5, 5, 0, 10, 0.9], 1), ([5, 5, 10, -1, 0.9], 2), ([5, 5, 10, 10, 0.001], 3), ([5, 5, 10, 10, 0.9], 4), ([5, 5, 10, 10, 0.9], -1)]
    for j, (row, c) in enumerate(bad):
        xywhs[j % K, :, (j // K) * 2] = row
        cat[j % K, (j // K) * 2] = c
    for k in range(K):
        n = 5 + k
        xywhs[k, 0:4, S:S + n] = np.stack([rng.integers(0, 60, n), rng.integers(0, 60, n), rng.integers(10, 40, n), rng.integers(10, 40, n)], 0)
        xywhs[k, 4, S:S + n] = np.round(rng.uniform(0.05, 1.0, n), 5)
        cat[k, S:S + n] = 2
    for f, n in ((2, 1), (4, 63), (6, 64), (7, 65)):
        for j in range(n):
            k, s = j % K, j // K
            xywhs[k, :, f * S + s] = [40.0, 30.0, 50.0, 60.0, round(0.2 + 0.01 * (j % 7), 5)]
            cat[k, f * S + s] = 3
    return xywhs, cat, F, Cn


@pytest.mark.parametrize('method', METHODS)
def test_empty_and_near_empty_frames(method):
    K, S = 3, 24
    xywhs, cat, F, Cn = _edge_frames(K, S)
    got = _device_merge(xywhs, cat, F, S, WEIGHTS[:K], Cn, method, 0.5, 0.01)
    exp = host_fuse_slots(xywhs, cat, F, S, WEIGHTS[:K], Cn, method, 0.5, 0.01)
    _assert_same(got, exp)
    assert exp[2].tolist()[0] == 0 and exp[2].tolist()[2:] == [1, 0, 1, 0, 1, 1] and exp[2][1] > 0
    assert set(exp[1][K * S:2 * K * S].tolist()) == {0, 2}


def _raw_call(xywhs, cat, F, S, K, weights, Cn, method, thr, min_score, out, ws, ws_bytes):
    from waymo_2d_tracking_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return _lib.lib().wt_fuse_slots_dev(p(xywhs), p(cat), C.c_int64(F), C.c_int64(S), C.c_int(K), p(weights), C.c_int(Cn), C.c_int(method),
                                        C.c_double(thr), C.c_double(min_score), p(out[0]), p(out[1]), p(out[2]), p(ws), C.c_size_t(ws_bytes), None)


def _sentinel_outputs(F, S, K):
    return (torch.full((5, max(F * K * S, 1)), -7.0, dtype=torch.float64, device='cuda'),
            torch.full((max(F * K * S, 1),), -7, dtype=torch.int32, device='cuda'), torch.full((max(F, 1),), -7, dtype=torch.int64, device='cuda'))


def _untouched(out):
    torch.cuda.synchronize()
    return all(bool((t == -7).all()) for t in out)


def test_zero_frames_and_zero_slots_are_ok_and_write_nothing():
    from waymo_2d_tracking_amd import _lib
    lib = _lib.lib()
    w = torch.ones(2, dtype=torch.float64, device='cuda')
    ws = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    for F, S in ((0, 20), (3, 0)):
        assert int(lib.wt_fuse_slots_workspace(C.c_int64(F), C.c_int64(S), C.c_int(2), C.c_int(4), C.c_int(1))) > 0
        out = _sentinel_outputs(F, S, 2)
        x = torch.zeros((2, 5, max(F * S, 1)), dtype=torch.float64, device='cuda')
        c = torch.zeros((2, max(F * S, 1)), dtype=torch.int32, device='cuda')
        assert _raw_call(x, c, F, S, 2, w, 4, 1, 0.5, 0.0, out, ws, 4096) == 0
        assert _untouched(out)


def test_error_returns_come_before_any_launch():
    from waymo_2d_tracking_amd import _lib
    lib = _lib.lib()
    F, S, K, Cn = 2, 20, 2, 4
    xywhs, cat = random_view_slots(np.random.default_rng(3), K, F, S, Cn)
    x, c = torch.from_numpy(xywhs).cuda(), torch.from_numpy(cat).cuda()
    w = torch.ones(16, dtype=torch.float64, device='cuda')
    size = lambda f, s, k, cn, m: int(lib.wt_fuse_slots_workspace(C.c_int64(f), C.c_int64(s), C.c_int(k), C.c_int(cn), C.c_int(m)))
    need = size(F, S, K, Cn, 0)
    assert need > 0 and need == size(F, S, K, Cn, 1)
    for bad in ((F, S, K, Cn, 2), (F, S, K, Cn, -1), (F, S, 0, Cn, 0), (F, S, 17, Cn, 0), (-1, S, K, Cn, 0), (F, -1, K, Cn, 0), (F, S, K, 0, 0)):
        assert size(*bad) == 0, bad
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    out = _sentinel_outputs(F, S, K)
    INVALID, CAPACITY = 1, 4
    assert _raw_call(x, c, F, S, K, w, Cn, 2, 0.5, 0.0, out, ws, need) == INVALID                    # bad method
    assert _raw_call(x, c, F, S, K, w, Cn, -1, 0.5, 0.0, out, ws, need) == INVALID
    assert _raw_call(x, c, F, S, 0, w, Cn, 0, 0.5, 0.0, out, ws, need) == INVALID                    # K = 0, K = 17
    assert _raw_call(x, c, F, S, 17, w, Cn, 0, 0.5, 0.0, out, ws, need) == INVALID
    assert _raw_call(x, c, -1, S, K, w, Cn, 0, 0.5, 0.0, out, ws, need) == INVALID                   # bad shapes
    assert _raw_call(x, c, F, S, K, w, 0, 0, 0.5, 0.0, out, ws, need) == INVALID
    assert _raw_call(x, c, F, S, K, w, Cn, 0, 0.5, 0.0, out, ws, need - 1) == CAPACITY               # one byte short
    assert b'too small' in lib.wt_last_error()
    for hole in range(7):                                                                            # null pointers
        a = [x, c, w, out[0], out[1], out[2], ws]
        a[hole] = None
        assert _raw_call(a[0], a[1], F, S, K, a[2], Cn, 0, 0.5, 0.0, (a[3], a[4], a[5]), a[6], need) == INVALID, hole
    assert _untouched(out)
    assert _raw_call(x, c, F, S, K, w, Cn, 0, 0.5, 0.0, out, ws, need) == 0                          # and the good call still runs
    torch.cuda.synchronize()
    exp = host_fuse_slots(xywhs, cat, F, S, [1.0, 1.0], Cn, 'weighted_fusion_b', 0.5, 0.0)
    _assert_same([t.cpu().numpy() for t in out], exp)


@pytest.mark.parametrize('method', METHODS)
def test_wsum_hand_worked_case(method):
    xywhs, cat, F, S, Cn, expected = wsum_case()
    got = _device_merge(xywhs, cat, F, S, WSUM_WEIGHTS, Cn, method, 0.5, WSUM_MIN_SCORE)
    _assert_same(got, expected[method])


@pytest.mark.parametrize('method', METHODS)
def test_scores_round_like_numpy(method):
    """Single-row groups (conf = the row's score under both rules, wsum = 1) at and beside 5-decimal half-way points."""
    rng = np.random.default_rng(5)
    halves = (rng.integers(0, 100000, 1000) + 0.5) / 1e5
    s = [0.649415, np.nextafter(0.649415, 0.0), np.nextafter(0.649415, 1.0), 0.000015, 0.5, 0.999995]
    s += halves.tolist() + np.nextafter(halves, 0.0).tolist() + np.nextafter(halves, 1.0).tolist()
    s += rng.uniform(0.0, 1.0, 500).tolist()
    s = np.asarray([v for v in s if v > 0], np.float64)
    F = len(s)
    xywhs = np.zeros((1, 5, F))
    xywhs[0, 0:4] = np.array([[10.5], [20.25], [30.0], [40.75]])
    xywhs[0, 4] = s
    cat = np.ones((1, F), np.int32)
    ox, oc, on = _device_merge(xywhs, cat, F, 1, [1.0], 1, method, 0.5, 0.0)
    assert np.array_equal(on, np.ones(F, np.int64))
    want = np.asarray([round(np.float64(v), 5) for v in s], np.float64)
    assert np.array_equal(ox[4], want)
    assert ox[4][0] == 0.64942                                   # numpy's around; CPython's round gives 0.64941
    assert np.array_equal(ox[0:4, 0], [10.5, 20.25, 30.0, 40.75])  # float boxes, not truncated


@pytest.mark.parametrize('method', METHODS)
def test_graph_capture_replay_equals_eager(method):
    from waymo_2d_tracking_amd.devpath import SlotEnsemble
    F, S, Cn, K = 6, 100, 4, 2
    ens = SlotEnsemble(F, S, [1.0, 0.7], Cn, method, 0.5, 1.0, 0.01)
    sx = torch.zeros((K, 5, F * S), dtype=torch.float64, device='cuda')
    sc = torch.zeros((K, F * S), dtype=torch.int32, device='cuda')
    out = ens.outputs()
    ens.run(sx, sc, out=out)                                      # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ens.run(sx, sc, out=out)
    for seed in (1, 2, 3):
        x, c = random_view_slots(np.random.default_rng(seed), K, F, S, Cn)
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


@pytest.fixture(scope='module')
def view_model():
    from waymo_2d_tracking_amd.detnet.nn.detectron2_det import Detectron2Det
    return Detectron2Det(seed=0).cuda().eval()


@pytest.mark.parametrize('method', ['weighted_fusion_b', 'nmw'])
def test_pipeline_views_fuse_and_track(oracle, view_model, method):
    """3 steps = one segment of 3 chunks of 2 frames per camera; merged slots equal the host composition, SORT equals the oracle on
    them, and the serial and the two-lane deferred settings give the same history."""
    from waymo_2d_tracking_amd.bench_e2e import DetectTrackPipeline, check_against
    ve = dict(method=method, iou_thresh=0.55, min_score=0.01, weights=[1.0, 0.8])
    results = {}
    for n_inflight, defer in ((1, False), (2, True)):
        pipe = DetectTrackPipeline(5, 2, height=256, width=384, seed=0, model=view_model, segment_frames=6, n_inflight=n_inflight,
                                   deterministic=True, defer_tracking=defer, views=VIEWS, view_ensemble=ve)
        for _ in range(3):
            pipe.step()
        pipe.flush()
        h = pipe.view_history()
        assert h['xywhs'].shape == (3, 2, 5, 10 * 100)
        for c in range(3):
            exp = host_fuse_slots(h['xywhs'][c], h['category'][c], 10, 100, pipe.view_ensemble['weights'], 4, method, 0.55, 0.01)
            assert np.array_equal(h['merged_counts'][c], exp[2]), (n_inflight, defer, c)
            assert np.array_equal(h['merged_category'][c], exp[1]), (n_inflight, defer, c)
            assert np.array_equal(h['merged_xywhs'][c], exp[0]), (n_inflight, defer, c)
        rep = check_against(pipe, oracle.track_streams)
        assert rep['ok'], rep
        assert rep['dets'] > 0 and rep['rows'] > 0
        results[(n_inflight, defer)] = (h, pipe.history()[1])
        del pipe
        torch.cuda.empty_cache()
    (ref_h, ref_rows), (h, rows) = results[(1, False)], results[(2, True)]
    for k in ('xywhs', 'category', 'merged_xywhs', 'merged_category', 'merged_counts'):
        assert np.array_equal(h[k], ref_h[k]), k
    for k in ref_rows:
        assert np.array_equal(rows[k], ref_rows[k]), k


def _by_image_and_category(rows):
    """A detection file's rows, stably regrouped by (image in first-appearance order, category): inside one (image, category) the
    file's own order stays.  ensemble_b orders an image's rows by the unrounded conf across categories, merge_view_rows by the
    5-decimal score: the two agree per category, and across categories wherever the rounded scores differ."""
    rank = {name: i for i, name in enumerate(dict.fromkeys(r['image_id'] for r in rows))}
    return sorted(rows, key=lambda r: (rank[r['image_id']], r['category_id']))


@pytest.mark.parametrize('method', METHODS)
def test_merged_view_rows_equal_the_ensemble_b_cli(tmp_path, method):
    """min_score = -inf (ensemble_b has no minimum score): image ids, categories and float boxes identical, scores within one unit of
    the 5th decimal (numpy's rounding here, CPython's round there)."""
    from test_gpu_view_ensemble import _synthetic_view_rows
    from waymo_2d_tracking_amd.detnet import ensemble_b as EB
    from waymo_2d_tracking_amd.detnet.export import write_detections_json
    from waymo_2d_tracking_amd.detnet.inference import merge_view_rows
    image_ids = ['seg/%d/FRONT' % (100 + i) for i in range(8)]
    views = _synthetic_view_rows(np.random.default_rng(len(method)), len(image_ids), 2)
    files = []
    for k, r in enumerate(views):
        files.append(str(tmp_path / ('view%d.json' % k)))
        write_detections_json(files[-1], image_ids, r)
    EB.main(files + ['-o', str(tmp_path / 'file_route.json'), '-m', EB_NAME[method], '--iou-thresh', '0.55'])
    rows = merge_view_rows(image_ids, views, [1.0, 1.0], method, 0.55, 1.0, -np.inf, batch_frames=3)
    assert rows['bbox'].dtype == np.float64
    order = list(dict.fromkeys(rows['image'].tolist()))
    assert order[0] == 1 and order[-2:] == [0, 3]                      # images 0 and 3 (view 1 only) come after view 0's images
    EB.write_detections_json(tmp_path / 'device.json', image_ids, rows)
    g, w = json.load(open(tmp_path / 'device.json')), json.load(open(tmp_path / 'file_route.json'))
    assert len(g) == len(w) > 0
    assert list(dict.fromkeys(r['image_id'] for r in g)) == list(dict.fromkeys(r['image_id'] for r in w))
    g, w = _by_image_and_category(g), _by_image_and_category(w)
    assert [(r['image_id'], r['category_id'], r['bbox']) for r in g] == [(r['image_id'], r['category_id'], r['bbox']) for r in w]
    assert all(isinstance(v, float) for r in g for v in r['bbox'])
    assert all(abs(a['score'] - b['score']) <= 1.0000001e-5 for a, b in zip(g, w))


def test_inference_cli_views_nmw_writes_the_merged_view_rows(tmp_path):
    """inference.py --views --views-method nmw: the merged file has float boxes and equals merge_view_rows of the --export-views files."""
    from PIL import Image
    from test_gpu_detector import _random_model_file
    from waymo_2d_tracking_amd.detnet import ensemble_b as EB
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
    merged, vdir = tmp_path / 'M.json', tmp_path / 'V'
    I.main(['-m', model, '-i', str(root), '--batch-size=1', '--views', 'orig;x1.5,hflip', '--export', str(merged),
            '--export-views', str(vdir), '--views-method', 'nmw', '--views-iou-thresh', '0.55', '--views-min-score', '0.01'])
    image_ids = [i for i, _ in I.list_images(root)]
    index = {name: i for i, name in enumerate(image_ids)}
    views = []
    for k in range(2):
        rs = json.load(open(vdir / ('view%d.json' % k)))
        views.append(dict(image=np.asarray([index[r['image_id']] for r in rs], np.int32), category=np.asarray([r['category_id'] for r in rs], np.int32),
                          bbox=np.asarray([r['bbox'] for r in rs], np.int64).reshape(-1, 4), score=np.asarray([r['score'] for r in rs], np.float64)))
    rows = I.merge_view_rows(image_ids, views, [1.0, 1.0], 'nmw', 0.55, 1.0, 0.01)
    assert len(rows['image']) > 0 and rows['bbox'].dtype == np.float64
    EB.write_detections_json(tmp_path / 'D.json', image_ids, rows)
    got = json.load(open(merged))
    assert len(got) > 0 and all(isinstance(v, float) for r in got for v in r['bbox'])
    assert merged.read_bytes() == (tmp_path / 'D.json').read_bytes()
