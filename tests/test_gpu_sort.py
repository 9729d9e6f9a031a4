"""HIP SORT engine (through the C ABI of libwaymotrack.so) against the reference-generated golden vectors and
against the CPU oracle on seeded inputs.  Track IDs / assignments / order bit-exact; boxes within 1e-6 of the
reference fixture (north_star: 1e-4) and bit-identical to the oracle except the libm-vs-ocml exp() of the
confidence (<= 2 ulp).  Adversarial inputs for every Munkres / association variant are in test_gpu_sort_assignment.py."""
import json
import os

import numpy as np
import pytest

from track_stage_support import predictions_of
from waymo_2d_tracking_amd.tracking import utils as T

pytestmark = pytest.mark.gpu
BOX_TOL = 1e-6


def _rows(tracks):
    return [(t['image_id'], t['category_id'], t['object_id']) for t in tracks]


@pytest.mark.parametrize('variant', ['a', 'b', 'c'])
def test_track_streams_golden(golden_dir, oracle, variant):
    exp = json.load(open(os.path.join(golden_dir, 'sort_g4_expected_%s.json' % variant)))
    p = exp['params']
    predictions = T.read_data_file(os.path.join(golden_dir, 'sort_g4_input.json'), p['score_threshold'])
    packed = T.pack_streams(predictions)
    out, births = T.track_packed(packed, p['iou_threshold'], p['max_age'], p['min_hits'], p['score_threshold'])
    assert births == exp['n_ids']
    got = T.format_tracks(packed, out)
    assert _rows(got) == _rows(exp['tracks'])
    gb = np.array([t['bbox'] + [t['score']] for t in got])
    eb = np.array([t['bbox'] + [t['score']] for t in exp['tracks']])
    np.testing.assert_allclose(gb, eb, rtol=0, atol=BOX_TOL)
    # and bit-identical boxes vs the oracle (same operation order, no FMA contraction)
    ref = oracle.track_streams(packed, p['max_age'], p['min_hits'], p['score_threshold'], p['iou_threshold'])
    assert np.array_equal(out['object_id'], ref['object_id'])
    assert np.array_equal(out['frame'], ref['frame'])
    assert np.array_equal(out['bbox'], ref['bbox'])
    np.testing.assert_allclose(out['score'], ref['score'], rtol=4e-16, atol=0)


def test_cli_track_golden(golden_dir, tmp_path, capsys):
    from waymo_2d_tracking_amd.tracking import track
    exp = json.load(open(os.path.join(golden_dir, 'sort_g4_expected_a.json')))
    T.reset_global_ids(0)
    out = tmp_path / 'tracks.json'
    rc = track.main(['--input', os.path.join(golden_dir, 'sort_g4_input.json'), '--output', str(out), '--max-age=2',
                     '--min-hits=0', '--score-threshold=0.3,0.3,1.0,0.2', '--iou-threshold=0.01,0.01,1.0,0.0'])
    assert rc == 0
    printed = capsys.readouterr().out
    assert 'duration:' in printed and 'segment-10203656353524179475' in printed
    got = json.load(open(out))
    assert _rows(got) == _rows(exp['tracks'])
    assert set(got[0].keys()) == {'image_id', 'bbox', 'score', 'category_id', 'object_id'}
    # the native-I/O default and the Python-json path write the same bytes
    T.reset_global_ids(0)
    out2 = tmp_path / 'tracks_py.json'
    assert track.main(['--input', os.path.join(golden_dir, 'sort_g4_input.json'), '--output', str(out2), '--max-age=2',
                       '--min-hits=0', '--score-threshold=0.3,0.3,1.0,0.2', '--iou-threshold=0.01,0.01,1.0,0.0',
                       '--python-io']) == 0
    assert open(out, 'rb').read() == open(out2, 'rb').read()


def test_track_sort_api_per_stream_matches_batch(golden_dir):
    """utils.track_sort called stream by stream (reference loop) == one batched call, incl. the global ID order."""
    exp = json.load(open(os.path.join(golden_dir, 'sort_g4_expected_a.json')))
    p = exp['params']
    predictions = T.read_data_file(os.path.join(golden_dir, 'sort_g4_input.json'), p['score_threshold'])
    T.reset_global_ids(0)
    out = []
    for segment_id in predictions.keys():
        for camera_id in predictions[segment_id]:
            out += T.track_sort(predictions, segment_id, camera_id, p['iou_threshold'], p['max_age'], p['min_hits'])
    assert _rows(out) == _rows(exp['tracks'])


def test_sort_update_calls_golden(golden_dir):
    from waymo_2d_tracking_amd.tracking.sort.sort import Sort, KalmanBoxTracker
    KalmanBoxTracker.count = 0
    z = np.load(os.path.join(golden_dir, 'sort_update_calls.npz'))
    s = Sort(max_age=2, min_hits=1)
    for i in range(len(z['in_off']) - 1):
        dets = z['dets'][z['in_off'][i]:z['in_off'][i + 1]]
        exp = z['rows'][z['out_off'][i]:z['out_off'][i + 1]]
        got = s.update(dets if len(dets) else np.array([], dtype=np.float32), 0.2)
        assert got.shape == exp.shape
        assert np.array_equal(got[:, 4], exp[:, 4])
        np.testing.assert_allclose(got, exp, rtol=0, atol=BOX_TOL)


def test_nonfinite_predicted_boxes_golden(golden_dir):
    """Reference-run G9: float32 area overflow -> predicted box [inf, NaN, ..] -> the track is dropped at the next predict
    (sort.py:258-265), the other tracks and the id sequence are unaffected.  HIP drops on any non-finite coordinate, the
    reference on NaN: indistinguishable on reachable states (oracle/gen_golden_sort_nonfinite.py docstring)."""
    from waymo_2d_tracking_amd.tracking.sort.sort import Sort, KalmanBoxTracker
    KalmanBoxTracker.count = 0
    z = np.load(os.path.join(golden_dir, 'sort_g9_nonfinite.npz'))
    s = Sort(max_age=2, min_hits=0)
    for i in range(len(z['in_off']) - 1):
        dets = z['dets'][z['in_off'][i]:z['in_off'][i + 1]]
        exp = z['rows'][z['out_off'][i]:z['out_off'][i + 1]]
        got = s.update(dets if len(dets) else np.array([], dtype=np.float32), 0.1)
        assert got.shape == exp.shape, i
        assert np.array_equal(got[:, 4], exp[:, 4]), i
        assert np.array_equal(np.isfinite(got), np.isfinite(exp)), i
        np.testing.assert_allclose(got, exp, rtol=0, atol=BOX_TOL)
        ids = s.state()[0]
        assert sorted(int(v) for v in ids) == sorted(z['live_ids'][z['live_off'][i]:z['live_off'][i + 1]].tolist()), i


def test_multiclass_tracker_traces_golden(golden_dir):
    """MultiClassTrackerSort.track frame by frame; Kalman x / P of every live track vs the reference trace."""
    from waymo_2d_tracking_amd.tracking.sort.sort import KalmanBoxTracker
    from waymo_2d_tracking_amd.tracking.sort.tracker_sort import MultiClassTrackerSort
    exp = json.load(open(os.path.join(golden_dir, 'sort_g4_expected_a.json')))
    p = exp['params']
    tr = np.load(os.path.join(golden_dir, 'sort_g4_trace.npz'))
    predictions = T.read_data_file(os.path.join(golden_dir, 'sort_g4_input.json'), p['score_threshold'])
    KalmanBoxTracker.count = 0
    so = tr['a_state_off']
    call = 0
    seg = next(iter(predictions))
    cam = next(iter(predictions[seg]))
    tracker = MultiClassTrackerSort(p['max_age'], p['min_hits'])
    for frame_id in sorted(predictions[seg][cam]):
        dets = [[e['bbox'][0], e['bbox'][1], e['bbox'][0] + e['bbox'][2], e['bbox'][1] + e['bbox'][3], e['score'],
                 e['category_id']] for e in predictions[seg][cam][frame_id]]
        tracker.track(dets, p['iou_threshold'])
        for c in tracker.trackers:
            ids, x, P = tracker.trackers[c].state()
            assert np.array_equal(ids, tr['a_ids'][so[call]:so[call + 1]]), (frame_id, c)
            np.testing.assert_allclose(x, tr['a_x'][so[call]:so[call + 1]], rtol=1e-9, atol=1e-7)
            np.testing.assert_allclose(P, tr['a_P'][so[call]:so[call + 1]], rtol=1e-9, atol=1e-7)
            call += 1
    assert call > 100


def test_linear_assignment_vs_oracle(oracle):
    from waymo_2d_tracking_amd.tracking.sort.sort import linear_assignment
    rng = np.random.default_rng(11)
    for trial in range(120):
        n, m = rng.integers(1, 40, 2)
        if trial % 10 == 0:
            n, m = int(rng.integers(90, 130)), int(rng.integers(90, 130))     # beyond the LDS cost budget
        cost = -np.round(rng.uniform(0, 1, (n, m)), 2).astype(np.float32)
        cost[rng.uniform(size=(n, m)) < [0.0, 0.5, 0.9][trial % 3]] = 0
        assert np.array_equal(linear_assignment(cost), oracle.linear_assignment(cost)), (n, m)
    for n, m in ((90, 300), (300, 90), (100, 384), (128, 383), (60, 250), (129, 200), (100, 385), (100, 400)):      # wide register variants + LDS fallback
        cost = -np.round(rng.uniform(0, 1, (n, m)), 2).astype(np.float32)
        cost[rng.uniform(size=(n, m)) < 0.9] = 0
        assert np.array_equal(linear_assignment(cost), oracle.linear_assignment(cost)), (n, m)
    for shape in ((3, 5), (5, 3), (1, 1), (70, 65)):
        z = np.zeros(shape, np.float32)
        assert np.array_equal(linear_assignment(z), [[i, i] for i in range(min(shape))])


def test_associate_vs_oracle(oracle):
    from waymo_2d_tracking_amd.tracking.sort.sort import associate_detections_to_trackers
    rng = np.random.default_rng(12)
    for trial in range(60):
        n, t = int(rng.integers(0, 50)), int(rng.integers(0, 50))
        base = rng.uniform(0, 1000, (max(n, t), 2))
        wh = rng.uniform(20, 200, (max(n, t), 2))
        dets = np.concatenate([base[:n] + rng.normal(0, 8, (n, 2)), base[:n] + wh[:n], rng.uniform(size=(n, 1))], axis=1)
        trks = np.concatenate([base[:t], base[:t] + wh[:t] + rng.normal(0, 8, (t, 2))], axis=1)[rng.permutation(t)]
        thr = [0.0, 0.01, 0.3, 0.7][trial % 4]
        m, ud, ut = associate_detections_to_trackers(dets.astype(np.float32), trks, thr)
        em, eud, eut = oracle.associate(dets.astype(np.float32), trks, thr)
        assert np.array_equal(m, em) and np.array_equal(ud, eud) and np.array_equal(ut, eut), (trial, n, t)


@pytest.mark.parametrize('seed,n_objects,integer', [(1, 100, True), (2, 40, False), (3, 250, True)])
def test_synthetic_streams_vs_oracle(oracle, seed, n_objects, integer):
    """Waymo-shaped streams: 2 segments x 5 cameras; IDs, order and boxes identical to the oracle."""
    from waymo_2d_tracking_amd import synthetic as syn
    dets = syn.make_sequence_json(seed, n_segments=2, n_frames=40, n_objects=n_objects, integer_boxes=integer)
    packed = T.pack_streams(predictions_of(dets))
    sthr, ithr = [0.3, 0.2, 1.0, 0.1], [0.01, 0.01, 1.0, 0.0]
    out, births = T.track_packed(packed, ithr, 2, 0, sthr)
    ref = oracle.track_streams(packed, 2, 0, sthr, ithr)
    assert births == ref['n_births']
    assert np.array_equal(out['object_id'], ref['object_id'])
    assert np.array_equal(out['frame'], ref['frame'])
    assert np.array_equal(out['category'], ref['category'])
    assert np.array_equal(out['bbox'], ref['bbox'])
    np.testing.assert_allclose(out['score'], ref['score'], rtol=4e-16, atol=0)


def test_full_size_properties():
    """Config 1 at full size (198 frames x 5 cameras, ~100 boxes/frame): invariants that need no oracle."""
    from waymo_2d_tracking_amd import synthetic as syn
    dets = syn.make_sequence_json(0, n_segments=1, n_frames=198, n_objects=100)
    packed = T.pack_streams(predictions_of(dets))
    ithr = [0.01, 0.01, 1.0, 0.0]
    out, births = T.track_packed(packed, ithr, 2, 0, [0.0] * 4)
    out2, births2 = T.track_packed(packed, ithr, 2, 0, [0.0] * 4)
    assert births == births2 and all(np.array_equal(out[k], out2[k]) for k in out)      # deterministic
    assert out['object_id'].min() >= 1 and out['object_id'].max() <= births
    assert len(np.unique(out['object_id'])) == births or births >= len(np.unique(out['object_id']))
    assert np.all(np.diff(out['frame']) >= 0)                                            # stream/frame order
    key = out['frame'] * (births + 1) + out['object_id']
    assert len(np.unique(key)) == len(key)                                               # an id appears once per frame
    assert np.all(out['bbox'][:, 2] >= 1) and np.all(out['bbox'][:, 3] >= 1)             # utils.py:45
    assert np.all((out['score'] >= 0.2) & (out['score'] <= 1.0))                         # utils.py:49
    assert len(out['frame']) <= packed['x'].size                                         # one row per matched det at most


def test_edge_cases_empty_and_single(oracle):
    """Empty / ragged inputs: streams whose frames are all empty, a single frame, everything filtered by the score
    threshold, an empty tracker call - same outputs as the oracle, no crash."""
    from waymo_2d_tracking_amd.tracking.sort.sort import Sort, KalmanBoxTracker
    # (1) frames exist but carry no detection at all
    predictions = {'segA': {'FRONT': {100: [], 200: [], 300: []}, 'SIDE_LEFT': {100: []}}}
    packed = T.pack_streams(predictions)
    out, births = T.track_packed(packed, [0.01, 0.01, 1.0, 0.0], 2, 0, [0.0] * 4)
    assert births == 0 and len(out['frame']) == 0
    # (2) one frame, one detection; (3) all detections below the threshold
    one = {'s': {'FRONT': {7: [{'bbox': [10, 20, 30, 40], 'score': 0.9, 'category_id': 2}]}}}
    packed = T.pack_streams(one)
    out, births = T.track_packed(packed, [0.01, 0.01, 1.0, 0.0], 2, 0, [0.0] * 4)
    ref = oracle.track_streams(packed, 2, 0, [0.0] * 4, [0.01, 0.01, 1.0, 0.0])
    assert births == 1 and np.array_equal(out['bbox'], ref['bbox']) and out['object_id'].tolist() == [1]
    out, births = T.track_packed(packed, [0.01, 0.01, 1.0, 0.0], 2, 0, [0.95] * 4)
    assert births == 0 and len(out['frame']) == 0
    # (4) Sort.update with empty detections on a fresh and on a populated tracker
    KalmanBoxTracker.count = 0
    s = Sort(max_age=1, min_hits=0)
    assert s.update(np.array([], dtype=np.float32), 0.3).shape == (0, 6)
    r = s.update(np.array([[0, 0, 10, 10, 1.0], [50, 50, 80, 90, 0.5]], dtype=np.float32), 0.3)
    assert r.shape == (2, 6) and sorted(r[:, 4].tolist()) == [1.0, 2.0]
    assert s.update(np.array([], dtype=np.float32), 0.3).shape == (0, 6)
    assert s.update(np.array([], dtype=np.float32), 0.3).shape == (0, 6)          # tracks reaped (max_age 1)
    ids, _, _ = s.state()
    assert len(ids) == 0


def test_large_frames_use_the_global_cost_path(oracle):
    """Frames with several hundred boxes of one class: the N x T cost matrix exceeds the LDS budget (global scratch),
    the zero bitmaps need > 1 word per row, the per-object Sort grows its device state - still identical to the oracle."""
    from waymo_2d_tracking_amd import synthetic as syn
    rng = np.random.default_rng(9)
    d = syn.stream_detections(rng, 12, 420, 'FRONT', clutter=0.05)
    d['cat'][:] = 1                                     # one class: N ~ 400 per frame, T up to ~ 3 N
    dets = syn.detections_json([('seg', 'FRONT', d)])
    packed = T.pack_streams(predictions_of(dets))
    ithr, sthr = [0.05, 0.01, 1.0, 0.0], [0.0] * 4
    out, births = T.track_packed(packed, ithr, 2, 0, sthr)
    ref = oracle.track_streams(packed, 2, 0, sthr, ithr)
    assert births == ref['n_births']
    assert np.array_equal(out['object_id'], ref['object_id']) and np.array_equal(out['bbox'], ref['bbox'])
    # the per-object API on the same data (device state grows past its initial 256 slots)
    from waymo_2d_tracking_amd.tracking.sort.sort import Sort, KalmanBoxTracker
    KalmanBoxTracker.count = 0
    s = Sort(max_age=2, min_hits=0)
    o = oracle.Sort(2, 0)
    for f in range(4):
        sel = d['frame'] == f
        arr = np.stack([d['x'][sel], d['y'][sel], d['x'][sel] + d['w'][sel], d['y'][sel] + d['h'][sel], d['score'][sel]], 1).astype(np.float32)
        a, b = s.update(arr, 0.05), o.update(arr, 0.05)
        assert a.shape == b.shape and np.array_equal(a[:, :5], b[:, :5])


def test_mct_c_abi_order_and_errors():
    """wt_mct_* (tracker_sort.py:22-51): classes come back in first-seen order, known classes are updated every frame
    even without detections, rows equal independent per-class Sorts sharing one ID counter, and a class without an
    iou threshold is an error (IndexError in the reference)."""
    import ctypes as C
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking.sort.sort import KalmanBoxTracker, Sort
    from waymo_2d_tracking_amd.tracking.sort.tracker_sort import MultiClassTrackerSort
    rng = np.random.default_rng(3)
    thr = [0.01, 0.01, 1.0, 0.0]

    def frame(n):
        xy = rng.uniform(0, 1500, (n, 2)); wh = rng.uniform(20, 200, (n, 2))
        return np.concatenate((xy, xy + wh, rng.uniform(0.1, 1, (n, 1)), rng.choice([4, 2, 1], (n, 1))), 1)

    frames = [frame(12), frame(0), frame(7), frame(15)]
    frames[0][:, 5] = [4] * 5 + [2] * 4 + [1] * 3                       # first-seen order 4, 2, 1
    KalmanBoxTracker.count = 0
    mct = MultiClassTrackerSort(max_age=2, min_hits=0)
    got = [mct.track(f.tolist(), thr) for f in frames]
    assert list(mct.trackers) == [4, 2, 1] and all(list(g) == [4, 2, 1] for g in got)
    n_ids = KalmanBoxTracker.count
    KalmanBoxTracker.count = 0
    sorts = {c: Sort(2, 0) for c in (4, 2, 1)}
    for f, g in zip(frames, got):
        for c in (4, 2, 1):
            want = sorts[c].update(np.asarray([r[:5] for r in f.tolist() if r[5] == c], dtype=np.float32), thr[c - 1])
            assert np.array_equal(g[c], want)
    assert KalmanBoxTracker.count == n_ids > 0
    bad = frame(3); bad[:, 5] = 7
    with pytest.raises(RuntimeError):
        mct.track(bad.tolist(), thr)
    assert _lib.lib().wt_mct_tracker(mct._h, C.c_int(3)) is None


@pytest.mark.parametrize('n_segments', [1, 14])
def test_helper_waves_and_plain_kernel_both_equal_the_oracle(oracle, n_segments):
    """Round 4: with at most 256 trackers the persistent SORT kernel runs with three helper waves per tracker (IoU matrix, Munkres steps
    1 / 6 split over four waves: sort_streams_kernel<true, false>); beyond that the plain single-wave instantiation runs.  1 segment = 5 streams x
    4 classes = 20 trackers (helpers), 14 segments = 280 trackers (plain): rows, ids, births and boxes identical to the oracle in both."""
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.tracking import utils as T
    dets = syn.make_sequence_json(21, n_segments=n_segments, n_frames=12, n_objects=45)
    packed = T.pack_streams(predictions_of(dets))
    assert len(packed['stream_frame_offsets']) - 1 == 5 * n_segments
    sthr, ithr = [0.0, 0.0, 0.0, 0.0], [0.01, 0.01, 0.3, 0.0]
    out, births = T.track_packed(packed, ithr, 2, 0, sthr)
    ref = oracle.track_streams(packed, 2, 0, sthr, ithr)
    assert births == ref['n_births'] and len(out['frame']) == len(ref['frame']) > 0
    assert np.array_equal(out['object_id'], ref['object_id']) and np.array_equal(out['frame'], ref['frame'])
    assert np.array_equal(out['bbox'], ref['bbox'])
