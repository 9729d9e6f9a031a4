"""The two track layout steps on the GPU (csrc/tracks_layout.hip) against the host code they are twins of:
wt_tracks_layout_* equals _trackset.prepare field by field, wt_tracks_to_eval_* equals evaluate.pack_results - integers equal,
float columns the same bits - on the cases of tests/layout_cases.py, through the host form and the device form, and on the
tracked fixtures; DeviceRefine on a DeviceTrackSet gives the reference's rows."""
import numpy as np
import pytest

import layout_cases as LC
import refine_ref
from track_cases import N_CLASSES
from track_stage_support import G4, G5, STAGES, arrays, packed_for, predictions_of, same_bits, tracked_fixtures

pytestmark = pytest.mark.gpu

INTS = ('category', 'local', 'set_row_offsets', 'frame_row_offsets', 'n_traj', 'traj_offsets')


class Rows(object):
    """a hand-made result in HBM, in buffers of its own as DeviceTracker leaves one (capacity = rows + 1)"""

    def __init__(self, res, count=None):
        import torch
        a = arrays(res)
        n = len(a['frame'])
        up = lambda v, dtype, tail=(): torch.from_numpy(np.concatenate([np.asarray(v, dtype).reshape((n,) + tail), np.zeros((1,) + tail, dtype)])).cuda()
        self.out_frame, self.out_category = up(a['frame'], np.int64), up(a['category'], np.int32)
        self.out_bbox, self.out_score, self.out_id = up(a['bbox'], np.float64, (4,)), up(a['score'], np.float64), up(a['object_id'], np.int64)
        self.counts = torch.tensor([n if count is None else count, 0], dtype=torch.int64).cuda()


def assert_equals_prepare(got, p, results):
    for name in ('x', 'y', 'w', 'h', 'score'):
        assert same_bits(got[name], p[name]), name
    for name in INTS:
        assert got[name].dtype == p[name].dtype and got[name].tolist() == p[name].tolist(), name
    assert (got['n_rows'], got['n_traj_total'], got['max_traj']) == (p['n_rows'], p['n_traj_total'], p['max_traj']), 'totals'
    S = p['n_streams']
    want = np.zeros(p['n_traj_total'], np.int64)                           # per trajectory the id of its first row
    for r, res in enumerate(results):
        lo = int(p['set_row_offsets'][r])
        frame, oid = np.asarray(res['frame'], np.int64), np.asarray(res['object_id'], np.int64)
        stream = np.searchsorted(p['stream_frame_offsets'], frame, side='right') - 1
        for i in reversed(range(frame.size)):
            want[int(p['traj_offsets'][r * S + stream[i]]) + int(p['local'][lo + i])] = oid[i]
    assert got['traj_object_id'].tolist() == want.tolist(), 'traj_object_id'


def check_layout(case):
    """host form and device form equal prepare(); a second launch on the same buffers repeats the answer"""
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    offsets, results, claim = case
    packed, outs = packed_for(offsets), [arrays(r) for r in results]
    p = TS.prepare(packed, outs, [], N_CLASSES, 'layout')
    claim(p)
    assert_equals_prepare(TS.layout_tracks_host(packed, outs, N_CLASSES), p, results)
    dev = TS.DeviceTrackSet(packed, [Rows(r) for r in results], N_CLASSES)
    dev.launch()
    first = dev.fetch()
    assert_equals_prepare(first, p, results)
    dev.launch()
    again = dev.fetch()
    for name in first:
        assert np.asarray(first[name]).tobytes() == np.asarray(again[name]).tobytes(), (name, 'differs after a second launch')
    return dev


@pytest.mark.parametrize('name', sorted(LC.LAYOUT_CASES))
def test_layout_case_equals_prepare(name):
    check_layout(LC.LAYOUT_CASES[name]())


def test_colliding_ids_in_every_order_of_first_appearance():
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    check_layout(LC.colliding_ids(TS.layout_probe, TS.layout_limits()[1]))


@pytest.mark.parametrize('above', [0, 1])
def test_rows_on_either_side_of_the_lds_limit(above):
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    check_layout(LC.many_rows(TS.layout_limits()[0] + above))


def test_scan_seams():
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    for n in LC.SEAMS + (TS.layout_limits()[2] + 1,):
        check_layout(LC.scan_seam(n))


def test_workspace_one_byte_short_is_refused_before_any_launch():
    import torch
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    offsets, results, _ = LC.same_id_elsewhere()
    rows = [Rows(r) for r in results]
    good = TS.DeviceTrackSet(packed_for(offsets), rows, N_CLASSES)
    small = TS.DeviceTrackSet(packed_for(offsets), rows, N_CLASSES, workspace_bytes=good.ws_bytes - 1)
    small.t['totals'].fill_(-7)
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY'):
        small.launch()
    torch.cuda.synchronize()
    assert small.t['totals'].tolist() == [-7, -7, -7]


@pytest.mark.parametrize('name', sorted(LC.REFUSALS))
def test_refusals_are_reported(name):
    import torch
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    offsets, results, counts, status = LC.REFUSALS[name]()
    dev = TS.DeviceTrackSet(packed_for(offsets), [Rows(r, c) for r, c in zip(results, counts)], N_CLASSES)
    dev.launch()
    with pytest.raises(_lib.WaymoTrackError, match=status):
        dev.wait()
    torch.cuda.synchronize()
    if min(counts) >= 0:                                                    # the host form names the result and the row
        with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_INVALID.*result 0, row'):
            TS.layout_tracks_host(packed_for(offsets), [arrays(r) for r in results], N_CLASSES)


def test_more_rows_than_the_buffers_hold_is_capacity():
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    offsets, results, _ = LC.second_row_is_last()
    dev = TS.DeviceTrackSet(packed_for(offsets), [Rows(results[0], count=len(results[0]['frame']) + 2)], N_CLASSES)
    dev.launch()
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY'):
        dev.wait()


# ---- wt_tracks_to_eval_* ----

def layout_of(offsets, results):
    """the shared layout of hand-made results without prepare()'s category check"""
    n_frames = offsets[-1]
    local = [LC.first_appearance(offsets, r)[0] for r in results]
    return dict(set_row_offsets=np.concatenate([[0], np.cumsum([len(r['frame']) for r in results])]).astype(np.int64),
                frame_row_offsets=np.stack([np.searchsorted(np.asarray(r['frame'], np.int64), np.arange(n_frames + 1)) for r in results]).astype(np.int64),
                category=np.concatenate([np.asarray(r['category'], np.int32) for r in results] + [np.zeros(0, np.int32)]),
                local=np.concatenate([np.asarray(v, np.int32) for v in local] + [np.zeros(0, np.int32)]),
                bbox=np.concatenate([np.asarray(r['bbox'], np.float64).reshape(-1, 4) for r in results]))


def assert_equals_pack_results(got, want, stream_of_row):
    for name in ('x', 'y', 'w', 'h'):
        assert same_bits(got[name], want[name]), name
    for name in ('category', 'set_row_offsets', 'frame_hyp_offsets'):
        assert got[name].dtype == want[name].dtype and got[name].tolist() == want[name].tolist(), name
    assert [o.tolist() for o in got['orders']] == [o.tolist() for o in want['orders']], 'orders'
    for k, order in enumerate(want['orders']):                              # h_id: the same equality classes per (result, stream)
        lo, hi = int(want['set_row_offsets'][k]), int(want['set_row_offsets'][k + 1])
        assert (got['h_id'][lo:hi] >= 0).all(), 'h_id'
        assert first_row_of_class(stream_of_row[k][order], got['h_id'][lo:hi]).tolist() == first_row_of_class(stream_of_row[k][order], want['h_id'][lo:hi]).tolist(), ('h_id', k)


def first_row_of_class(stream, ids):
    """per row the first row with its (stream, id): equal for two id columns <=> they have the same equality classes per stream"""
    if len(ids) == 0:
        return np.zeros(0, np.int64)
    key = np.asarray(stream, np.int64) * (int(np.max(ids)) + 1) + np.asarray(ids, np.int64)
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    return first[inverse]


def eval_reference(offsets, results, gt_json):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    gt, packed = E.load_ground_truth(gt_json), packed_for(offsets)
    want = E.pack_results(gt, [E.tracks_from_packed(packed, arrays(r)) for r in results], N_CLASSES)
    streams = [np.searchsorted(np.asarray(offsets), np.asarray(r['frame'], np.int64), side='right') - 1 for r in results]
    return gt, packed, want, streams


@pytest.mark.parametrize('name', sorted(LC.EVAL_CASES))
def test_eval_case_equals_pack_results(name):
    import torch
    from waymo_2d_tracking_amd.tracking import chain, evaluate as E
    offsets, results, gt_json, claim = LC.EVAL_CASES[name]()
    gt, packed, want, streams = eval_reference(offsets, results, gt_json)
    claim([E._align(gt, E.tracks_from_packed(packed, arrays(r)), N_CLASSES) for r in results])
    lay, smap, G = layout_of(offsets, results), chain.slot_map(packed, gt), int(gt['frame_ids'].size)
    columns = [np.ascontiguousarray(lay['bbox'][:, i]) for i in range(4)]
    side = E.max_frame_boxes({'frame_ids': gt['frame_ids'], 'category': np.zeros(0, np.int32), 'frame_gt_offsets': np.zeros(G + 1, np.int64)}, want, N_CLASSES)
    for got in (chain.to_eval_host(lay, columns, smap, G, N_CLASSES), chain.to_eval_host(lay, lay['bbox'], smap, G, N_CLASSES, box_stride=4)):
        assert_equals_pack_results(got, want, streams)
        assert got['max_frame_boxes'] == side, 'max_frame_boxes'


def test_to_eval_refuses_a_map_that_names_a_slot_twice():
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import chain
    offsets, results, gt_json, _ = LC.unknown_slots()
    lay = layout_of(offsets, results)
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_INVALID.*named by the frame slots 1 and 2'):
        chain.to_eval_host(lay, lay['bbox'], np.asarray([-1, 0, 0, -1, 2, -1], np.int64), 3, N_CLASSES, box_stride=4)


# ---- the tracked fixtures: two DeviceTracker runs -> DeviceTrackSet -> DeviceRefine / DeviceToEval ----

def two_runs(packed, iou, settings):
    """`packed` tracked on the GPU once per (max_age, score thresholds): (packed, the trackers after run(), their fetched results)"""
    from waymo_2d_tracking_amd import devpath
    trackers = [devpath.DeviceTracker(packed, iou, age, 0, score) for age, score in settings]
    for t in trackers:
        t.run()
    return packed, trackers, [t.results()[0] for t in trackers]


@pytest.fixture(scope='module')
def tracked():
    """synthetic detections of one segment and two cameras, tracked with max_age 3 from score 0.3 and with max_age 1 from 0.6"""
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.tracking import utils as T
    dets, gt_json = syn.make_tracking_json(23, n_segments=1, n_frames=12, n_objects=12, cameras=('FRONT', 'SIDE_LEFT'))
    packed, trackers, outs = two_runs(T.pack_streams(predictions_of(dets)), [0.01] * N_CLASSES, ((3, [0.3] * N_CLASSES), (1, [0.6] * N_CLASSES)))
    assert len(outs[0]['frame']) != len(outs[1]['frame']) and min(len(o['frame']) for o in outs) > 64
    return packed, trackers, outs, gt_json


def test_device_trackset_of_two_trackers_equals_prepare(golden_dir, tracked):
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    sets = [two_runs(packed, cfg['iou'], ((2, None), (1, None))) for (packed, _), cfg in zip(tracked_fixtures(golden_dir), (G4, G5))] + [tracked[:3]]
    for (packed, out), (_, _, outs) in zip(tracked_fixtures(golden_dir), sets):
        for name in out:                                                    # the device tracker's rows are the host form's
            assert out[name].tobytes() == outs[0][name].tobytes(), name
    for packed, trackers, outs in sets:
        p = TS.prepare(packed, outs, [], N_CLASSES, 'layout')
        ts = TS.DeviceTrackSet(packed, trackers, N_CLASSES)
        ts.launch()
        assert_equals_prepare(ts.fetch(), p, outs)


def test_device_refine_on_a_trackset_gives_the_reference_rows(tracked):
    from waymo_2d_tracking_amd.tracking import _trackset as TS, refine
    packed, trackers, outs, _ = tracked
    jobs = [{'max_gap': 2, 'min_len': 2, 'result': 0}, {'max_gap': 1, 'min_len': 3, 'score_mode': 'mean', 'result': 1}, {'result': 1}]
    ts = TS.DeviceTrackSet(packed, trackers, N_CLASSES)
    ts.launch()
    dev = refine.DeviceRefine(packed, ts, jobs, N_CLASSES)
    dev.launch()
    got = dev.results()
    assert len(got) == len(jobs)
    for g, job in zip(got, jobs):
        out = outs[job['result']]
        rows = dict((k, out[k].tolist()) for k in out)
        ref = refine_ref.refine(packed['stream_frame_offsets'].tolist(), rows, refine_cases_job(job))
        STAGES['refine'].assert_same(g, ref, out)


def refine_cases_job(job):
    import refine_cases
    return refine_cases.job(job.get('max_gap', 0), job.get('min_len', 1), job.get('score_mode', 'keep'))


def test_to_eval_dev_on_a_trackset_and_on_refined_rows_equals_pack_results(tracked):
    """the device form on both sources it takes; the ground truth lacks the SIDE_LEFT camera and every third frame of the other"""
    import torch
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import _trackset as TS, chain, evaluate as E, refine
    packed, trackers, outs, gt_json = tracked
    keep = lambda image_id: image_id.endswith('/FRONT') and (int(image_id.split('/')[1]) // 100000) % 3 != 0
    gt = E.load_ground_truth({'images': [im for im in gt_json['images'] if keep(im['id'])],
                              'annotations': [a for a in gt_json['annotations'] if keep(a['image_id'])]})
    smap, G = chain.slot_map(packed, gt), int(gt['frame_ids'].size)
    assert 0 < (smap >= 0).sum() < 12 and smap.size == 24
    ts = TS.DeviceTrackSet(packed, trackers, N_CLASSES)
    ts.launch()
    ts.wait()
    dsmap = torch.from_numpy(smap).cuda()
    jobs = [{'max_gap': 2, 'min_len': 2, 'result': 0}, {'result': 1}]
    ref = refine.DeviceRefine(packed, ts, jobs, N_CLASSES)
    ref.launch()
    refined = ref.results()
    for source, results in ((ts, outs), (ref, refined)):
        order = chain.DeviceToEval(source, dsmap, G, N_CLASSES)
        order.launch()
        order.wait()
        want = E.pack_results(gt, [E.tracks_from_packed(packed, r) for r in results], N_CLASSES)
        n = int(want['set_row_offsets'][-1])
        got = dict((k, order.out[k].cpu().numpy()[:n]) for k in ('x', 'y', 'w', 'h', 'category', 'h_id'))
        got.update(set_row_offsets=order.out['set_row_offsets'].cpu().numpy(), frame_hyp_offsets=order.out['frame_hyp_offsets'].cpu().numpy())
        o = order.out['order'].cpu().numpy()
        got['orders'] = [o[int(want['set_row_offsets'][k]):int(want['set_row_offsets'][k + 1])] for k in range(len(results))]
        streams = [np.searchsorted(packed['stream_frame_offsets'], np.asarray(r['frame'], np.int64), side='right') - 1 for r in results]
        assert_equals_pack_results(got, want, streams)
        side = E.max_frame_boxes({'frame_ids': gt['frame_ids'], 'category': np.zeros(0, np.int32), 'frame_gt_offsets': np.zeros(G + 1, np.int64)}, want, N_CLASSES)
        assert order.max_frame_boxes == side, 'max_frame_boxes'
        small = chain.DeviceToEval(source, dsmap, G, N_CLASSES, workspace_bytes=order.ws_bytes - 1)
        with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY'):
            small.launch()
