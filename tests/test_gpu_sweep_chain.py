"""The tracking sweep with the rows resident in HBM (tracking/chain.py, evaluate.sweep(device_chain=True))
equals the host route - settings, count tables, the bits of iou_sum, ignored rows, ranked, best - on one segment with two cameras,
with and without the second association, with and without refinement; what the chain does not carry is refused by name; one
setting is tied to the restatements (tests/refine_ref.py, tests/mot_ref.py)."""
import json

import numpy as np
import pytest

import mot_ref
import refine_cases
import track_stage_support as H

pytestmark = pytest.mark.gpu

GRID = {'score': [0.3, 0.6], 'iou': [0.01], 'max_age': [1, 3], 'min_hits': [0], 'gap': [0, 1, 2], 'min_len': [1, 2]}
SECOND = dict(GRID, low_score=[0.2])


@pytest.fixture(scope='module')
def sweep_set(tmp_path_factory):
    return H.sweep_set(tmp_path_factory, 'chain_sweep')


@pytest.fixture(scope='module')
def both_routes(sweep_set):
    """(host route, chain) of GRID and of SECOND, each swept once"""
    from waymo_2d_tracking_amd.tracking import evaluate as E
    path, _, gt_json = sweep_set
    gt = E.load_ground_truth(gt_json)
    return dict((name, (E.sweep(path, gt, grid), E.sweep(path, gt, grid, device_chain=True))) for name, grid in (('plain', GRID), ('second', SECOND)))


def assert_same_sweep(host, chain):
    assert host['settings'] == chain['settings']
    assert len(host['results']) == len(chain['results']) == len(host['settings'])
    for k, (a, b) in enumerate(zip(host['results'], chain['results'])):
        assert a.counts.dtype == b.counts.dtype and a.counts.tolist() == b.counts.tolist(), ('counts', k)
        assert H.same_bits(b.iou_sum, a.iou_sum), ('iou_sum', k)
        assert a.ignored_rows == b.ignored_rows, ('ignored_rows', k)
    for key in ('ranked', 'best'):
        assert json.dumps(host[key], sort_keys=True) == json.dumps(chain[key], sort_keys=True), key
    assert sorted(host) == sorted(chain)


@pytest.mark.parametrize('name', ['plain', 'second'])
def test_chain_equals_the_host_route(both_routes, name):
    host, chain = both_routes[name]
    assert len(host['settings']) == 24 and ('low_score' in host['settings'][0]) == (name == 'second')
    assert sum(int(r.counts[..., 1].sum()) for r in host['results']) > 0                  # something is matched: the tables are not empty
    assert len(set(json.dumps(r.counts.tolist()) for r in host['results'])) > 6            # and the settings differ
    assert_same_sweep(host, chain)


def test_without_refinement_the_layout_goes_straight_to_the_metric_order(sweep_set, monkeypatch):
    from waymo_2d_tracking_amd.tracking import evaluate as E, refine
    path, _, gt_json = sweep_set
    gt = E.load_ground_truth(gt_json)
    grid = dict((k, GRID[k]) for k in ('score', 'iou', 'max_age', 'min_hits'))
    host = E.sweep(path, gt, grid)

    def no_refinement(*args, **kw):
        raise AssertionError('the refinement is off: DeviceRefine must not be built')
    monkeypatch.setattr(refine, 'DeviceRefine', no_refinement)
    assert_same_sweep(host, E.sweep(path, gt, grid, device_chain=True))
    assert sorted(host['settings'][0]) == ['iou', 'max_age', 'min_hits', 'score']


def test_what_the_chain_does_not_carry_is_refused_by_name(sweep_set):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    path, _, gt_json = sweep_set
    gt = E.load_ground_truth(gt_json)
    with pytest.raises(ValueError, match='stitch.*--link-gap-grid'):
        E.sweep(path, gt, dict(GRID, link_gap=[0, 2]), device_chain=True)
    with pytest.raises(ValueError, match='identity'):
        E.sweep(path, gt, GRID, identity=True, device_chain=True)
    with pytest.raises(ValueError, match='hota'):
        E.sweep(path, gt, GRID, rank_by='hota', device_chain=True)
    with pytest.raises(ValueError, match='smooth.*coverage'):
        E.sweep(path, gt, dict(GRID, smooth_window=[0, 1]), coverage=True, device_chain=True)


def test_a_ground_truth_without_one_camera_gives_equal_tables(sweep_set):
    """the rows of the camera the ground truth lacks are the ignored ones, on both routes"""
    from waymo_2d_tracking_amd.tracking import evaluate as E
    path, _, gt_json = sweep_set
    front = {'images': [im for im in gt_json['images'] if im['id'].endswith('/FRONT')],
             'annotations': [a for a in gt_json['annotations'] if a['image_id'].endswith('/FRONT')]}
    assert 0 < len(front['images']) < len(gt_json['images'])
    gt = E.load_ground_truth(front)
    host, chain = E.sweep(path, gt, GRID), E.sweep(path, gt, GRID, device_chain=True)
    assert_same_sweep(host, chain)
    assert all(r.ignored_rows > 0 for r in chain['results'])


def test_one_point_per_round_gives_the_same_tables(sweep_set, both_routes):
    """a workspace limit of one byte: every tracked point is a round of its own"""
    from waymo_2d_tracking_amd.tracking import chain as CH, evaluate as E, utils as T
    path, _, gt_json = sweep_set
    host, _ = both_routes['plain']
    _, plans = E.sweep_settings(GRID)
    chain = CH.DeviceChain(T.pack_streams(E._detections(path)), E.load_ground_truth(gt_json), 4, E.DEFAULT_IOU_THRESHOLD, workspace_limit_bytes=1)
    results = chain.run([args for _, args in E._tracked_points(GRID, plans['second'])], plans['refine'].jobs)
    assert chain.rounds == 4 and len(results) == 24
    for k, (a, b) in enumerate(zip(host['results'], results)):
        assert a.counts.tolist() == b.counts.tolist() and H.same_bits(b.iou_sum, a.iou_sum) and a.ignored_rows == b.ignored_rows, k


def test_one_group_of_settings_equals_the_restatements(sweep_set, both_routes):
    """ties the chain to tests/refine_ref.py and tests/mot_ref.py, not only to the host route"""
    from waymo_2d_tracking_amd.tracking import evaluate as E
    _, dets, gt_json = sweep_set
    _, chain = both_routes['plain']
    of_setting = H.sweep_reference(dets, gt_json, lambda s: {'refine': refine_cases.job(max_gap=s['interp_gap'], min_len=s['min_len'])}, metrics=('mot',))
    for k in (18, 23):                                                                     # max_age 3, score 0.6: no refinement; gap 2 and min_len 2
        s = chain['settings'][k]
        assert (s['max_age'], s['score'], s['interp_gap'], s['min_len']) == ((3, 0.6, 0, 1) if k == 18 else (3, 0.6, 2, 2))
        table = of_setting(s)[0]
        for c in E.ALL_CLASSES:
            for lv in (1, 2):
                assert [chain['results'][k].table[c][lv][f] for f in mot_ref.FIELDS] == [table[c][lv][f] for f in mot_ref.FIELDS], (k, c, lv)
