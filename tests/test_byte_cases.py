"""Every input of tests/byte_cases.py reaches the path it is named for: proved on the CPU from the counters the reference
returns (second associations run, their matches, rejected pairs, transposed passes, ...).  No GPU."""
import numpy as np
import pytest

import byte_cases as BC
import byte_ref


def _run(c):
    return byte_ref.track_streams(c['packed'], c['max_age'], c['min_hits'], c['score'], c['iou'], c['low_score'], c['low_iou'])


def _reaches(c, ref):
    for name, least in c['reach'].items():
        assert ref['stats'][name] >= least, (name, ref['stats'])


@pytest.mark.parametrize('name', sorted(BC.PATHS))
def test_path_cases_reach_their_path(name):
    c = BC.PATHS[name]()
    assert c['reach']
    _reaches(c, _run(c))


@pytest.mark.parametrize('n_low,n_left', BC.WAVE_EDGES)
def test_wave_edge_cases_reach_their_shape(n_low, n_left):
    c = BC.wave_edges(n_low, n_left)
    p = c['packed']
    assert np.diff(p['frame_det_offsets']).tolist() == [n_left, n_low, n_left]
    assert np.all(p['score'][n_left:n_left + n_low] < BC.HIGH) and np.all(p['score'][n_left:n_left + n_low] >= BC.LOW)
    ref = _run(c)
    _reaches(c, ref)
    assert ref['stats']['second_run'] == 1                       # exactly one second pass: n_low x n_left
    assert ref['stats']['second_match'] + ref['stats']['second_reject'] == min(n_low, n_left)
    assert ref['n_births'] >= n_left


def test_edge_thresholds_sit_on_the_float32_neighbours():
    """The three thresholds of the edge test: the pair's float32 IoU is equal to, the nearest value below, and above them; the
    reference keeps the pair at the first and the third and rejects it at the second."""
    v = byte_ref.low_pair_iou(BC.EDGE_TRACK, BC.EDGE_DET)
    assert 0.5 < float(v) < 0.9
    up, down = np.nextafter(v, np.float32(1)), np.nextafter(v, np.float32(0))
    assert down < v < up
    for thr, kept in ((float(v), 1), (float(up), 0), (float(down), 1)):
        ref = _run(BC.edge(thr))
        assert ref['stats']['second_run'] == 1
        assert (ref['stats']['second_match'], ref['stats']['second_reject']) == (kept, 1 - kept), thr
        assert ref['frame'].tolist() == ([0, 1, 2] if kept else [0, 2]) and ref['object_id'].tolist() == [1] * (2 + kept)
        assert ref['n_births'] == 1


def test_contested_cases_are_exact_ties():
    """Both contested cases offer the assignment two equal costs."""
    a = byte_ref.low_pair_iou((100, 100, 60, 60), (120, 100, 60, 60))
    b = byte_ref.low_pair_iou((140, 100, 60, 60), (120, 100, 60, 60))
    assert a == b and a > np.float32(0.2)
    a = byte_ref.low_pair_iou((120, 100, 60, 60), (100, 100, 60, 60))
    b = byte_ref.low_pair_iou((120, 100, 60, 60), (140, 100, 60, 60))
    assert a == b and a > np.float32(0.2)


def test_off_lds_case_is_on_the_global_cost_path():
    """plan_tracking of sort_engine.hip restated: more than 256 trackers keep the 8192-float LDS cost budget; the second cost matrix
    of the case has n * ld floats with n = 100 rows and ld = 100 | 1."""
    c = BC.off_lds()
    p = c['packed']
    n_trackers = (len(p['stream_frame_offsets']) - 1) * BC.C4
    cap_n = int(np.diff(p['frame_det_offsets']).max())
    cap = cap_n * (c['max_age'] + 2)
    assert n_trackers > 256 and cap_n * (cap | 1) > 8192         # cost_g is allocated
    assert 100 * (100 | 1) > 8192                                  # and the second pass needs it
    ref = _run(c)
    assert ref['stats']['second_run'] == 1 and ref['stats']['second_match'] + ref['stats']['second_reject'] == 100


@pytest.mark.parametrize('max_age,min_hits', BC.AGE_HITS)
def test_random_streams_have_scores_between_and_reach_every_kind_of_second_pass(max_age, min_hits):
    c = BC.random_streams(5, 1, 12, 40, max_age, min_hits, streams=3)
    s = c['packed']['score']
    share = np.mean((s >= 0.3) & (s < 0.6))
    assert 0.2 < share < 0.4
    _reaches(c, _run(c))
