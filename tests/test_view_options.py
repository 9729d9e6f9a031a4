"""CPU checks of the multi-view options: view specs, weight normalisation and the slot-ensemble workspace query."""
import ctypes as C

import pytest

from waymo_2d_tracking_amd.detnet.ensemble import normalise_weights as normalise_view_weights
from waymo_2d_tracking_amd.detnet.nn.tta import parse_view


def test_view_specs_fold_into_scale_and_flip():
    assert parse_view('orig') == (1.0, False)
    assert parse_view('') == (1.0, False)
    assert parse_view('x1.5,hflip') == (1.5, True)
    assert parse_view('x1.2') == (1.2, False)
    for bad in ('brute', 'dflip', 'x1.5,vflip'):
        with pytest.raises(ValueError):
            parse_view(bad)


def test_view_weights_are_normalised_by_their_maximum():
    assert normalise_view_weights(None, 3) == [1.0, 1.0, 1.0]
    assert normalise_view_weights([2, 1], 2) == [1.0, 0.5]
    assert normalise_view_weights([1, 0.8], 2) == [1.0, 0.8]
    with pytest.raises(ValueError):
        normalise_view_weights([1.0], 2)
    with pytest.raises(ValueError):
        normalise_view_weights([0.0, 0.0], 2)


def test_pipeline_rejects_views_together_with_tta():
    from waymo_2d_tracking_amd.bench_e2e import DetectTrackPipeline
    with pytest.raises(ValueError, match='exclusive'):
        DetectTrackPipeline(tta='x1.5', views=('orig', 'x1.5'), device='cpu')
    with pytest.raises(ValueError):
        DetectTrackPipeline(views=('orig', 'brute'), device='cpu')


def test_slot_ensemble_workspace_query():
    from waymo_2d_tracking_amd import _lib
    lib = _lib.lib()
    ws = lambda *a: int(lib.wt_ensemble_slots_workspace(C.c_int64(a[0]), C.c_int64(a[1]), C.c_int(a[2]), C.c_int(a[3]), C.c_int(a[4])))
    assert ws(10, 100, 2, 4, 2) >= 2 * 10 * 4 * 200 * 5 * 8          # gathered + merged rows of every (frame, category) group
    assert ws(10, 100, 8, 4, 0) > ws(10, 100, 8, 4, 2)               # 8-view fusion groups take the global scratch path
    assert ws(10, 100, 0, 4, 2) == 0 and ws(10, 100, 2, 4, 3) == 0 and ws(10, 100, 2, 0, 1) == 0
