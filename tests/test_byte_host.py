"""What the second association refuses before it touches a device, and the flags of tracking/track.py and tracking/evaluate.py
around it (no GPU)."""
import numpy as np
import pytest

import byte_cases as BC

INVALID = 1


def _modules():
    from waymo_2d_tracking_amd import build
    build.build(verbose=False)
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.tracking import utils
    return _lib, utils


@pytest.mark.parametrize('low_score,low_iou,text', [
    ([0.1, 0.7, 0.1, 0.1], [0.5] * 4, 'class 2: low_score_threshold 0.7 above score_threshold 0.6'),
    ([0.1, 0.1, np.nan, 0.1], [0.5] * 4, 'class 3: a threshold of the second association is NaN'),
    ([0.1] * 4, [0.5, 0.5, 0.5, np.nan], 'class 4: a threshold of the second association is NaN'),
    ([0.1] * 4, [1.5, 0.5, 0.5, 0.5], 'class 1: low_iou_threshold 1.5 outside [0, 1]'),
    ([0.1] * 4, [0.5, -0.01, 0.5, 0.5], 'class 2: low_iou_threshold -0.01 outside [0, 1]'),
])
def test_bad_thresholds_are_invalid_and_name_the_class(low_score, low_iou, text):
    _lib, T = _modules()
    c = BC.dip()
    with pytest.raises(_lib.WaymoTrackError) as e:
        T.track_packed_byte(c['packed'], c['iou'], 1, 0, c['score'], low_score, low_iou)
    assert 'WT_ERR_INVALID' in str(e.value) and text in str(e.value)


def test_workspace_is_zero_for_bad_thresholds_and_grows_by_the_remaining_list():
    import ctypes as C
    _lib, T = _modules()
    lib = _lib.lib()
    params, keep = T.make_params(1, 0, [0.6] * 4, [0.3] * 4)
    low, liou, bad = _lib.as_f64([0.1] * 4), _lib.as_f64([0.5] * 4), _lib.as_f64([0.9] * 4)
    args = (C.c_int64(1000), C.c_int64(50), C.c_int32(5), C.c_int64(40), C.byref(params))
    plain = lib.wt_track_streams_workspace(*args)
    assert lib.wt_track_streams_byte_workspace(*args, _lib.ptr(bad), _lib.ptr(liou)) == 0
    byte = lib.wt_track_streams_byte_workspace(*args, _lib.ptr(low), _lib.ptr(liou))
    cap = 40 * 3
    assert plain > 0 and 5 * 4 * cap * 4 <= byte - plain <= 5 * 4 * cap * 4 + 3 * 256       # cap ints per tracker and two threshold arrays


def test_per_class_lengths():
    _lib, T = _modules()
    assert T.per_class([0.5], 4, 'x') == [0.5] * 4 and T.per_class([1, 2, 3, 4], 4, 'x') == [1, 2, 3, 4]
    with pytest.raises(ValueError):
        T.per_class([0.5, 0.5], 4, 'x')


def test_track_parser_defaults_are_off():
    from waymo_2d_tracking_amd.tracking import track
    args = track.build_parser().parse_args([])
    assert args.low_score_threshold is None and args.low_iou_threshold == [0.5]
    assert not track.second_association(args) and track.read_threshold(args) == args.score_threshold
    args = track.build_parser().parse_args(['--low-score-threshold=0.3,0.2,1.0,0.1', '--low-iou-threshold=0.4'])
    assert track.second_association(args) and track.read_threshold(args) == [0.3, 0.2, 1.0, 0.1] and args.low_iou_threshold == [0.4]


def test_track_refuses_the_flag_under_torchrun(monkeypatch, tmp_path):
    from waymo_2d_tracking_amd.tracking import track
    monkeypatch.setenv('WORLD_SIZE', '2')
    monkeypatch.setenv('RANK', '0')
    with pytest.raises(SystemExit) as e:
        track.main(['--input', str(tmp_path / 'none.json'), '--output', str(tmp_path / 'out.json'), '--low-score-threshold=0.3,0.3,1.0,0.2'])
    assert '--low-score-threshold is not available under torchrun' in str(e.value)


def test_evaluate_parser_defaults_and_flag_line():
    from waymo_2d_tracking_amd.tracking import evaluate
    args = evaluate.build_parser().parse_args(['--annotations', 'gt.json'])
    assert args.low_score_grid == '' and args.low_iou_grid == '0.5'
    plain = {'score_threshold': [0.6] * 4, 'iou_threshold': [0.1] * 4, 'max_age': 1, 'min_hits': 0}
    assert 'low' not in evaluate.flag_line(plain)
    line = evaluate.flag_line(dict(plain, low_score_threshold=[0.3, 0.3, 0.6, 0.3], low_iou_threshold=[0.5] * 4))
    assert line.endswith('--low-score-threshold=0.3,0.3,0.6,0.3 --low-iou-threshold=0.5,0.5,0.5,0.5')
    from waymo_2d_tracking_amd.tracking import track
    parsed = track.build_parser().parse_args(line.split())
    assert parsed.low_score_threshold == [0.3, 0.3, 0.6, 0.3] and parsed.score_threshold == [0.6] * 4
