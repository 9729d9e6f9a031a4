"""The HOTA metric's host side without a GPU: what wt_mot_hota_host refuses before it touches a device (status and the full
wt_last_error() text, straight through ctypes, in the manner of tests/test_mot_host_validation.py), how wt_mot_hota_workspace grows,
how evaluate_hota splits K results into calls, HotaResult from hand-made counts including every NaN case, and the parser."""
import ctypes as C
import math

import numpy as np
import pytest

INVALID, CAPACITY = 1, 4


@pytest.fixture(scope='module')
def _lib():
    from waymo_2d_tracking_amd import build
    build.build(verbose=False)
    from waymo_2d_tracking_amd import _lib
    return _lib


def _layout(n_classes=2):
    """1 stream x 2 frames x 2 boxes of class 1 on both sides, four spare rows behind (never inside n_gt or a set's rows)."""
    f64 = lambda v: np.asarray(v, np.float64)
    i32 = lambda v: np.asarray(v, np.int32)
    i64 = lambda v: np.asarray(v, np.int64)
    box = dict(x=f64([0, 50, 0, 50, 0, 50, 0, 50]), y=f64([0] * 8), w=f64([10] * 8), h=f64([10] * 8))
    a = dict(n_gt=4, n_frames=2, n_streams=1, k_sets=1, n_classes=n_classes, thr=f64([0.5] * 17),
             g_category=i32([1] * 8), g_level=i32([1] * 8), g_id=i32([0, 1, 0, 1, 2, 3, 2, 3]),
             frame_gt_offsets=i64([0, 2, 4]), stream_frame_offsets=i64([0, 2, 2]),
             set_row_offsets=i64([0, 4]), frame_hyp_offsets=i64([0, 2, 4]),
             h_category=i32([1] * 8), h_id=i32([0, 1, 0, 1, 2, 3, 2, 3]),
             g_ntraj=i32([4] * 34), h_ntraj=i32([4] * 34), limit=0, counts=True, sums=True)
    for side in 'gh':
        for k, v in box.items():
            a[side + k] = v.copy()
    return a


def _call(_lib, a):
    """(status, last error text) of wt_mot_hota_host on the layout `a`; outputs are sized for the layout and never looked at."""
    p = lambda name: _lib.ptr(a[name]) if a[name] is not None else None
    n_problems = max(1, a['k_sets'] * a['n_streams'] * 17)
    counts, sums, match = np.zeros(n_problems * 2 * 21, np.int64), np.zeros(n_problems * 2 * 19 * 4, np.float64), np.zeros(8 * 2, np.int64)
    rc = _lib.lib().wt_mot_hota_host(
        C.c_int64(a['n_gt']), p('gx'), p('gy'), p('gw'), p('gh'), p('g_category'), p('g_level'), p('g_id'),
        C.c_int64(a['n_frames']), p('frame_gt_offsets'), C.c_int32(a['n_streams']), p('stream_frame_offsets'),
        C.c_int32(a['k_sets']), p('set_row_offsets'), p('frame_hyp_offsets'),
        p('hx'), p('hy'), p('hw'), p('hh'), p('h_category'), p('h_id'), p('g_ntraj'), p('h_ntraj'), C.c_int32(a['n_classes']), p('thr'),
        C.c_size_t(a['limit']), _lib.ptr(counts) if a['counts'] else None, _lib.ptr(sums) if a['sums'] else None, _lib.ptr(match))
    msg = _lib.lib().wt_last_error()
    return rc, msg.decode() if msg else ''


def _set(name, index, value):
    def change(a):
        a[name][index] = value
    return change


def _replace(**kw):
    def change(a):
        a.update((k, np.asarray(v, a[k].dtype) if isinstance(v, list) else v) for k, v in kw.items())
    return change


def _many_boxes(n):
    """One frame with n boxes of class 1 in the ground truth (trajectory i = box i), one hypothesis."""
    def change(a):
        a.update(n_gt=n, n_frames=1, gx=np.arange(n, dtype=np.float64) * 20, gy=np.zeros(n), gw=np.full(n, 10.), gh=np.full(n, 10.),
                 g_category=np.ones(n, np.int32), g_level=np.ones(n, np.int32), g_id=np.arange(n, dtype=np.int32),
                 frame_gt_offsets=np.asarray([0, n], np.int64), stream_frame_offsets=np.asarray([0, 1], np.int64),
                 frame_hyp_offsets=np.asarray([0, 1], np.int64), set_row_offsets=np.asarray([0, 1], np.int64),
                 g_ntraj=np.asarray([n, 0], np.int32))
    return change


BAD, COVER = 'wt_mot_hota_host: bad argument', 'wt_mot_hota_host: CSR offsets do not cover the rows'
CASES = [
    ('null_thr', _replace(thr=None), INVALID, BAD),
    ('null_frame_hyp_offsets', _replace(frame_hyp_offsets=None), INVALID, BAD),
    ('null_set_row_offsets', _replace(set_row_offsets=None), INVALID, BAD),
    ('null_g_ntraj', _replace(g_ntraj=None), INVALID, BAD),
    ('null_h_ntraj', _replace(h_ntraj=None), INVALID, BAD),
    ('null_counts', _replace(counts=False), INVALID, BAD),
    ('null_sums', _replace(sums=False), INVALID, BAD),
    ('no_result_set', _replace(k_sets=0), INVALID, BAD),
    ('n_classes_0', _replace(n_classes=0), INVALID, 'wt_mot_hota: n_classes must be 1..16'),
    ('n_classes_17', _replace(n_classes=17), INVALID, 'wt_mot_hota: n_classes must be 1..16'),
    ('gt_offsets_do_not_end_at_n_gt', _set('frame_gt_offsets', 2, 3), INVALID, COVER),
    ('set_row_offsets_do_not_start_at_0', _set('set_row_offsets', 0, 1), INVALID, COVER),
    ('stream_offsets_do_not_end_at_n_frames', _set('stream_frame_offsets', 1, 1), INVALID, COVER),
    ('stream_offsets_decrease', _replace(n_streams=2, stream_frame_offsets=[0, 3, 2]), INVALID, 'stream_frame_offsets must be non-decreasing'),
    ('hyp_offsets_do_not_fit', _set('frame_hyp_offsets', 2, 5), INVALID, 'result set 0: frame_hyp_offsets do not fit its rows'),
    ('hyp_offsets_decrease', _replace(frame_hyp_offsets=[0, 3, 2], h_id=[0, 1, 2, 3, 4, 5, 6, 7]), INVALID,
     'result set 0: frame_hyp_offsets must be non-decreasing'),
    ('gt_trajectory_twice', _set('g_id', 3, 0), INVALID, 'ground truth: a trajectory index is out of range or occurs twice in frame 1'),
    ('hyp_trajectory_equal_to_its_count', _set('h_ntraj', 0, 1), INVALID,
     'result set 0: a trajectory index is out of range or occurs twice in frame 0'),
    ('negative_g_ntraj', _set('g_ntraj', 1, -1), INVALID, 'g_ntraj[1] is negative'),
    ('negative_h_ntraj', _set('h_ntraj', 0, -2), INVALID, 'h_ntraj[0] is negative'),
    ('4097_boxes_in_one_frame', _many_boxes(4097), CAPACITY, '4097 boxes of one class in one frame: the assignment kernel takes at most 4096 a side'),
    ('4097_trajectories', _set('h_ntraj', 0, 4097), CAPACITY, '4097 trajectories of one class in one stream: the HOTA kernel takes at most 4096 a side'),
    ('65536_frames_in_one_stream', _replace(n_frames=65536, stream_frame_offsets=[0, 65536], frame_gt_offsets=[0] * 65536 + [4]), CAPACITY,
     '65536 frames in one stream: the HOTA kernel takes at most 65535'),
]


@pytest.mark.parametrize('change,status,expected', [pytest.param(c, s, t, id=n) for n, c, s, t in CASES])
def test_refused_before_the_device_with_this_text(_lib, change, status, expected):
    a = _layout()
    change(a)
    assert _call(_lib, a) == (status, expected)


def _workspace(_lib, *args):
    fn = _lib.lib().wt_mot_hota_workspace
    fn.restype = C.c_size_t
    k, s, c, boxes, g, h, cells = args
    return int(fn(C.c_int32(k), C.c_int32(s), C.c_int32(c), C.c_int64(boxes), C.c_int64(g), C.c_int64(h), C.c_int64(cells)))


def test_workspace_limit_is_refused_before_the_device(_lib):
    a = _layout()
    a['limit'] = 64
    # 1 result x 1 stream x 2 classes, 2 boxes a frame, 4 trajectories a side by the counts: per class two matrices of 4 x 4 cells
    size = _workspace(_lib, 1, 1, 2, 2, 4, 4, 2 * 2 * 4 * 4)
    assert size > 64
    assert _call(_lib, a) == (INVALID, 'HOTA evaluation workspace too small: need %d bytes, the limit is 64 (score fewer results per call)' % size)


def test_workspace_grows_with_every_argument(_lib):
    base = (2, 3, 4, 100, 50, 60, 10000)
    size = _workspace(_lib, *base)
    assert size > 10000 * 46                                   # a cell is a float64 and 19 uint16
    for i, more in enumerate((3, 4, 5, 200, 5000, 5000, 20000)):
        args = list(base)
        args[i] = more
        if i in (4, 5):
            assert _workspace(_lib, *args) == 0                # more than 4096 trajectories: no size
            args[i] = 4096
        assert _workspace(_lib, *args) > size, i
    assert _workspace(_lib, 1, 1, 1, 4097, 1, 1, 0) == 0 and _workspace(_lib, 0, 1, 1, 1, 1, 1, 0) == 0
    assert _workspace(_lib, 1, 1, 1, 91, 1, 1, 0) - _workspace(_lib, 1, 1, 1, 90, 1, 1, 0) > 91 * 91 * 4      # the matrix leaves LDS: a copy per wave in the workspace
    assert _workspace(_lib, 1, 0, 1, 1, 1, 1, 0) > 0


def test_call_splitting(_lib):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    g_ntraj = np.asarray([[10, 0, 0, 5]], np.int32)
    h_ntraj = np.asarray([[[12, 0, 0, 3]], [[40, 1, 0, 9]], [[7, 0, 0, 7]], [[7, 0, 0, 7]]], np.int32)
    cells = E._matrix_cells(g_ntraj, h_ntraj)
    assert cells.tolist() == [[[240, 0, 0, 30]], [[800, 0, 0, 90]], [[140, 0, 0, 70]], [[140, 0, 0, 70]]]
    lib = _lib.lib()
    assert E._hota_calls(lib, g_ntraj, h_ntraj, 20, 0) == [(0, 4)] == E._hota_calls(lib, g_ntraj, h_ntraj, 20, E.DEFAULT_WORKSPACE_LIMIT)
    assert E._hota_calls(lib, g_ntraj, h_ntraj, 20, 1) == [(0, 1), (1, 2), (2, 3), (3, 4)]       # a limit nothing fits: one set per call, the library refuses
    # a limit that admits the last two results together and neither other pair of neighbours
    last_two = E._hota_workspace(lib, 2, 1, 4, 20, 10, 7, int(cells[2:].sum()))
    assert last_two < E._hota_workspace(lib, 2, 1, 4, 20, 10, 40, int(cells[:2].sum()))
    assert last_two < E._hota_workspace(lib, 2, 1, 4, 20, 10, 40, int(cells[1:3].sum()))
    assert E._hota_calls(lib, g_ntraj, h_ntraj, 20, last_two) == [(0, 1), (1, 2), (2, 4)]


def _result(counts, sums):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    return E.HotaResult(np.asarray(counts, np.int64), np.asarray(sums, np.float64), 0, ['s%d' % i for i in range(len(counts))])


def test_hota_result_from_hand_made_counts():
    from waymo_2d_tracking_amd.tracking import evaluate as E
    counts = np.zeros((2, 4, 2, 21), np.int64)
    sums = np.zeros((2, 4, 2, 19, 4), np.float64)
    # class 1, LEVEL_2: stream 0 has gt 6, hyp 5, tp 4 up to alpha_9 and 2 above; stream 1 has gt 2, hyp 3, tp 2 up to alpha_9
    counts[0, 0, 1] = [6, 5] + [4] * 10 + [2] * 9
    counts[1, 0, 1] = [2, 3] + [2] * 10 + [0] * 9
    sums[0, 0, 1, :10] = [3.0, 3.5, 3.25, 3.2]
    sums[0, 0, 1, 10:] = [1.0, 1.5, 1.25, 1.8]
    sums[1, 0, 1, :10] = [1.0, 2.0, 1.0, 1.5]
    # class 2, LEVEL_2: ground truth only; class 4: hypotheses only; class 3 and all of LEVEL_1: nothing
    counts[0, 1, 1, 0] = 7
    counts[1, 3, 1, 1] = 9
    r = _result(counts, sums)
    row = r.table[1][2]
    assert (row['gt'], row['hyp'], row['tp']) == (8, 8, [6] * 10 + [2] * 9)
    assert row['per_alpha']['DetA'] == [6 / 10] * 10 + [2 / 14] * 9 and row['per_alpha']['DetRe'] == [6 / 8] * 10 + [2 / 8] * 9
    assert row['per_alpha']['AssA'] == [4.0 / 6] * 10 + [1.0 / 2] * 9 and row['per_alpha']['AssRe'][0] == 5.5 / 6 and row['per_alpha']['AssPr'][18] == 1.25 / 2
    assert row['per_alpha']['LocA'] == [4.7 / 6] * 10 + [1.8 / 2] * 9
    assert row['per_alpha']['HOTA'][0] == math.sqrt(6 / 10 * (4.0 / 6)) and row['HOTA(0)'] == row['per_alpha']['HOTA'][0]
    assert row['HOTA'] == pytest.approx((10 * math.sqrt(0.4) + 9 * math.sqrt(1 / 14)) / 19, rel=1e-15)
    assert row['DetA'] == pytest.approx((10 * 0.6 + 9 * 2 / 14) / 19, rel=1e-15) and row['LocA(0)'] == 4.7 / 6
    assert row['sums']['ass'] == [4.0] * 10 + [1.0] * 9
    # ground truth only: detection 0, precision undefined, no threshold with a match
    row = r.table[2][2]
    assert row['DetA'] == 0.0 and row['DetRe'] == 0.0 and math.isnan(row['DetPr']) and math.isnan(row['LocA']) and math.isnan(row['LocA(0)'])
    assert row['HOTA'] == 0.0 and row['AssA'] == 0.0 and row['AssRe'] == 0.0 and row['AssPr'] == 0.0 and row['HOTA(0)'] == 0.0
    # hypotheses only: recall undefined
    row = r.table[4][2]
    assert row['DetA'] == 0.0 and row['DetPr'] == 0.0 and math.isnan(row['DetRe']) and math.isnan(row['LocA']) and row['HOTA'] == 0.0
    # nothing on either side: everything undefined but the association scores, which are 0 without a match
    for row in (r.table[3][2], r.table[1][1], r.table['ALL'][1]):
        assert all(math.isnan(row[n]) for n in ('HOTA', 'DetA', 'DetRe', 'DetPr', 'LocA', 'HOTA(0)', 'LocA(0)'))
        assert row['AssA'] == 0.0 and row['AssRe'] == 0.0 and row['AssPr'] == 0.0
    # ALL = classes 1, 2, 4 from the added counts
    row = r.table['ALL'][2]
    assert (row['gt'], row['hyp'], row['tp']) == (15, 17, [6] * 10 + [2] * 9)
    assert row['per_alpha']['DetA'][0] == 6 / 26 and row['per_alpha']['AssA'][0] == 4.0 / 6 and r.hota() == row['HOTA']
    # LocA averages over the thresholds with a match only
    counts[:, :, :, 2 + 10:] = 0
    row = _result(counts, sums).table[1][2]
    assert row['LocA'] == pytest.approx(4.7 / 6, rel=1e-15) and row['DetA'] == pytest.approx(10 * 0.6 / 19, rel=1e-15)
    assert set(E.HOTA_NAMES) <= set(row) and r.as_json()['table']['1']['LEVEL_2']['gt'] == 8
    text = E.format_hota_table(r, 'name').split('\n')
    assert text[0] == 'name  HOTA' and len(text) == 2 + 5 * 2 and text[1].split()[:4] == ['class', 'level', 'HOTA', 'DetA']


def test_parser_options():
    from waymo_2d_tracking_amd.tracking import evaluate as E
    parse = E.build_parser().parse_args
    args = parse(['--annotations', 'gt.json', 'a.json'])
    assert args.hota is False and args.identity is False and args.rank_by == 'mota'
    assert parse(['--annotations', 'gt.json', '--hota', 'a.json']).hota is True
    args = parse(['--annotations', 'gt.json', '--sweep', 'd.json', '--rank-by', 'hota'])
    assert args.rank_by == 'hota' and args.hota is False          # main() turns the flag on, as it does for idf1 and --identity
    assert parse(['--annotations', 'gt.json', '--sweep', 'd.json', '--rank-by', 'idf1']).rank_by == 'idf1'
    with pytest.raises(SystemExit):
        parse(['--annotations', 'gt.json', '--rank-by', 'motp'])
