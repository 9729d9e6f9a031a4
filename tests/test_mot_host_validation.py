"""What wt_mot_eval_host and wt_mot_identity_host refuse before they touch a device (no GPU): the status code and the full
wt_last_error() text of every layout check the two host forms make, called straight through ctypes.

Every case starts from 1 stream x 2 frames x 2 boxes on either side and breaks one thing.  Two cases need more than that
layout to be expressible at all: decreasing stream_frame_offsets takes a second (empty) stream, because with one stream the
cover check fires first; and the decreasing-offset cases hand over arrays with four spare rows behind the four real ones,
because the walk reads the rows of the frames in front of the offending one before it reaches it.
"The same id in two classes of one frame" is accepted by the checks, so on its own it would go on to the device: here it is
followed by a broken offset array, and the text of that later check shows that the scan let it pass."""
import ctypes as C

import numpy as np
import pytest

INVALID = 1


def _lib_or_skip():
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
             g_ntraj=i32([4] * 34), h_ntraj=i32([4] * 34), limit=0)
    for side in 'gh':
        for k, v in box.items():
            a[side + k] = v.copy()
    return a


def _call(_lib, form, a):
    """(status, last error text) of one host form on the layout `a`; outputs are sized for the layout and never looked at."""
    p = lambda name: _lib.ptr(a[name]) if a[name] is not None else None
    n_problems = max(1, a['k_sets'] * a['n_streams'] * 17)
    n_rows = 8
    lead = [C.c_int64(a['n_gt']), p('gx'), p('gy'), p('gw'), p('gh'), p('g_category'), p('g_level'), p('g_id'),
            C.c_int64(a['n_frames']), p('frame_gt_offsets'), C.c_int32(a['n_streams']), p('stream_frame_offsets'),
            C.c_int32(a['k_sets']), p('set_row_offsets'), p('frame_hyp_offsets'),
            p('hx'), p('hy'), p('hw'), p('hh'), p('h_category'), p('h_id')]
    lib = _lib.lib()
    if form == 'eval':
        counts, iou_sum = np.zeros(n_problems * 10, np.int64), np.zeros(n_problems * 2, np.float64)
        match, switch = np.zeros(n_rows, np.int64), np.zeros(n_rows, np.uint8)
        rc = lib.wt_mot_eval_host(*lead, C.c_int32(a['n_classes']), p('thr'), _lib.ptr(counts), _lib.ptr(iou_sum),
                                  _lib.ptr(match), _lib.ptr(switch))
    else:
        counts, match = np.zeros(n_problems * 6, np.int64), np.zeros(n_rows * 2, np.int64)
        rc = lib.wt_mot_identity_host(*lead, p('g_ntraj'), p('h_ntraj'), C.c_int32(a['n_classes']), p('thr'),
                                      C.c_size_t(a['limit']), _lib.ptr(counts), _lib.ptr(match))
    msg = lib.wt_last_error()
    return rc, msg.decode() if msg else ''


def _set(name, index, value):
    def change(a):
        a[name][index] = value
    return change


def _replace(**kw):
    def change(a):
        a.update((k, np.asarray(v, a[k].dtype) if isinstance(v, list) else v) for k, v in kw.items())
    return change


def _both(*changes):
    def change(a):
        for c in changes:
            c(a)
    return change


FITS = 'result set 0: frame_hyp_offsets do not fit its rows'
HYP_ORDER = 'result set 0: frame_hyp_offsets must be non-decreasing'
TWICE = 'ground truth: a trajectory index is out of range or occurs twice in frame %d'
HYP_TWICE = 'result set 0: a trajectory index is out of range or occurs twice in frame %d'

# name, change to the layout, expected text of the CLEAR-MOT form, expected text of the identity form (None: not applicable)
CASES = [
    ('null_thr', _replace(thr=None), 'wt_mot_eval_host: bad argument', 'wt_mot_identity_host: bad argument'),
    ('null_frame_hyp_offsets', _replace(frame_hyp_offsets=None), 'wt_mot_eval_host: bad argument', 'wt_mot_identity_host: bad argument'),
    ('no_result_set', _replace(k_sets=0), 'wt_mot_eval_host: bad argument', 'wt_mot_identity_host: bad argument'),
    ('n_classes_0', _replace(n_classes=0), 'wt_mot_eval: n_classes must be 1..16', 'wt_mot_identity: n_classes must be 1..16'),
    ('n_classes_17', _replace(n_classes=17), 'wt_mot_eval: n_classes must be 1..16', 'wt_mot_identity: n_classes must be 1..16'),
    ('gt_offsets_do_not_end_at_n_gt', _set('frame_gt_offsets', 2, 3),
     'wt_mot_eval_host: CSR offsets do not cover the rows', 'wt_mot_identity_host: CSR offsets do not cover the rows'),
    ('set_row_offsets_do_not_start_at_0', _set('set_row_offsets', 0, 1),
     'wt_mot_eval_host: CSR offsets do not cover the rows', 'wt_mot_identity_host: CSR offsets do not cover the rows'),
    ('stream_offsets_decrease', _replace(n_streams=2, stream_frame_offsets=[0, 3, 2]),
     'stream_frame_offsets must be non-decreasing', 'stream_frame_offsets must be non-decreasing'),
    ('gt_offsets_decrease', _both(_set('frame_gt_offsets', 1, 5), _replace(g_id=[0, 1, 2, 3, 4, 5, 6, 7], g_ntraj=[8] * 34)),
     'frame_gt_offsets must be non-decreasing', 'frame_gt_offsets must be non-decreasing'),
    ('hyp_offsets_do_not_fit', _set('frame_hyp_offsets', 2, 5), FITS, FITS),
    ('hyp_offsets_do_not_start_at_0', _set('frame_hyp_offsets', 0, 1), FITS, FITS),
    ('hyp_offsets_decrease', _replace(frame_hyp_offsets=[0, 3, 2], h_id=[0, 1, 2, 3, 4, 5, 6, 7]), HYP_ORDER, HYP_ORDER),
    ('negative_gt_id', _set('g_id', 1, -1), 'ground-truth row 1: negative object id', TWICE % 0),
    ('negative_gt_id_outside_the_classes', _both(_set('g_id', 3, -5), _set('g_category', 3, 3), _set('frame_hyp_offsets', 2, 5)),
     'ground-truth row 3: negative object id', FITS),          # the identity form skips the row, the CLEAR-MOT form looks at every id
    ('gt_id_twice', _set('g_id', 3, 0), 'ground truth: an object id occurs twice in frame 1', TWICE % 1),
    ('gt_id_in_two_classes_is_accepted', _both(_set('g_id', 1, 0), _set('g_category', 1, 2), _set('frame_hyp_offsets', 2, 5)), FITS, FITS),
    ('hyp_id_twice', _set('h_id', 1, 0), 'result set 0: an object id is negative or occurs twice in frame 0', HYP_TWICE % 0),
    ('negative_hyp_id', _set('h_id', 2, -1), 'result set 0: an object id is negative or occurs twice in frame 1', HYP_TWICE % 1),
    ('hyp_id_in_two_classes_is_accepted', _both(_set('h_id', 1, 0), _set('h_category', 1, 2), _replace(frame_hyp_offsets=[0, 2, 1])),
     HYP_ORDER, HYP_ORDER),
    ('hyp_row_outside_the_classes_is_skipped', _both(_set('h_id', 0, -7), _set('h_category', 0, 3), _replace(frame_hyp_offsets=[0, 2, 1])),
     HYP_ORDER, HYP_ORDER),
    ('gt_trajectory_equal_to_its_count', _set('g_ntraj', 0, 1), None, TWICE % 0),
    ('hyp_trajectory_equal_to_its_count', _set('h_ntraj', 0, 1), None, HYP_TWICE % 0),
    ('negative_g_ntraj', _set('g_ntraj', 1, -1), None, 'g_ntraj[1] is negative'),
    ('negative_h_ntraj', _set('h_ntraj', 0, -2), None, 'h_ntraj[0] is negative'),
]


PARAMS = [pytest.param(form, change, text, id='%s-%s' % (name, form))
          for name, change, eval_text, identity_text in CASES
          for form, text in (('eval', eval_text), ('identity', identity_text)) if text is not None]


@pytest.mark.parametrize('form,change,expected', PARAMS)
def test_refused_before_the_device_with_this_text(form, change, expected):
    _lib = _lib_or_skip()
    a = _layout()
    change(a)
    rc, text = _call(_lib, form, a)
    assert (rc, text) == (INVALID, expected)


def test_identity_workspace_limit_is_refused_before_the_device():
    _lib = _lib_or_skip()
    a = _layout()
    a['limit'] = 64
    need = _lib.lib().wt_mot_identity_workspace
    need.restype = C.c_size_t
    # 1 result x 1 stream x 2 classes, 4 trajectories a side by the counts: per class two matrices of 4 x 5 floats
    size = int(need(C.c_int32(1), C.c_int32(1), C.c_int32(2), C.c_int64(4), C.c_int64(4), C.c_int64(2 * 2 * 4 * 5)))
    assert size > 64
    rc, text = _call(_lib, 'identity', a)
    assert (rc, text) == (INVALID, 'identity evaluation workspace too small: need %d bytes, the limit is 64 (score fewer results per call)' % size)
