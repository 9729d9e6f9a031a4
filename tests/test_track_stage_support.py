"""The comparators of tests/track_stage_support.py, on a CPU: each stage's assert_same accepts a result built from the reference's
own output in the shape tracking/<stage>.py returns, and refuses it once one element of any compared field is changed or the dtype
of a field whose dtype is checked is cast; same_bits keeps the strict rule."""
import numpy as np
import pytest

import track_stage_support as S

I32, I64, F64 = np.int32, np.int64, np.float64
KEEP = {'keep': I32, 'by': I32, 'match': I32, 'row_keep': I32, 'n_dropped': I64, 'traj_offsets': I64}


def _surviving(ref, out):
    return dict((k, np.asarray(out[k])[np.asarray(ref['row_keep'], bool)]) for k in S.COLUMNS)


# stage: (a small case, the extra arrays of its result with their dtypes, the extra lists and numbers, the rows of its result,
#         the fields whose dtype the comparator checks)
SHAPES = {
    'refine': ('gap_limits', {'source': I64, 'frame_row_offsets': I64}, (), lambda ref, out: S.arrays(ref), ('bbox', 'score')),
    'stitch': ('chain_of_five', {'pred': I32, 'root': I32, 'affinity': F64, 'row_root': I32, 'n_links': I64, 'traj_offsets': I64}, ('links',),
               lambda ref, out: S.with_ids(out, ref), ('affinity',) + S.COLUMNS),
    'smooth': ('ends', {'pairs': I32}, (), lambda ref, out: S.with_boxes(out, ref), ('pairs',) + S.COLUMNS),
    'dedup': ('equal_twins', KEEP, ('dropped',), _surviving, S.COLUMNS),
    'xclass': ('rider_in_cyclist', KEEP, ('dropped',), _surviving, S.COLUMNS),
    'split': ('threshold_edge', {'piece': I32, 'new': I64, 'test': F64, 'breaks': I32, 'n_new_pieces': I64, 'traj_offsets': I64}, ('n_new',),
              lambda ref, out: S.with_ids(out, ref), ('piece', 'new', 'test', 'breaks') + S.COLUMNS),
}


def accepted(stage):
    """(got, ref, out) of the first job of the stage's case whose every compared field has something in it"""
    name, extra, plain, rows, _ = SHAPES[stage]
    offsets, result, jobs, _ = S.STAGES[stage].cases.CASES[name]()
    out = S.arrays(result)
    for job in jobs:
        ref = S.STAGES[stage].reference(offsets, result, job)
        got = dict(rows(ref, out))
        for k, dtype in extra.items():
            got[k] = np.asarray(ref[k], dtype).reshape((-1, 2) if k == 'test' else (-1,))
        for k in plain:
            got[k] = list(ref[k]) if isinstance(ref[k], list) else ref[k]
        if all(np.size(v) for v in got.values()) and all(np.isfinite(v).all() for v in got.values() if isinstance(v, np.ndarray)):
            return got, ref, out
    raise AssertionError('no job of %s fills every field with finite values' % name)


def changed(value):
    """the value with one element changed by the least there is"""
    if isinstance(value, np.ndarray):
        v = value.copy()
        v.flat[v.size // 2] = np.nextafter(v.flat[v.size // 2], np.inf) if v.dtype.kind == 'f' else v.flat[v.size // 2] + 1
        return v
    return value[:-1] if isinstance(value, list) else value + 1


def cast(value):
    return value.astype({'float64': np.float32, 'int32': I64, 'int64': I32}[value.dtype.name])


@pytest.mark.parametrize('stage', S.ORDER)
def test_assert_same_accepts_the_reference_and_refuses_every_single_change(stage):
    got, ref, out = accepted(stage)
    compare = S.STAGES[stage].assert_same
    compare(got, ref, out)
    assert set(SHAPES[stage][1]) | set(SHAPES[stage][2]) | set(S.COLUMNS) == set(got)
    for k in got:
        with pytest.raises(AssertionError):
            compare(dict(got, **{k: changed(got[k])}), ref, out)
    for k in SHAPES[stage][4]:
        with pytest.raises(AssertionError):
            compare(dict(got, **{k: cast(got[k])}), ref, out)


def test_same_bits_is_the_strict_rule():
    a = np.asarray([[1.0, np.nan], [0.0, -2.5]])
    assert S.same_bits(a, a.copy()) and S.same_bits(a, a.tolist())
    assert S.same_bits(np.asarray([np.nan]), np.asarray([-np.nan])) and S.same_bits(np.asarray([np.nan]), [np.float64(np.nan) * 2])
    assert not S.same_bits(np.asarray([0.0]), [-0.0]) and not S.same_bits(np.asarray([-0.0]), [0.0])
    assert not S.same_bits(np.asarray([1.0]), [np.nextafter(1.0, 2.0)]) and not S.same_bits(np.asarray([1.0]), [np.nextafter(1.0, 0.0)])
    assert not S.same_bits(np.asarray([1.0, 2.0], np.float32), [1.0, 2.0]) and not S.same_bits([1.0, 2.0], [1.0, 2.0])
    assert not S.same_bits(np.asarray([1.0, np.nan]), [np.nan, 1.0]) and not S.same_bits(np.asarray([1.0]), [np.nan])
    assert not S.same_bits(a, a.reshape(4)) and not S.same_bits(a[:1], a)
    assert S.same_bits(a.T, a.T.copy()) and S.same_bits(np.zeros((0, 2)), np.zeros((0, 2))) and not S.same_bits(np.zeros((0, 2)), [])


def test_reference_passes_run_in_the_order_of_the_command_line():
    from waymo_2d_tracking_amd.tracking import track
    assert [asked.__name__ for asked, _ in track.PASSES] == ['splits', 'stitches', 'dedups', 'xclasses', 'refines', 'smooths']
    assert S.ORDER == ('split', 'stitch', 'dedup', 'xclass', 'refine', 'smooth')
    # two objects two slots apart in time, the second track 3 px beside the first: stitching first makes one track of 21 and 22,
    # which the deduplication then meets in enough rows to drop track 30; given in the opposite order the answer is the same
    box = lambda dx: [100.0 + dx, 50.0, 70.0, 30.0]
    rows = [(f, 1, box(0.0), 0.9, 30) for f in range(2, 8)] + [(f, 1, box(5.0), 0.8, 21) for f in range(4)] + [(f, 1, box(5.0), 0.8, 22) for f in range(6, 10)]
    from track_cases import result
    out, packed = S.arrays(result(sorted(rows, key=lambda r: r[0]))), S.packed_for([0, 10])
    link = {'max_link': [3] * 4, 'link_iou': [0.3] * 4, 'motion': 'hold'}
    dup = {'min_frames': [2] * 4, 'dup_iou': [0.7] * 4, 'dup_frac': [0.6] * 4}
    for passes in ({'stitch': link, 'dedup': dup}, [('dedup', dup), ('stitch', link)]):
        got, refs = S.reference_passes(packed, out, passes)
        assert refs['stitch']['links'] == [(21, 22, 3, 1.0)] and refs['dedup']['dropped'] == [(30, 21, 4)] and got['object_id'].tolist() == [21] * 8
    assert S.reference_passes(packed, out, {'dedup': dup})[1]['dedup']['dropped'] == []
    with pytest.raises(AssertionError):
        S.reference_passes(packed, out, {'recover': {}})
