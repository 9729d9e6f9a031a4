"""tests/split_ref.py (the plain-Python restatement of DESIGN.md section 25) pinned with answers computed by hand, and the two
chains the pass exists for - split, then stitch (tests/stitch_ref.py), then refine (tests/refine_ref.py).  No GPU."""
import refine_cases
import refine_ref
import split_cases
import split_ref
import stitch_cases
import stitch_ref
from split_cases import job, line, result

OFFSETS = [0, 10]


def pieces(rows, j):
    return split_ref.split(OFFSETS, result(rows), j)['piece']


def test_a_fast_object_is_not_shredded_under_linear_motion():
    """40 px per slot at width 50: the held boxes meet in 10 x 40 of 2 * 2000 - 400, IoU 1/9; every prediction is exact"""
    done = split_ref.split(OFFSETS, result(line(1, range(10), v=40.0)), job(0.3))
    assert done['piece'] == [0] * 10 and done['n_new'] == 0 and done['object_id'] == [1] * 10
    assert done['test'] == [[-1.0, -1.0], [-1.0, 1.0]] + [[1.0, 1.0]] * 7 + [[1.0, -1.0]]


def test_one_jump_is_one_break():
    """+500 from slot 5 on: both tests of the pair (4, 5) are 0; the pair (5, 6) fails forward (the velocity spans the jump) and
    passes backward"""
    done = split_ref.split(OFFSETS, result(line(1, range(10), v=40.0, jump={f: 500.0 for f in range(5, 10)})), job(0.3))
    assert done['piece'] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1]
    assert done['test'][5] == [0.0, 0.0] and done['test'][6] == [0.0, 1.0] and done['test'][4] == [1.0, 0.0]
    assert done['object_id'] == [1] * 5 + [2] * 5 and done['new'] == [-1] * 5 + [0] * 5 and done['breaks'] == [1] and done['n_new_pieces'] == [1]


def test_an_outlier_row_becomes_a_piece_of_its_own():
    for v in (3.0, 40.0):
        done = split_ref.split(OFFSETS, result(line(1, range(10), v=v, jump={5: 500.0})), job(0.3))
        assert done['piece'] == [0, 0, 0, 0, 0, 1, 2, 2, 2, 2], v
        assert done['object_id'] == [1] * 5 + [2] + [3] * 4
        assert done['test'][7] == [0.0, 1.0]                              # the pair after the outlier's passes on its backward test


def test_hold_breaks_every_pair_of_the_fast_object():
    done = split_ref.split(OFFSETS, result(line(1, range(10), v=40.0)), job(0.3, motion='hold'))
    assert done['piece'] == list(range(10)) and done['n_new'] == 9
    assert done['test'] == [[-1.0, -1.0]] + [[400.0 / 3600.0, -1.0]] * 9
    slow = split_ref.split(OFFSETS, result(line(1, range(10), v=3.0)), job(0.3, motion='hold'))
    assert slow['piece'] == [0] * 10 and slow['test'][1] == [(47.0 * 40.0) / (4000.0 - 47.0 * 40.0), -1.0]


def test_two_rows_under_linear_use_the_hold_test():
    rows = line(1, [2, 3], v=40.0)
    for motion in ('linear', 'hold'):
        done = split_ref.split(OFFSETS, result(rows), job(0.3, motion=motion))
        assert done['test'] == [[-1.0, -1.0], [400.0 / 3600.0, -1.0]] and done['piece'] == [0, 1]
    assert split_ref.split(OFFSETS, result(rows), job(0.1))['piece'] == [0, 0]


def test_rules_off_change_nothing_and_first_new_id_is_taken():
    rows = line(5, range(10), v=40.0, jump={f: 500.0 for f in range(5, 10)})
    off = split_ref.split(OFFSETS, result(rows), job())
    assert off['piece'] == [0] * 10 and off['object_id'] == [5] * 10 and all(t == [-1.0, -1.0] for t in off['test'])
    assert split_ref.split(OFFSETS, result(rows), job(0.3))['object_id'] == [5] * 5 + [6] * 5
    assert split_ref.split(OFFSETS, result(rows), job(0.3, first_new_id=40))['object_id'] == [5] * 5 + [40] * 5
    shuffled = [rows[i] for i in (7, 2, 9, 0, 5, 1, 8, 3, 6, 4)]
    done = split_ref.split(OFFSETS, result(shuffled), job(0.3))
    assert done['piece'] == [1 if r[0] >= 5 else 0 for r in shuffled]     # per-row outputs in the caller's order


def with_ids(res, done):
    return dict(res, object_id=list(done['object_id']))


def test_swap_chain_split_then_stitch_gives_two_pure_identities():
    """two objects on parallel lines; the tracker's ids swap from slot 10 on"""
    rows = []
    for f in range(20):
        a, b = (1, 2) if f < 10 else (2, 1)
        rows += [(f, 1, [10.0 * f, 0.0, 50.0, 40.0], 0.9, a), (f, 1, [10.0 * f, 200.0, 50.0, 40.0], 0.9, b)]
    res = result(rows)
    done = split_ref.split([0, 20], res, job(0.3))
    assert done['n_new'] == 2 and done['breaks'] == [1, 1]
    assert sorted(set(done['object_id'])) == [1, 2, 3, 4]
    linked = stitch_ref.stitch([0, 20], with_ids(res, done), stitch_cases.job(max_link=1, link_iou=0.3))
    assert sorted((f, t, n) for f, t, n, _ in linked['links']) == [(1, 4, 1), (2, 3, 1)]
    line_of = lambda i: res['bbox'][i][1]
    assert set(linked['object_id'][i] for i in range(40) if line_of(i) == 0.0) == {1}
    assert set(linked['object_id'][i] for i in range(40) if line_of(i) == 200.0) == {2}
    # without the split, stitching has nothing to link and the impurity stays
    assert stitch_ref.stitch([0, 20], res, stitch_cases.job(max_link=1, link_iou=0.3))['links'] == []


def test_outlier_chain_split_stitch_refine_replaces_the_outlier():
    res = result(line(1, range(10), v=3.0, jump={5: 500.0}))
    done = split_ref.split(OFFSETS, res, job(0.3))
    assert done['object_id'] == [1] * 5 + [2] + [3] * 4
    linked = stitch_ref.stitch(OFFSETS, with_ids(res, done), stitch_cases.job(max_link=2, link_iou=0.3, motion='linear'))
    assert linked['object_id'] == [1] * 5 + [2] + [1] * 4 and [(f, t, n) for f, t, n, _ in linked['links']] == [(1, 3, 2)]
    refined = refine_ref.refine(OFFSETS, with_ids(res, linked), refine_cases.job(max_gap=1, min_len=2))
    assert refined['frame'] == list(range(10)) and refined['object_id'] == [1] * 10
    assert refined['bbox'][5] == [15.0, 0.0, 50.0, 40.0] and refined['source'][5] < 0
    assert [b[0] for b in refined['bbox']] == [3.0 * f for f in range(10)]


def test_same_trajectory_twice_in_a_slot_is_refused():
    import pytest
    rows = line(1, range(3)) + [(1, 1, [0.0, 0.0, 5.0, 5.0], 0.9, 1)]
    with pytest.raises(ValueError, match='occurs twice in slot 1'):
        split_ref.split(OFFSETS, result(rows), job(0.3))
    assert sorted(split_cases.CASES) == sorted(['threshold_edge', 'contraction', 'holes', 'ends', 'disagreement', 'gap_rule', 'classes', 'extremes',
                                                'non_finite', 'stream_sharing'])
