"""Every case of tests/layout_cases.py is in the class its name says - shown with the host code the kernels are twins of
(_trackset.prepare / dense_local, evaluate._align), a restatement of first-appearance numbering and the library's host function
wt_tracks_layout_probe alone.  No device is touched."""
import numpy as np
import pytest

import layout_cases as LC
from track_cases import N_CLASSES
from track_stage_support import arrays, packed_for


def prepared(offsets, results):
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    return TS.prepare(packed_for(offsets), [arrays(r) for r in results], [], N_CLASSES, 'layout')


def check_layout(case):
    offsets, results, claim = case
    p = prepared(offsets, results)
    claim(p)
    for r, res in enumerate(results):                         # prepare() itself numbers by first appearance
        local, counts = LC.first_appearance(offsets, res)
        assert LC.locals_of(p, r) == local and p['n_traj'][r].tolist() == counts, r
        assert all(np.array_equal(order, np.arange(order.size)) for order in p['orders']), 'the rows of a case ascend by slot'
    return p


def limits():
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    return TS.layout_limits()


@pytest.mark.parametrize('name', sorted(LC.LAYOUT_CASES))
def test_layout_case_is_what_it_claims(name):
    check_layout(LC.LAYOUT_CASES[name]())


def test_limits_and_probe():
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    lds_rows, lds_slots, scan_rows = limits()
    assert 64 < lds_rows <= 4096 and lds_slots >= 2 * lds_rows and scan_rows % 64 == 0 and scan_rows >= 64
    for capacity in (1, 7, lds_slots, 2 * (lds_rows + 1)):
        slots = [TS.layout_probe(i, capacity) for i in (0, 1, -1, 5, 5 + (1 << 32), -(1 << 63), (1 << 63) - 1)]
        assert all(0 <= s < capacity for s in slots), capacity
    assert TS.layout_probe(5, 0) == -1
    assert TS.layout_probe(5, lds_slots) != TS.layout_probe(5 + (1 << 32), lds_slots)      # the high word takes part


def test_colliding_ids_collide_in_the_table_in_use():
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    lds_rows, lds_slots, _ = limits()
    case = LC.colliding_ids(TS.layout_probe, lds_slots)
    p = check_layout(case)
    assert int(np.diff(p['set_row_offsets']).max()) <= lds_rows                             # so the table has lds_slots slots


@pytest.mark.parametrize('above', [0, 1])
def test_rows_on_either_side_of_the_lds_limit(above):
    lds_rows, _, _ = limits()
    check_layout(LC.many_rows(lds_rows + above))


def test_scan_seams():
    _, _, scan_rows = limits()
    for n in LC.SEAMS + (scan_rows + 1,):
        check_layout(LC.scan_seam(n))


def aligned(offsets, results, gt_json):
    from waymo_2d_tracking_amd.tracking import evaluate as E
    gt = E.load_ground_truth(gt_json)
    packed = packed_for(offsets)
    return [E._align(gt, E.tracks_from_packed(packed, arrays(r)), N_CLASSES) for r in results]


@pytest.mark.parametrize('name', sorted(LC.EVAL_CASES))
def test_eval_case_is_what_it_claims(name):
    offsets, results, gt_json, claim = LC.EVAL_CASES[name]()
    claim(aligned(offsets, results, gt_json))


def test_slot_map_names_the_frames_align_finds():
    """the host-made map of the chain sends every row where _align sends it"""
    from waymo_2d_tracking_amd.tracking import chain, evaluate as E
    for name in sorted(LC.EVAL_CASES):
        offsets, results, gt_json, _ = LC.EVAL_CASES[name]()
        gt, packed = E.load_ground_truth(gt_json), packed_for(offsets)
        smap = chain.slot_map(packed, gt)
        assert smap.shape == (offsets[-1],) and smap.dtype == np.int64
        known = smap[smap >= 0]
        assert len(set(known.tolist())) == known.size, name                                # no ground-truth slot is named twice
        for res, (order, hyp_offsets, _) in zip(results, aligned(offsets, results, gt_json)):
            n_on = int(hyp_offsets[-1])
            frame_of = np.searchsorted(hyp_offsets, np.arange(n_on), side='right') - 1
            cat = np.asarray(res['category'])
            for i, g in zip(order[:n_on].tolist(), frame_of.tolist()):
                assert smap[res['frame'][i]] == g, (name, i)
            for i in order[n_on:].tolist():
                assert smap[res['frame'][i]] < 0 or not 1 <= cat[i] <= N_CLASSES, (name, i)


def test_refusals_are_what_they_claim():
    from waymo_2d_tracking_amd.tracking import _trackset as TS
    offsets, results, counts, _ = LC.REFUSALS['descending_slots']()
    p = TS.prepare(packed_for(offsets), [arrays(r) for r in results], [], N_CLASSES, 'layout')
    assert p['orders'][0].tolist() != list(range(counts[0]))                                # prepare() has to sort them: not the device route's input
    offsets, results, counts, _ = LC.REFUSALS['slot_beyond_the_set']()
    assert max(results[0]['frame']) == offsets[-1]
    with pytest.raises(ValueError, match='frame outside'):
        TS.prepare(packed_for(offsets), [arrays(r) for r in results], [], N_CLASSES, 'layout')
    offsets, results, counts, status = LC.REFUSALS['negative_row_count']()
    assert sorted(counts)[0] == -5 and status == 'WT_ERR_NUMERIC' and len(results) == 3
