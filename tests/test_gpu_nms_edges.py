"""Exact-answer tests of the integer-answer kernels behind the detector's selection step (csrc/det_nms.hip, gather_kept_kernel of
csrc/det_tail.hip): the column sweep (n <= 6144), the row sweep (above) and the segmented form of the hard NMS on the adversarial cases of
tests/nms_cases.py (chains as deep as the input, dependencies many tiles apart, uniform masks, threshold edges, degenerate and non-finite
rows, IoUs within an ulp of the threshold), the kept-row counts the sweeps write, and the compaction of a keep mask into fixed-size lists.
Every expectation is a closed form that tests/test_nms_cases.py proves on the CPU against two NMS implementations; every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import nms_cases as N
from waymo_2d_tracking_amd import _lib
from waymo_2d_tracking_amd.detnet.nn import ops

pytestmark = pytest.mark.gpu

WT_ERR_INVALID, WT_ERR_CAPACITY = 1, 4


def _dev(case):
    boxes = torch.from_numpy(case.boxes).cuda()
    idxs = None if case.idxs is None else torch.from_numpy(case.idxs).cuda()
    return boxes, idxs


def _run_single(case):
    boxes, idxs = _dev(case)
    keep, cnt = ops.nms_sorted_mask(boxes, idxs, case.thr, return_count=True)
    assert keep.dtype == torch.uint8 and cnt.dtype == torch.int32 and cnt.shape == (1,)
    return keep.cpu().numpy(), int(cnt.item())


def _assert_mask(got, want, what):
    assert set(np.unique(got).tolist()) <= {0, 1}, what                    # a uint8 mask of zeros and ones, not merely truthy
    bad = np.nonzero(got.astype(bool) != want)[0]
    assert bad.size == 0, '%s: %d rows differ, first %s (got %s, want %s)' % (what, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(),
                                                                           want[bad[:8]].tolist())


@pytest.mark.parametrize('n', N.COL_SIZES + N.ROW_SIZES)
@pytest.mark.parametrize('name', list(N.CASES))
def test_single_problem_sweeps(name, n):
    """Every case through ops.nms_sorted_mask at the sizes around a tile, at the column sweep's limit and, above it, with a last row-sweep
    tile of 1, 16, 17 and 64 rows: the keep mask is the closed form, n_keep its sum."""
    case = N.CASES[name](n)
    got, cnt = _run_single(case)
    _assert_mask(got, case.keep, '%s n=%d' % (name, n))
    assert cnt == int(case.keep.sum())
    if name == 'disjoint':
        assert cnt == n


@pytest.mark.parametrize('per_class', [N.KNIFE_PAIRS_BELOW, N.KNIFE_PAIRS_ABOVE])        # 2400 rows: column sweep, 6240 rows: row sweep
def test_knife_edge_pairs_are_decided_like_the_float32_sequence(per_class):
    """Pairs whose float32 quotient is nextafter(0.5, 0), 0.5 or nextafter(0.5, 1) at thr = 0.5: only the last suppress.  Hundreds of them
    change side if a product is fused into the sum that follows it (the count is asserted in tests/test_nms_cases.py), so a contracted
    iou_gt fails here."""
    case, flips = N.knife_edge(per_class)
    assert (case.boxes.shape[0] <= 6144) == (per_class == N.KNIFE_PAIRS_BELOW) and flips.sum() >= N.KNIFE_MIN_FLIPS
    got, cnt = _run_single(case)
    wrong = np.nonzero(got[1::2].astype(bool) != case.keep[1::2])[0]
    print('knife-edge %d rows: %d of %d pairs decided unlike the reference (%d of them among the %d that a fused form flips); per class %s'
          % (case.boxes.shape[0], wrong.size, 3 * per_class, int(flips[wrong].sum()), int(flips.sum()),
             [int((wrong % 3 == c).sum()) for c in range(3)]))
    _assert_mask(got, case.keep, 'knife-edge %d pairs' % (3 * per_class))
    assert cnt == int(case.keep.sum())
    # the same pairs in another order (other lanes, other tiles): the decisions travel with the pairs
    perm = np.random.default_rng(per_class).permutation(3 * per_class)
    rows = np.stack([2 * perm, 2 * perm + 1], axis=1).reshape(-1)
    shuffled = N.Case(case.boxes[rows], case.idxs[rows], case.thr, case.keep[rows])
    got, cnt = _run_single(shuffled)
    _assert_mask(got, shuffled.keep, 'knife-edge shuffled')
    assert cnt == int(shuffled.keep.sum())


def test_empty_input_returns_an_empty_mask_and_a_zero_count():
    keep, cnt = ops.nms_sorted_mask(torch.zeros((0, 4), device='cuda'), None, 0.5, return_count=True)
    assert keep.shape == (0,) and cnt.tolist() == [0]
    assert ops.nms_sorted_mask(torch.zeros((0, 4), device='cuda'), None, 0.5).shape == (0,)            # the default return stays a tensor
    keep, cnt = ops.nms_segmented(torch.zeros((0, 4), device='cuda'), None, [0, 0, 0], 0.5, return_count=True)
    assert keep.shape == (0,) and cnt.tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------------------------
# segmented form

def _knife_below():
    return N.knife_edge(N.KNIFE_PAIRS_BELOW)[0]


# (rows, builder) per segment; sizes 0, 1, 63, 64, 65 and 6144 in one call of 8 segments, in two arrangements
SEG_LAYOUTS = {
    'interleaved_6144': [(65, lambda n: N.ladder(n, 2)), (0, N.identical), (1, N.identical), (63, N.identical),
                         (64, lambda n: N.ladder(n, 3)), (6144, lambda n: N.interleaved_ladders(n, 256)), (2400, lambda n: _knife_below()),
                         (33, lambda n: N.ladder(n, 5))],
    'ladder_6144': [(65, N.identical), (6144, lambda n: N.ladder(n, 2)), (0, N.identical), (1, lambda n: N.ladder(n, 2)),
                    (63, lambda n: N.ladder(n, 3)), (64, lambda n: N.ladder(n, 5)), (2400, lambda n: _knife_below()),
                    (129, N.degenerate_in_ladder)],
}


def _run_segments(parts):
    cases = [build(n) for n, build in parts]
    sizes = [c.boxes.shape[0] for c in cases]
    assert sizes == [n for n, _ in parts] and all(c.thr == 0.5 for c in cases)
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert all(o % 64 for o in offs[1:-1]), offs                       # no later segment starts on a mask-word boundary of the whole list
    boxes = torch.from_numpy(np.concatenate([c.boxes for c in cases])).cuda()
    idxs = torch.from_numpy(np.concatenate([c.idxs if c.idxs is not None else np.zeros(c.boxes.shape[0], dtype=np.int32)
                                            for c in cases])).cuda()
    keep, cnt = ops.nms_segmented(boxes, idxs, offs, 0.5, return_count=True)
    keep, cnt = keep.cpu().numpy(), cnt.cpu().tolist()
    for z, c in enumerate(cases):
        _assert_mask(keep[offs[z]:offs[z + 1]], c.keep, 'segment %d (%d rows)' % (z, sizes[z]))
    assert cnt == [int(c.keep.sum()) for c in cases]                   # per segment, 0 for the empty ones
    return cases, keep


@pytest.mark.parametrize('layout', sorted(SEG_LAYOUTS))
def test_segmented_nms_eight_segments(layout):
    parts = SEG_LAYOUTS[layout]
    assert len(parts) == 8 and {0, 1, 63, 64, 65, 6144} <= {n for n, _ in parts}
    _run_segments(parts)


@pytest.mark.parametrize('n,name', [(1, 'identical'), (63, 'ladder3'), (64, 'ladder2'), (65, 'ladder2'), (6144, 'ladder2'),
                                    (6144, 'interleaved1000'), (6144, 'identical'), (2400, 'knife')])
def test_segmented_nms_one_segment(n, name):
    build = (lambda n: _knife_below()) if name == 'knife' else N.CASES[name]
    cases, keep = _run_segments([(n, build)])
    boxes, idxs = _dev(cases[0])
    assert np.array_equal(keep, ops.nms_sorted_mask(boxes, idxs, 0.5).cpu().numpy())          # and the single-problem entry agrees


def test_nms_argument_checks_return_the_error_before_any_launch():
    """9 segments, a segment above the column sweep's 6144 rows, offsets that do not start at 0 and a short workspace are refused with the
    library's error code; outputs keep their sentinel.  Every buffer is real and large enough for what the offsets describe."""
    lib = _lib.lib()
    n = 6145
    boxes = torch.from_numpy(N.disjoint(n).boxes).cuda()
    ws = torch.empty(int(lib.wd_nms_workspace(C.c_int(n))), dtype=torch.uint8, device='cuda')
    keep = torch.full((n,), 7, dtype=torch.uint8, device='cuda')
    cnt = torch.full((9,), -7, dtype=torch.int32, device='cuda')

    def segmented(offsets, n_seg=None, ws_bytes=None):
        offs = (C.c_int32 * len(offsets))(*offsets)
        return lib.wd_nms_segmented_f32(ops._p(boxes), None, offs, C.c_int(len(offsets) - 1 if n_seg is None else n_seg), C.c_float(0.5),
                                        ops._p(keep), ops._p(cnt), ops._p(ws), C.c_size_t(ws.numel() if ws_bytes is None else ws_bytes),
                                        ops._stream())

    assert segmented(list(range(0, 100, 10))) == WT_ERR_INVALID                               # 9 segments
    assert b'segments' in lib.wt_last_error()
    assert segmented([0, 0], n_seg=0) == WT_ERR_INVALID
    assert segmented([0, 6145]) == WT_ERR_INVALID                                             # one row above the column sweep
    assert b'6145' in lib.wt_last_error()
    assert segmented([0, 10, 9]) == WT_ERR_INVALID                                            # a segment of -1 rows
    assert segmented([1, 65]) == WT_ERR_CAPACITY                                              # offsets must start at 0
    need = int(lib.wd_nms_workspace(C.c_int(65)))
    assert segmented([0, 65], ws_bytes=need - 1) == WT_ERR_CAPACITY                           # the buffer itself is larger than claimed
    need = int(lib.wd_nms_workspace(C.c_int(n)))
    assert lib.wd_nms_sorted_f32(ops._p(boxes), None, C.c_int(n), C.c_float(0.5), ops._p(keep), ops._p(cnt), ops._p(ws),
                                 C.c_size_t(need - 1), ops._stream()) == WT_ERR_CAPACITY
    assert b'workspace too small' in lib.wt_last_error()
    with pytest.raises(_lib.WaymoTrackError):
        ops.nms_segmented(boxes, None, [0, 6145], 0.5)
    torch.cuda.synchronize()
    assert (keep == 7).all() and (cnt == -7).all()
    assert segmented([0, 65]) == _lib.WT_OK                                                    # and the accepted call does write
    assert cnt[:1].tolist() == [65] and (keep[:65] == 1).all() and (keep[65:] == 7).all()
    assert segmented([0, 0]) == _lib.WT_OK and cnt[:2].tolist() == [0, -7]                    # one empty segment: a zero count, no launch


# ---------------------------------------------------------------------------------------------------------------------------------
# compaction

COMPACT_SIZES = (1, 255, 256, 257, 3000)
NC = 7


def _masks(n):
    rows = np.arange(n)
    out = {'zeros': rows < 0, 'ones': rows >= 0, 'last': rows == n - 1, 'ladder': rows % 2 == 0}
    for r in (255, 256):
        if r < n:
            out['row%d' % r] = rows == r
    return out


def _caps(total, n):
    return sorted({c for c in (1, 255, 256, 257, total - 1, total, total + 1, n + 5) if c >= 1})


def _select_kept(keep, valid, order, cap):
    out = torch.full((cap,), -7, dtype=torch.int64, device='cuda')
    cnt = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib().wd_select_kept(ops._p(keep), ops._p(valid), ops._p(order), C.c_int(keep.shape[0]), C.c_int(cap), ops._p(out),
                                         ops._p(cnt), ops._stream()), 'wd_select_kept')
    return out, cnt


def _compaction_inputs(n):
    rng = np.random.default_rng(n)
    order = rng.permutation(n).astype(np.int64)
    valid = rng.random(n) < 0.7
    boxes = rng.random((n, 4), dtype=np.float32) + 1                   # no zero row: a padded slot cannot pass for a gathered one
    scores = rng.random(n, dtype=np.float32) + 1
    return order, valid, boxes, scores


@pytest.mark.parametrize('n', COMPACT_SIZES)
def test_select_kept_equals_nonzero(n):
    order, valid, _, _ = _compaction_inputs(n)
    order_d = torch.from_numpy(order).cuda()
    results = []
    for mname, keep in _masks(n).items():
        keep_d = torch.from_numpy(keep.astype(np.uint8)).cuda()
        for vname, v in (('none', None), ('random', valid), ('none_valid', np.zeros(n, dtype=bool))):
            v_d = None if v is None else torch.from_numpy(v.astype(np.uint8)).cuda()
            sel = np.nonzero(keep if v is None else keep & v)[0]
            for cap in _caps(len(sel), n):
                for oname, o_d in (('perm', order_d), ('rows', None)):
                    want = np.full(cap, -1, dtype=np.int64)
                    want[:min(len(sel), cap)] = (order[sel] if o_d is not None else sel)[:cap]
                    results.append(((mname, vname, cap, oname), _select_kept(keep_d, v_d, o_d, cap), want, min(len(sel), cap)))
    for what, (out, cnt), want, count in results:
        assert cnt.item() == count, what
        assert np.array_equal(out.cpu().numpy(), want), what             # unused slots are -1


@pytest.mark.parametrize('n', COMPACT_SIZES)
def test_gather_kept_equals_nonzero(n):
    order, valid, boxes, scores = _compaction_inputs(n)
    order_d, boxes_d, scores_d = torch.from_numpy(order).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    results = []
    for mname, keep in _masks(n).items():
        keep_d = torch.from_numpy(keep.astype(np.uint8)).cuda()
        for vname, v in (('all', np.ones(n, dtype=bool)), ('random', valid)):
            v_d = torch.from_numpy(v.astype(np.uint8)).cuda()
            sel = np.nonzero(keep & v)[0]
            for cap in _caps(len(sel), n):
                results.append(((mname, vname, cap), sel[:cap], cap, ops.gather_kept(keep_d, v_d, boxes_d, scores_d, order_d, cap),
                                ops.gather_kept(keep_d, v_d, boxes_d, scores_d, order_d, cap, num_classes=NC)))
    for what, sel, cap, (pb, pcnt), (db, ds, dc, dcnt) in results:
        k = len(sel)
        assert pcnt.item() == k and dcnt.item() == k, what
        want_b = np.zeros((cap, 4), dtype=np.float32)
        want_b[:k] = boxes[sel]
        want_s, want_c = np.zeros(cap, dtype=np.float32), np.zeros(cap, dtype=np.int64)
        want_s[:k], want_c[:k] = scores[sel], order[sel] % NC
        assert np.array_equal(pb.cpu().numpy(), want_b) and np.array_equal(db.cpu().numpy(), want_b), what      # unused rows are zero
        assert np.array_equal(ds.cpu().numpy(), want_s) and np.array_equal(dc.cpu().numpy(), want_c), what      # class = order % nc


def test_compaction_early_exit_on_and_off_a_chunk_boundary():
    """The kernels stop after the 256-row chunk that fills the list.  With all rows set the list is full exactly at a chunk boundary for
    cap = 256 and 512, inside a chunk for 255, 257 and 300; with every other row set the boundary cases are 128 and 256.  Every result is
    the prefix of the uncapped one, whatever lies in the chunks the kernel never reads."""
    n = 3000
    order, _, boxes, scores = _compaction_inputs(n)
    order_d, boxes_d, scores_d = torch.from_numpy(order).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    ones = torch.ones(n, dtype=torch.uint8, device='cuda')
    for keep in (np.ones(n, dtype=bool), np.arange(n) % 2 == 0):
        keep_d = torch.from_numpy(keep.astype(np.uint8)).cuda()
        sel = np.nonzero(keep)[0]
        full_idx, full_cnt = _select_kept(keep_d, None, order_d, n)
        full_b, _, full_c, _ = ops.gather_kept(keep_d, ones, boxes_d, scores_d, order_d, n, num_classes=NC)
        assert full_cnt.item() == len(sel) and np.array_equal(full_idx.cpu().numpy()[:len(sel)], order[sel])
        for cap in (127, 128, 129, 255, 256, 257, 300, 512, 513):
            idx, cnt = _select_kept(keep_d, None, order_d, cap)
            b, s, c, gcnt = ops.gather_kept(keep_d, ones, boxes_d, scores_d, order_d, cap, num_classes=NC)
            assert cnt.item() == cap and gcnt.item() == cap
            assert torch.equal(idx, full_idx[:cap]) and torch.equal(b, full_b[:cap]) and torch.equal(c, full_c[:cap])


@pytest.mark.parametrize('name,n', [('ladder3', 700), ('interleaved256', 3000), ('identical', 300)])
def test_nms_select_is_batched_nms_truncated_and_padded(name, n):
    """ops.nms_select (sort, NMS, wd_select_kept) on unsorted input: the indices of the kept & valid rows in score order, -1 beyond."""
    case = N.CASES[name](n)
    rng = np.random.default_rng(n)
    perm = rng.permutation(n)                                            # input row perm[r] holds the r-th best box
    boxes, scores, valid = np.empty_like(case.boxes), np.empty(n, dtype=np.float32), np.empty(n, dtype=bool)
    boxes[perm] = case.boxes
    scores[perm] = np.linspace(1, 0, n, dtype=np.float32)
    valid_sorted = rng.random(n) < 0.8
    valid[perm] = valid_sorted
    boxes_d, scores_d, valid_d = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(valid).cuda()
    for v_d, sel in ((None, np.nonzero(case.keep)[0]), (valid_d, np.nonzero(case.keep & valid_sorted)[0])):
        for cap in _caps(len(sel), n):
            idx, cnt = ops.nms_select(boxes_d, scores_d, None, case.thr, cap, valid=v_d)
            want = np.full(cap, -1, dtype=np.int64)
            want[:min(len(sel), cap)] = perm[sel][:cap]
            assert cnt.item() == min(len(sel), cap) and np.array_equal(idx.cpu().numpy(), want), (cap, v_d is None)
    assert ops.batched_nms(boxes_d, scores_d, None, case.thr).cpu().tolist() == perm[case.keep].tolist()
