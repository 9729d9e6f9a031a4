"""Exact-answer tests of the selection kernels of the detector tail (csrc/det_tail.hip) on the adversarial cases of tests/tail_cases.py:
rpn_topk_stage_kernel with its host stage plan (ties through every chunk and thread stride, winners in the last chunk, signed zeros,
NaNs of every sign and payload, infinities and denormals, level sizes around the 8192-key chunk, one to three and more stages, k up
to 8192, refusals before any launch), sort_candidates_kernel<0> (the same score families with a payload in every column),
sort_candidates_kernel<1> (means within an ulp of the threshold, poisoned rows, clipping, n_valid) and wire_kernel (pixel boundaries,
truncation toward zero, decimal ties of the score).  Every expectation is a closed form that tests/test_tail_cases.py proves on the
CPU; every comparison is exact; output buffers start out as sentinels and rows a call must not write keep them."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import nms_cases as N
import tail_cases as T
from waymo_2d_tracking_amd import _lib
from waymo_2d_tracking_amd.detnet.nn import ops

pytestmark = pytest.mark.gpu

WT_ERR_INVALID, WT_ERR_CAPACITY = 1, 4
EXTRA = 8                                  # sentinel rows behind every output
S_BOX, S_SCORE, S_GROUP, S_VALID, S_ORDER, S_WS = -777.0, -555.0, -77, 7, -99, 0xA5


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_scores(got, want):
    """Equal as values (-0.0 == +0.0: the kernels document one key for both), NaN against NaN."""
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


def _outputs(rows, order=False):
    out = [torch.full((rows + EXTRA, 4), S_BOX, dtype=torch.float32, device='cuda'),
           torch.full((rows + EXTRA,), S_SCORE, dtype=torch.float32, device='cuda'),
           torch.full((rows + EXTRA,), S_GROUP, dtype=torch.int32, device='cuda'),
           torch.full((rows + EXTRA,), S_VALID, dtype=torch.uint8, device='cuda')]
    if order:
        out.append(torch.full((rows + EXTRA,), S_ORDER, dtype=torch.int64, device='cuda'))
    return out


def _untouched(out, start=0):
    sent = (S_BOX, S_SCORE, S_GROUP, S_VALID, S_ORDER)
    return all(bool((t[start:] == s).all()) for t, s in zip(out, sent))


# ---------------------------------------------------------------------------------------------------------------------------------
# RPN top-k

@functools.lru_cache(maxsize=None)
def _trick(n):
    return torch.zeros((n, 4), dtype=torch.float32, device='cuda'), _cuda(T.trick_anchors(n))


def _raw_topk(logits, deltas, anchors, counts, k, img_h, img_w, ws_bytes_off=0, n_levels=None):
    """wd_rpn_topk_decode_f32 on device tensors with sentinel-filled outputs and workspace -> (rc, outputs, workspace, rows)."""
    lib = _lib.lib()
    n_levels = len(counts) if n_levels is None else n_levels
    c_counts = (C.c_int * len(counts))(*counts)
    need = int(lib.wd_rpn_topk_workspace(c_counts, C.c_int(len(counts)), C.c_int(max(k, 1))))
    ws = torch.full((need + 64,), S_WS, dtype=torch.uint8, device='cuda')
    rows = sum(min(max(k, 1), max(n, 1)) for n in counts)
    out = _outputs(rows)
    torch.cuda.synchronize()
    rc = lib.wd_rpn_topk_decode_f32(ops._ptr_array(logits), ops._ptr_array(deltas), ops._ptr_array(anchors), c_counts, C.c_int(n_levels),
                                    C.c_int(k), C.c_float(img_h), C.c_float(img_w), C.c_float(ops.SCALE_CLAMP), *[ops._p(t) for t in out],
                                    ops._p(ws), C.c_size_t(need + ws_bytes_off), ops._stream())
    torch.cuda.synchronize()
    return rc, out, ws, rows


def _assert_level(name, boxes, scores, group, valid, level, n, want_idx, want_scores):
    got_idx = boxes[:, 0].astype(np.int64)
    bad = np.nonzero(got_idx != want_idx)[0]
    assert bad.size == 0, '%s: %d slots name another anchor, first slots %s: got %s, want %s' % (
        name, bad.size, bad[:8].tolist(), got_idx[bad[:8]].tolist(), want_idx[bad[:8]].tolist())
    assert np.array_equal(boxes, T.trick_anchors(n)[want_idx]), name
    assert _same_scores(scores, want_scores), name
    assert (valid == 1).all() and (group == level).all(), name


@pytest.mark.parametrize('n,k', T.TOPK_PAIRS)
@pytest.mark.parametrize('family', list(T.FAMILIES))
def test_topk_one_level(family, n, k):
    logits, winners, want_scores = T.FAMILIES[family](n, k)
    deltas, anchors = _trick(n)
    boxes, scores, group, valid = ops.rpn_topk_decode([_cuda(logits)], [deltas], [anchors], k, 1.0, float(n + 1))
    assert boxes.shape == (min(k, n), 4) and scores.dtype == torch.float32 and group.dtype == torch.int32 and valid.dtype == torch.uint8
    _assert_level('%s n=%d k=%d' % (family, n, k), boxes.cpu().numpy(), scores.cpu().numpy(), group.cpu().numpy(), valid.cpu().numpy(), 0, n,
                  winners, want_scores)


@pytest.mark.parametrize('name', list(T.MULTI_LEVEL))
def test_topk_several_levels_in_one_call(name):
    """Level l's rows start at sum_{m<l} min(k, n_m) and are what the level gives alone (the closed form), whatever stage its neighbours
    finish in; the rows behind the last level keep their sentinel; the ops wrapper returns the same rows."""
    sizes, k, families = T.MULTI_LEVEL[name]
    cases = [T.FAMILIES[f](n, k) for f, n in zip(families, sizes)]
    logits = [_cuda(c[0]) for c in cases]
    deltas, anchors = [_trick(n)[0] for n in sizes], [_trick(n)[1] for n in sizes]
    img_w = float(max(sizes) + 1)
    rc, out, ws, rows = _raw_topk(logits, deltas, anchors, list(sizes), k, 1.0, img_w)
    assert rc == _lib.WT_OK and rows == sum(min(k, n) for n in sizes)
    assert _untouched(out, rows)
    boxes, scores, group, valid = [t[:rows].cpu().numpy() for t in out]
    row = 0
    for level, (n, case) in enumerate(zip(sizes, cases)):
        kk = min(k, n)
        _assert_level('%s level %d (%s, n=%d)' % (name, level, families[level], n), boxes[row:row + kk], scores[row:row + kk],
                      group[row:row + kk], valid[row:row + kk], level, n, case[1], case[2])
        row += kk
    assert row == rows
    wrapped = ops.rpn_topk_decode(logits, deltas, anchors, k, 1.0, img_w)
    for a, b in zip(wrapped, out):
        assert np.array_equal(_bits(a.cpu().numpy()) if a.dtype == torch.float32 else a.cpu().numpy(),
                              _bits(b[:rows].cpu().numpy()) if b.dtype == torch.float32 else b[:rows].cpu().numpy())


@pytest.mark.parametrize('order', ['descending', 'ascending'])
@pytest.mark.parametrize('as_level', [0, 1])
def test_topk_validity_family(order, as_level):
    """Decoded boxes that are positive, zero-width, zero-height, negative, clipped to empty at each border and NaN: valid and group row by
    row, the boxes bit-exact to ops.decode_boxes on the expected anchors."""
    kinds, deltas, anchors, _, want_valid = T.validity_family()
    n = len(kinds)
    logits, winners, _ = T.FAMILIES[order](n, n)
    img_h, img_w = T.VALIDITY_IMG
    d_dev, a_dev = _cuda(deltas), _cuda(anchors)
    lv_logits, lv_deltas, lv_anchors, counts = [_cuda(logits)], [d_dev], [a_dev], [n]
    k = n
    first_rows = 0
    if as_level == 1:                                                   # behind a level of the identification trick
        m, k = 1500, 1000
        assert k >= n
        lv_logits.insert(0, _cuda(T.mod7(m, k)[0]))
        lv_deltas.insert(0, _trick(m)[0])
        lv_anchors.insert(0, _trick(m)[1])
        counts.insert(0, m)
        first_rows = k
    rc, out, ws, rows = _raw_topk(lv_logits, lv_deltas, lv_anchors, counts, k, img_h, img_w)
    assert rc == _lib.WT_OK and rows == first_rows + n and _untouched(out, rows)
    boxes, scores, group, valid = [t[first_rows:rows].cpu().numpy() for t in out]
    want_boxes = ops.decode_boxes(d_dev, a_dev, (1.0, 1.0, 1.0, 1.0), _cuda(winners), (img_h, img_w)).cpu().numpy()
    nan = np.isnan(want_boxes)
    assert np.array_equal(np.isnan(boxes), nan) and np.array_equal(_bits(boxes)[~nan], _bits(want_boxes)[~nan])
    for r, i in enumerate(winners):
        assert valid[r] == int(want_valid[i]) and group[r] == (as_level if want_valid[i] else -1), (r, kinds[i], boxes[r].tolist())
    assert np.array_equal(scores, logits[winners])
    if as_level == 1:
        b0 = out[0][:first_rows].cpu().numpy()
        assert np.array_equal(b0[:, 0].astype(np.int64), T.mod7(1500, 1000)[1]) and bool((out[2][:first_rows] == 0).all())


@pytest.mark.parametrize('k,n', T.STAGE_PLAN_CALLS)
def test_topk_stage_plan_serves_or_refuses_before_any_launch(k, n):
    """The rule of include/waymodet.h (tail_cases.served): a call whose plan ends within the stage limit returns the right answer, any
    other is refused with WT_ERR_INVALID before anything is launched: workspace and outputs keep their sentinels, the message names k."""
    lib = _lib.lib()
    logits, winners, want_scores = T.mod7(n, k)
    deltas, anchors = _trick(n)
    lg = _cuda(logits)
    rc, out, ws, rows = _raw_topk([lg], [deltas], [anchors], [n], k, 1.0, float(n + 1))
    print('k=%d n=%d: stages needed %s, rc %d' % (k, n, T.stages_needed(k, n), rc))
    if T.served(k, n):
        assert rc == _lib.WT_OK
        boxes, scores, group, valid = [t[:rows].cpu().numpy() for t in out]
        _assert_level('k=%d n=%d' % (k, n), boxes, scores, group, valid, 0, n, winners, want_scores)
        assert _untouched(out, rows)
        if n <= T.CHUNK:
            assert bool((ws == S_WS).all())                             # a single stage needs no key buffer
    else:
        assert rc == WT_ERR_INVALID
        assert ('k=%d' % k).encode() in lib.wt_last_error(), lib.wt_last_error()
        assert bool((ws == S_WS).all()) and _untouched(out)
        with pytest.raises(_lib.WaymoTrackError):
            ops.rpn_topk_decode([lg], [deltas], [anchors], k, 1.0, float(n + 1))


def test_topk_argument_checks_refuse_before_any_launch():
    """9 levels, an empty level, k = 0, k = 8193 and a workspace one byte short: every buffer is real and large enough."""
    lib = _lib.lib()
    n = 1000
    logits = _cuda(T.mod7(n, n)[0])
    deltas, anchors = _trick(n)

    def call(counts, k, **kw):
        m = len(counts)
        rc, out, ws, rows = _raw_topk([logits] * m, [deltas] * m, [anchors] * m, counts, k, 1.0, float(n + 1), **kw)
        return rc, bool((ws == S_WS).all()) and _untouched(out)

    assert call([100] * 9, 10) == (WT_ERR_INVALID, True)
    assert b'levels=9' in lib.wt_last_error()
    assert call([100, 0, 100], 10) == (WT_ERR_INVALID, True)
    assert b'empty level 1' in lib.wt_last_error()
    assert call([n], 0) == (WT_ERR_INVALID, True)
    assert b'k=0' in lib.wt_last_error()
    assert call([n], 8193) == (WT_ERR_INVALID, True)
    assert b'k=8193' in lib.wt_last_error()
    assert call([n], 10, n_levels=0) == (WT_ERR_INVALID, True)
    assert call([n, 900], 100, ws_bytes_off=-1) == (WT_ERR_CAPACITY, True)
    assert b'workspace too small' in lib.wt_last_error()
    with pytest.raises(_lib.WaymoTrackError):
        ops.rpn_topk_decode([logits], [deltas], [anchors], 8193, 1.0, float(n + 1))
    assert call([n, 900], 100) == (_lib.WT_OK, False)                    # and the accepted call does write


# ---------------------------------------------------------------------------------------------------------------------------------
# RPN candidate sort

def _raw_sort(c, n, rows=None):
    rows = n if rows is None else rows
    out = _outputs(rows, order=True)
    dev = {key: (None if c[key] is None else _cuda(c[key])) for key in ('boxes', 'scores', 'group', 'valid', 'valid2')}
    rc = _lib.lib().wd_sort_candidates_f32(ops._p(dev['boxes']), ops._p(dev['scores']), ops._p(dev['group']), ops._p(dev['valid']),
                                           ops._p(dev['valid2']), C.c_int(n), *[ops._p(t) for t in out], ops._stream())
    torch.cuda.synchronize()
    return rc, out, dev


@pytest.mark.parametrize('n', T.SORT_SIZES)
@pytest.mark.parametrize('family', list(T.FAMILIES))
def test_rpn_candidate_sort(family, n):
    for pattern in T.VALID_PATTERNS:
        c = T.sort_case(family, n, pattern)
        rc, out, dev = _raw_sort(c, n)
        what = '%s n=%d %s' % (family, n, pattern)
        assert rc == _lib.WT_OK and _untouched(out, n), what
        boxes, scores, group, valid, order = [t[:n].cpu().numpy() for t in out]
        bad = np.nonzero(order != c['order'])[0]
        assert bad.size == 0, '%s: %d rows out of order, first %s: got %s, want %s' % (what, bad.size, bad[:8].tolist(),
                                                                                     order[bad[:8]].tolist(), c['order'][bad[:8]].tolist())
        assert _same_scores(scores, c['out_scores']), what
        assert np.array_equal(boxes, c['out_boxes']) and np.array_equal(group, c['out_group']), what
        assert set(np.unique(valid).tolist()) <= {0, 1} and np.array_equal(valid, c['out_valid']), what
        if pattern == 'mod3':                                           # the wrapper returns the same rows
            got = ops.sort_candidates(dev['boxes'], dev['scores'], dev['group'], dev['valid'], dev['valid2'])
            assert torch.equal(got[4], out[4][:n]) and torch.equal(got[0], out[0][:n]) and torch.equal(got[3], out[3][:n])
            assert torch.equal(got[2], out[2][:n]) and _same_scores(got[1].cpu().numpy(), scores)


def test_rpn_candidate_sort_refuses_zero_and_8193_rows():
    lib = _lib.lib()
    c = T.sort_case('mod7', 8192, 'all')
    for key in ('boxes', 'scores', 'group', 'valid', 'valid2'):         # buffers of 8193 + EXTRA rows throughout
        c[key] = np.concatenate([c[key], c[key][:9]])
    for n in (0, 8193, -1):
        rc, out, dev = _raw_sort(c, n, rows=8193)
        assert rc == WT_ERR_INVALID and _untouched(out), n
        assert b'8192' in lib.wt_last_error()
    with pytest.raises(_lib.WaymoTrackError):
        ops.sort_candidates(dev['boxes'], dev['scores'], dev['group'], dev['valid'])
    rc, out, dev = _raw_sort(c, 8192, rows=8193)
    assert rc == _lib.WT_OK and _untouched(out, 8192) and not _untouched(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# box-head candidates

def _raw_box(boxes, s0, s1, s2, n_valid, thresh, rows, nc):
    n = rows * nc
    out = _outputs(n, order=True)
    nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device='cuda')
    dev = [_cuda(v) for v in (boxes, s0, s1, s2)]
    img_h, img_w = T.BOX_IMG
    rc = _lib.lib().wd_box_candidates_f32(*[ops._p(t) for t in dev], ops._p(nv), C.c_int(rows), C.c_int(nc), C.c_float(float(thresh)),
                                          C.c_float(img_h), C.c_float(img_w), *[ops._p(t) for t in out], ops._stream())
    torch.cuda.synchronize()
    return rc, out, dev, nv


@pytest.mark.parametrize('rows,nc', T.BOX_SHAPES)
@pytest.mark.parametrize('family', T.BOX_FAMILIES)
def test_box_candidates(family, rows, nc):
    """Real pairs: box (clipped, bit for bit), score, class and order; the rest: score -1.0, group -1, valid 0, in flat-index order."""
    c = T.box_case(family, rows, nc)
    n, n_real = rows * nc, c['n_real']
    rc, out, dev, nv = _raw_box(c['boxes'], c['s0'], c['s1'], c['s2'], c['n_valid'], c['thresh'], rows, nc)
    assert rc == _lib.WT_OK and _untouched(out, n)
    boxes, scores, group, valid, order = [t[:n].cpu().numpy() for t in out]
    bad = np.nonzero(order != c['order'])[0]
    assert bad.size == 0, '%d rows out of order, first %s: got %s, want %s' % (bad.size, bad[:8].tolist(), order[bad[:8]].tolist(),
                                                                              c['order'][bad[:8]].tolist())
    assert np.array_equal(_bits(scores), _bits(c['out_scores']))
    assert np.array_equal(group, c['out_group']) and np.array_equal(valid, c['out_valid'])
    assert np.array_equal(_bits(boxes[:n_real]), _bits(c['out_boxes'][:n_real]))
    if family == 'equal':                                               # the wrapper returns the same rows
        got = ops.box_candidates(dev[0], dev[1], dev[2], dev[3], nv, float(c['thresh']), *T.BOX_IMG)
        assert all(torch.equal(a, b[:n]) for a, b in zip(got, out))


def test_box_candidates_refuses_too_many_pairs_and_a_negative_threshold():
    lib = _lib.lib()
    for rows, nc in T.BOX_REFUSED_SHAPES:
        c = T.box_case('equal', rows, nc)
        rc, out, dev, nv = _raw_box(c['boxes'], c['s0'], c['s1'], c['s2'], None, T.THRESH, rows, nc)
        assert rc == WT_ERR_INVALID and _untouched(out), (rows, nc)
        assert b'8192' in lib.wt_last_error()
    c = T.box_case('equal', 37, 4)
    for thresh in (-0.05, float('nan')):
        rc, out, dev, nv = _raw_box(c['boxes'], c['s0'], c['s1'], c['s2'], None, thresh, 37, 4)
        assert rc == WT_ERR_INVALID and _untouched(out), thresh
        assert b'threshold' in lib.wt_last_error()
    with pytest.raises(_lib.WaymoTrackError):
        ops.box_candidates(dev[0], dev[1], dev[2], dev[3], None, -0.05, *T.BOX_IMG)
    for rows, nc in ((0, 4), (4, 0)):
        rc, out, dev, nv = _raw_box(c['boxes'], c['s0'], c['s1'], c['s2'], None, T.THRESH, rows, nc)
        assert rc == WT_ERR_INVALID and _untouched(out), (rows, nc)


def _real_flags(out, n):
    """Per (row, class) pair in flat order: the valid flag the kernel gave it."""
    valid, order = out[3][:n].cpu().numpy(), out[4][:n].cpu().numpy()
    assert sorted(order.tolist()) == list(range(n)) and set(np.unique(valid).tolist()) <= {0, 1}
    flags = np.empty(n, dtype=bool)
    flags[order] = valid.astype(bool)
    return flags


def test_box_candidates_knife_edge_means_are_decided_like_the_float32_sequence():
    """Means exactly nextafter(thresh, 0) and nextafter(thresh, 1) for thresh = float32(0.05) (no float32 sum reaches the threshold
    itself): only the latter are real.  Thousands of these pairs change side under the float64 mean, a division by 3.0f or the other
    association (counts asserted in tests/test_tail_cases.py), so a kernel that evaluates the mean another way fails here."""
    rows, nc = 2048, 4
    n = rows * nc
    total = wrong_n = 0
    flips = dict(flip_f64=0, flip_div=0, flip_assoc=0)
    wrong_flips = dict(flips)
    for seed in T.KNIFE_SEEDS:
        s0, s1, s2, info = T.knife_edge_scores(rows, nc, seed)
        boxes = T.box_case('equal', rows, nc)['boxes']
        rc, out, dev, nv = _raw_box(boxes, s0, s1, s2, None, T.THRESH, rows, nc)
        assert rc == _lib.WT_OK and _untouched(out, n)
        got = _real_flags(out, n)
        want = info['real'].reshape(-1)
        wrong = got != want
        total += n
        wrong_n += int(wrong.sum())
        for kind in flips:
            flips[kind] += int(info[kind].sum())
            wrong_flips[kind] += int((info[kind].reshape(-1) & wrong).sum())
        # real pairs come first, with the one score above the threshold, in flat order
        n_real = int(want.sum())
        assert np.array_equal(out[4][:n].cpu().numpy(), np.concatenate([np.nonzero(want)[0], np.nonzero(~want)[0]])) or wrong.any()
        assert wrong.any() or bool((out[1][:n_real] == float(np.nextafter(T.THRESH, T.F32(1)))).all())
        # the same pairs on other rows: the decisions travel with the pairs
        perm = np.random.default_rng(seed).permutation(rows)
        rc, out, dev, nv = _raw_box(boxes, s0[perm], s1[perm], s2[perm], None, T.THRESH, rows, nc)
        assert rc == _lib.WT_OK
        got_perm = _real_flags(out, n)
        assert np.array_equal(got_perm, info['real'][perm].reshape(-1)) or wrong.any()
    print('knife-edge means: %d of %d pairs decided unlike the float32 sequence; of them %d / %d / %d among the %d / %d / %d that the '
          'float64 mean / division by 3.0f / s0 + (s1 + s2) decide differently'
          % (wrong_n, total, wrong_flips['flip_f64'], wrong_flips['flip_div'], wrong_flips['flip_assoc'], flips['flip_f64'],
             flips['flip_div'], flips['flip_assoc']))
    assert min(flips.values()) >= T.KNIFE_MIN
    assert wrong_n == 0


def test_box_inference_composes_sort_nms_and_gather():
    """CascadeRCNN.inference on a poisoned, overlapping case against the torch sequence restated on the CPU: candidate mask, stable
    sort, greedy per-class NMS (the float32 reference of tests/nms_cases.py), first `topk` kept."""
    from waymo_2d_tracking_amd.detnet.nn.cascade_rcnn import CascadeRCNN
    rows, nc, topk, nms_thr = 1000, 4, 100, 0.5
    c = T.box_case('poison_odd', rows, nc)
    c['boxes'][:, 2:] += 100                                            # 140 x 130 boxes two pixels apart along the diagonal: long suppression chains
    n_valid = 801
    ns = types.SimpleNamespace(score_thresh=float(c['thresh']), nms_thresh=nms_thr, topk=topk)
    stages = [_cuda(c[key]) for key in ('s0', 's1', 's2')]
    img_h, img_w = T.BOX_IMG
    got = CascadeRCNN.inference(ns, _cuda(c['boxes']), stages, img_h, img_w, torch.tensor([n_valid], dtype=torch.int32, device='cuda'))
    # the restated sequence
    b, s = torch.from_numpy(c['boxes']), [torch.from_numpy(c[key]) for key in ('s0', 's1', 's2')]
    scores = (s[0] + s[1] + s[2]) * (1.0 / 3)
    row_ok = torch.isfinite(b).all(dim=1) & torch.isfinite(scores).all(dim=1) & (torch.arange(rows) < n_valid)
    b = torch.stack((b[:, 0].clamp(0, img_w), b[:, 1].clamp(0, img_h), b[:, 2].clamp(0, img_w), b[:, 3].clamp(0, img_h)), dim=1)
    real = ((scores[:, :-1] > float(c['thresh'])) & row_ok.unsqueeze(1)).reshape(-1)
    cand = torch.nonzero(real).flatten()
    cand = cand[torch.argsort(scores[:, :-1].reshape(-1)[cand], stable=True, descending=True)]
    cand_boxes, cand_cls = b[cand // nc].numpy(), (cand % nc).numpy().astype(np.int32)
    keep = N.greedy_nms_f32(cand_boxes, cand_cls, nms_thr)
    sel = cand.numpy()[keep][:topk]
    count = sel.shape[0]
    assert count == topk < keep.sum() < keep.size and real.sum() == 401 * nc      # rows 0, 2, ... 800 are real, the NMS thins them
    want_b, want_s, want_c = np.zeros((topk, 4), dtype=np.float32), np.zeros(topk, dtype=np.float32), np.zeros(topk, dtype=np.int64)
    want_b[:count], want_s[:count], want_c[:count] = b.numpy()[sel // nc], scores[:, :-1].reshape(-1).numpy()[sel], sel % nc
    assert int(got[3].item()) == count
    assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(want_b)) and np.array_equal(_bits(got[1].cpu().numpy()), _bits(want_s))
    assert np.array_equal(got[2].cpu().numpy(), want_c)


# ---------------------------------------------------------------------------------------------------------------------------------
# wire rows

@pytest.mark.parametrize('hflip', [False, True])
@pytest.mark.parametrize('sizes', T.WIRE_SIZES)
def test_wire_rows_equal_the_restatement(sizes, hflip):
    from waymo_2d_tracking_amd.detnet.nn.detectron2_det import detections_to_wire
    in_w, in_h, out_w, out_h = sizes
    seen = 0
    for name, case in T.wire_cases():
        if case['sizes'] != sizes or case['hflip'] != hflip:
            continue
        seen += 1
        n, count = case['n'], case['count']
        xywh, score, cat = T.wire_ref(case['boxes'], case['scores'], case['classes'], count, *sizes, hflip)
        boxes, scores, classes = _cuda(case['boxes']), _cuda(case['scores']), _cuda(case['classes'])
        cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device='cuda')
        xywhs, category = ops.detections_to_wire(boxes, scores, classes, cnt, in_w, in_h, out_w, out_h, hflip)
        assert xywhs.shape == (5, n) and xywhs.dtype == torch.float64 and category.dtype == torch.int32
        got = xywhs.cpu().numpy()
        want = np.array(xywh, dtype=np.float64).reshape(n, 4)
        bad = np.nonzero((got[:4].T != want).any(axis=1))[0]
        assert bad.size == 0, '%s: %d rows differ, first %s: got %s, want %s from box %s' % (
            name, bad.size, bad[:4].tolist(), got[:4].T[bad[:4]].tolist(), want[bad[:4]].tolist(), case['boxes'][bad[:4]].tolist())
        assert got[4].tolist() == score, name
        assert category.cpu().tolist() == cat, name
        # the module-level function on CUDA tensors (no count, the flip applied beforehand): the same launch
        b = torch.from_numpy(case['boxes'])
        if hflip:
            b = torch.stack((in_w - b[:, 2], b[:, 1], in_w - b[:, 0], b[:, 3]), dim=1)
        m_xywh, m_score, m_cat = detections_to_wire(b.cuda(), scores, classes, in_w, in_h, out_w, out_h)
        assert m_xywh.cpu().numpy().tolist() == want.tolist() and m_score.cpu().tolist() == score, name
        assert m_cat.cpu().tolist() == (case['classes'] + 1).tolist(), name
    assert seen == sum(len(T.wire_counts(n)) for n in T.WIRE_N)
