"""csrc/ensemble_wbf.hip (weighted boxes fusion / NMW, one wavefront per group) against the plain-Python restatement
tests/wbf_ref.py.  out5, out_counts, out_members and row_cluster are compared with ==: the kernel does the restatement's float64
operations in the same order, without contraction.  Every group of every call is compared."""
import ctypes as C
import json
import shlex

import numpy as np
import pytest

import wbf_ref as R
from wbf_cases import CASES

pytestmark = pytest.mark.gpu

METHODS = ('weighted_fusion', 'nmw')


def pack(groups, wsum=None):
    """[rows [score, x, y, w, h] per group] -> dets5, group_offsets, group_wsum"""
    dets5 = np.ascontiguousarray(np.concatenate([np.asarray(g, np.float64).reshape(-1, 5) for g in groups]) if groups else np.zeros((0, 5)))
    offsets = np.zeros(len(groups) + 1, np.int64)
    np.cumsum([len(g) for g in groups], out=offsets[1:])
    wsum = np.ones(len(groups)) if wsum is None else np.asarray(wsum, np.float64)
    return dets5, offsets, np.ascontiguousarray(wsum, dtype=np.float64)


def run_host(dets5, offsets, wsum, method, thr):
    from waymo_2d_tracking_amd.detnet import ensemble_b as EB
    return EB.merge_groups(dict(dets5=dets5, group_offsets=offsets, group_wsum=wsum, n_groups=len(offsets) - 1), method, thr)


def assert_equal(got, ref, offsets):
    out5, counts, members, row_cluster = got
    r5, rc, rm, rr = ref
    assert np.array_equal(counts, rc)
    assert np.array_equal(row_cluster, rr)
    for g, (o, c) in enumerate(zip(offsets[:-1].tolist(), rc.tolist())):          # rows past a group's count are not defined
        assert np.array_equal(out5[o:o + c], r5[o:o + c]), g
        assert np.array_equal(members[o:o + c], rm[o:o + c]), g


def check(groups, wsum, method, thr):
    dets5, offsets, wsum = pack(groups, wsum)
    ref = R.fuse_groups(dets5, offsets, wsum, method, thr)
    assert_equal(run_host(dets5, offsets, wsum, method, thr), ref, offsets)
    return ref


@pytest.mark.parametrize('name', sorted(CASES))
def test_hand_worked_case(name):
    rows, wsum, method, thr, out, members, row_cluster = CASES[name]
    xywh = [[r[0], r[1], r[2], r[3] - r[1], r[4] - r[2]] for r in rows]           # exact: the cases are dyadic
    dets5, offsets, ws = pack([xywh], [wsum])
    out5, counts, mem, rc = run_host(dets5, offsets, ws, method, thr)
    assert counts.tolist() == [len(out)] and out5[:len(out)].tolist() == [[float(v) for v in r] for r in out]
    assert mem[:len(out)].tolist() == members and rc.tolist() == row_cluster


SIZES = (0, 1, 63, 64, 65, 129)


@pytest.mark.parametrize('method', METHODS)
def test_disjoint_boxes_make_one_cluster_each(method):
    """The cluster count crosses the 64-lane stride of the matching loop; every score distinct, and all equal."""
    rng = np.random.default_rng(1)
    for equal_scores in (False, True):
        groups = []
        for n in SIZES:
            s = np.full(n, 0.5) if equal_scores else np.round(rng.permutation(n) / 256 + 0.125, 5)
            groups.append(np.stack([s, 30.0 * np.arange(n), 7.0 * np.arange(n), np.full(n, 20.0), np.full(n, 6.0)], axis=1))
        ref = check(groups, [2.0] * len(SIZES), method, 0.5)
        assert ref[1].tolist() == list(SIZES)


@pytest.mark.parametrize('method', METHODS)
def test_identical_boxes_make_one_cluster_of_n(method):
    rng = np.random.default_rng(2)
    groups = [np.concatenate([np.round(rng.uniform(0.05, 1, (n, 1)), 5), np.tile([[12.5, 40.25, 100.0, 61.5]], (n, 1))], axis=1) for n in SIZES]
    ref = check(groups, [3.0] * len(SIZES), method, 0.5)
    assert ref[1].tolist() == [min(n, 1) for n in SIZES]
    assert [int(ref[2][o]) for o, n in zip(np.cumsum((0,) + SIZES[:-1]).tolist(), SIZES) if n] == [n for n in SIZES if n]


def _crowd(rng, n):
    """n rows around n // 3 objects on a small canvas: clusters of several members, many clusters."""
    k = max(1, n // 3)
    cx, cy = rng.uniform(0, 900, k), rng.uniform(0, 600, k)
    w, h = rng.uniform(20, 80, k), rng.uniform(20, 80, k)
    o = rng.integers(0, k, n)
    return np.stack([np.round(rng.uniform(0.05, 1, n), 5), cx[o] + rng.normal(0, 2, n), cy[o] + rng.normal(0, 2, n),
                     np.maximum(w[o] + rng.normal(0, 2, n), 1), np.maximum(h[o] + rng.normal(0, 2, n), 1)], axis=1)


@pytest.mark.parametrize('method', METHODS)
def test_groups_at_and_over_the_lds_capacity(method):
    """cap rows: the LDS instance with every array full; cap + 1: the global-memory instance (a small group rides along in each
    call, so both instances also see a group far below the capacity)."""
    from waymo_2d_tracking_amd import _lib
    lib = _lib.lib()
    lib.wt_fuse_groups_lds_rows.restype = C.c_int64
    lib.wt_fuse_groups_workspace.restype = C.c_size_t
    cap = int(lib.wt_fuse_groups_lds_rows())
    assert cap == (64 * 1024) // (15 * 8 + 4 * 4)
    assert lib.wt_fuse_groups_workspace(C.c_int64(10 * cap), C.c_int64(10), C.c_int64(cap)) == 0
    assert lib.wt_fuse_groups_workspace(C.c_int64(cap + 6), C.c_int64(2), C.c_int64(cap + 1)) >= (cap + 6) * 136
    rng = np.random.default_rng(3)
    for n in (cap, cap + 1):
        ref = check([_crowd(rng, 5), _crowd(rng, n)], [2.0, 3.0], method, 0.5)
        assert 64 < ref[1][1] < n and ref[2].max() > 3


@pytest.mark.parametrize('method', METHODS)
def test_mix_of_empty_and_filled_groups_with_different_wsum(method):
    rng = np.random.default_rng(4)
    sizes = [0, 0, 7, 0, 1, 30, 0, 2, 0, 0, 11, 0]
    ref = check([_crowd(rng, n) for n in sizes], [1.0 + (g % 4) for g in range(len(sizes))], method, 0.4)
    assert [int(c > 0) for c in ref[1]] == [int(n > 0) for n in sizes]


@pytest.fixture(scope='module')
def random_groups():
    return R.random_groups(7)


@pytest.mark.parametrize('thr', [0.3, 0.5, 0.7])
@pytest.mark.parametrize('method', METHODS)
def test_200_random_groups(random_groups, method, thr):
    dets5, offsets, wsum = random_groups
    ref = R.fuse_groups(dets5, offsets, wsum, method, thr)
    m = [int(ref[2][o + j]) for o, c in zip(offsets[:-1].tolist(), ref[1].tolist()) for j in range(c)]
    print('%s thr %s: %d rows, %d clusters, %d with more than one member, %d with more than 3' % (method, thr, len(dets5), len(m), sum(v > 1 for v in m), sum(v > 3 for v in m)))
    assert sum(v > 1 for v in m) >= 0.3 * len(m) and max(m) > 3           # 3 inputs: some cluster holds two objects' rows
    assert_equal(run_host(dets5, offsets, wsum, method, thr), ref, offsets)


def _dev_call(lib, torch, t, n_rows, n_groups, max_rows, method, thr, ws, ws_bytes, stream, members=True):
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    return lib.wt_fuse_groups_dev(p(t['dets5']), p(t['offsets']), p(t['wsum']), C.c_int64(n_rows), C.c_int64(n_groups), C.c_int64(max_rows),
                                  C.c_int(method), C.c_double(thr), p(t['out5']), p(t['members'] if members else None),
                                  p(t['row_cluster'] if members else None), p(t['counts']), p(ws), C.c_size_t(ws_bytes),
                                  C.c_void_p(stream.cuda_stream if stream is not None else 0))


def _tensors(torch, dets5, offsets, wsum):
    dev = torch.device('cuda', 0)
    n = max(1, len(dets5))
    return dict(dets5=torch.from_numpy(dets5).to(dev) if len(dets5) else torch.zeros((1, 5), dtype=torch.float64, device=dev),
                offsets=torch.from_numpy(offsets).to(dev), wsum=torch.from_numpy(wsum).to(dev),
                out5=torch.zeros((n, 5), dtype=torch.float64, device=dev), members=torch.zeros(n, dtype=torch.int32, device=dev),
                row_cluster=torch.zeros(n, dtype=torch.int32, device=dev), counts=torch.zeros(len(offsets) - 1, dtype=torch.int64, device=dev))


@pytest.mark.parametrize('big', [False, True])
def test_dev_on_a_side_stream_with_a_caller_owned_workspace(big):
    import torch
    from waymo_2d_tracking_amd import _lib
    lib = _lib.lib()
    lib.wt_fuse_groups_lds_rows.restype = C.c_int64
    cap = int(lib.wt_fuse_groups_lds_rows())
    rng = np.random.default_rng(5)
    sizes = [9, 0, cap + 40 if big else 70, 25]
    dets5, offsets, wsum = pack([_crowd(rng, n) for n in sizes], [2.0, 1.0, 3.0, 2.0])
    ws_bytes = int(lib.wt_fuse_groups_workspace(C.c_int64(len(dets5)), C.c_int64(len(sizes)), C.c_int64(max(sizes))))
    assert (ws_bytes > 0) == big
    t = _tensors(torch, dets5, offsets, wsum)
    ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device='cuda:0')
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    for mi, method in enumerate(METHODS):
        rc = _dev_call(lib, torch, t, len(dets5), len(sizes), max(sizes), mi, 0.5, ws, ws_bytes, stream)
        _lib.check(rc, 'wt_fuse_groups_dev')
        stream.synchronize()
        got = (t['out5'].cpu().numpy(), t['counts'].cpu().numpy(), t['members'].cpu().numpy(), t['row_cluster'].cpu().numpy())
        assert_equal(got, R.fuse_groups(dets5, offsets, wsum, method, 0.5), offsets)
    # out_members / row_cluster may be NULL
    t['out5'].zero_(); t['counts'].zero_()
    torch.cuda.synchronize()
    _lib.check(_dev_call(lib, torch, t, len(dets5), len(sizes), max(sizes), 0, 0.5, ws, ws_bytes, stream, members=False), 'wt_fuse_groups_dev')
    stream.synchronize()
    ref = R.fuse_groups(dets5, offsets, wsum, 'weighted_fusion', 0.5)
    assert np.array_equal(t['counts'].cpu().numpy(), ref[1])
    out5 = t['out5'].cpu().numpy()
    for o, c in zip(offsets[:-1].tolist(), ref[1].tolist()):
        assert np.array_equal(out5[o:o + c], ref[0][o:o + c])


def test_a_group_larger_than_max_group_rows_is_reported_not_run():
    import torch
    from waymo_2d_tracking_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(6)
    dets5, offsets, wsum = pack([_crowd(rng, 5), _crowd(rng, 40)])
    t = _tensors(torch, dets5, offsets, wsum)
    _lib.check(_dev_call(lib, torch, t, len(dets5), 2, 8, 0, 0.5, None, 0, None), 'wt_fuse_groups_dev')       # LDS sized for 8 rows
    torch.cuda.synchronize()
    counts = t['counts'].cpu().numpy()
    assert counts[1] == -1 and counts[0] == R.fuse_groups(dets5, offsets, wsum, 0, 0.5)[1][0]


def test_error_returns():
    import torch
    from waymo_2d_tracking_amd import _lib
    lib = _lib.lib()
    lib.wt_fuse_groups_lds_rows.restype = C.c_int64
    lib.wt_fuse_groups_workspace.restype = C.c_size_t
    cap = int(lib.wt_fuse_groups_lds_rows())
    rng = np.random.default_rng(8)
    dets5, offsets, wsum = pack([_crowd(rng, 6), _crowd(rng, 4)])
    t = _tensors(torch, dets5, offsets, wsum)
    ws = torch.zeros(1024, dtype=torch.uint8, device='cuda:0')
    INVALID = 1

    def message():
        return lib.wt_last_error().decode()
    for method in (-1, 2, 16):
        assert _dev_call(lib, torch, t, 10, 2, 6, method, 0.5, None, 0, None) == INVALID and 'method' in message()
    for n_rows, n_groups, max_rows in ((-1, 2, 6), (10, -2, 6), (10, 2, -6)):
        assert _dev_call(lib, torch, t, n_rows, n_groups, max_rows, 0, 0.5, None, 0, None) == INVALID and 'negative' in message()
    # a group beyond the LDS capacity needs the workspace: none, and one that is too small
    need = int(lib.wt_fuse_groups_workspace(C.c_int64(10), C.c_int64(2), C.c_int64(cap + 1)))
    assert need > 1024
    assert _dev_call(lib, torch, t, 10, 2, cap + 1, 0, 0.5, None, 0, None) == INVALID and 'workspace' in message()
    assert _dev_call(lib, torch, t, 10, 2, cap + 1, 0, 0.5, ws, 1024, None) == INVALID and 'workspace' in message()
    assert lib.wt_fuse_groups_workspace(C.c_int64(-1), C.c_int64(2), C.c_int64(6)) == 0
    out5, counts = np.zeros((10, 5)), np.zeros(2, np.int64)
    host = lambda off, method: lib.wt_fuse_groups_host(_lib.ptr(dets5), _lib.ptr(off), _lib.ptr(wsum), C.c_int64(2), C.c_int(method), C.c_double(0.5),
                                                       _lib.ptr(out5), None, None, _lib.ptr(counts))
    assert host(offsets, 3) == INVALID and 'method' in message()
    assert host(np.asarray([0, 7, 5], np.int64), 0) == INVALID and 'non-decreasing' in message()
    assert lib.wt_fuse_groups_host(_lib.ptr(dets5), _lib.ptr(offsets), _lib.ptr(wsum), C.c_int64(-1), C.c_int(0), C.c_double(0.5),
                                   _lib.ptr(out5), None, None, _lib.ptr(counts)) == INVALID and 'negative' in message()
    torch.cuda.synchronize()
    # nothing above ran a kernel or broke the library: a valid call still works (members / row_cluster NULL on the host path)
    assert host(offsets, 0) == 0
    ref = R.fuse_groups(dets5, offsets, wsum, 0, 0.5)
    assert np.array_equal(counts, ref[1]) and np.array_equal(out5[:ref[1][0]], ref[0][:ref[1][0]])


def _inputs(tmp_path):
    from waymo_2d_tracking_amd import synthetic as syn
    subs = syn.ensemble_inputs_json(5, n_images=5, k_inputs=3, n_objects=30)
    subs[2] = [r for r in subs[2] if r['image_id'] != subs[0][0]['image_id']]
    paths = []
    for k, rows in enumerate(subs):
        paths.append(str(tmp_path / ('in%d.json' % k)))
        with open(paths[-1], 'w') as fp:
            json.dump(rows, fp)
    return subs, paths


@pytest.mark.parametrize('method', METHODS)
def test_cli_end_to_end_equals_the_host_path_on_the_restatement(tmp_path, method):
    from waymo_2d_tracking_amd.detnet import ensemble_b as EB
    subs, paths = _inputs(tmp_path)
    EB.main(paths + ['-o', str(tmp_path / 'gpu.json'), '-m', method, '--iou-thresh', '0.55'])
    EB.main(paths + ['-o', str(tmp_path / 'ref.json'), '-m', method, '--iou-thresh', '0.55'], merge_fn=R.merge_fn)
    assert (tmp_path / 'gpu.json').read_bytes() == (tmp_path / 'ref.json').read_bytes()
    rows = json.load(open(tmp_path / 'gpu.json'))
    assert rows == R.ensemble_rows(subs, method, 0.55) and len(rows) > 30
    assert any(isinstance(v, float) and v != int(v) for r in rows for v in r['bbox'])        # boxes are not truncated


def test_sweep_takes_the_new_methods_next_to_the_old(tmp_path):
    from waymo_2d_tracking_amd.detnet import ensemble_b as EB, evaluate as E
    subs, paths = _inputs(tmp_path)
    ids = sorted(set(r['image_id'] for r in subs[0]))
    annotations = {'images': [{'id': k, 'width': 1920, 'height': 1280} for k in ids],
                   'categories': [{'id': 1, 'name': 'vehicle'}, {'id': 2, 'name': 'pedestrian'}, {'id': 3, 'name': 'sign'}, {'id': 4, 'name': 'cyclist'}],
                   'annotations': [{'image_id': r['image_id'], 'category_id': r['category_id'], 'bbox': r['bbox']} for i, r in enumerate(subs[0]) if i % 5]}
    gt = E.pack_ground_truth(annotations)
    grid = {'method': ['soft_nms', 'weighted_fusion_b', 'nmw'], 'iou_thresh': [0.5, 0.6, 0.7], 'soft_nms_cut': [0.9, 1.0], 'min_score': [0.0, 0.3]}
    res = E.sweep(paths, gt, grid)
    old = E.sweep(paths, gt, dict(grid, method=['soft_nms']))
    assert len(old.settings) == 12 and res.settings[:12] == old.settings
    assert res.settings[12:] == [{'method': m, 'iou_thresh': v, 'soft_nms_cut': None, 'min_score': None}
                                 for m in ('weighted_fusion_b', 'nmw') for v in (0.5, 0.6, 0.7)]
    for i in range(12):
        assert np.array_equal(res.results[i].ap, old.results[i].ap) and np.array_equal(res.results[i].tp, old.results[i].tp)
    assert res.mean_ap[:12] == old.mean_ap and sorted(res.ranked) == list(range(18))
    # a new setting's score is the score of the file the ensemble_b command line of flag_line writes
    for i in (12, 16):
        tail = E.flag_line(res.settings[i])
        assert tail == '-m %s --iou-thresh=%r' % ('weighted_fusion' if i == 12 else 'nmw', res.settings[i]['iou_thresh'])
        out = tmp_path / ('out%d.json' % i)
        EB.main(paths + ['-o', str(out)] + shlex.split(tail))
        scored = E.evaluate_detection_sets(gt, [str(out)])[0]
        assert np.array_equal(scored.ap, res.results[i].ap) and scored.mean_ap() == res.mean_ap[i] and res.mean_ap[i] > 0.3
    with pytest.raises(ValueError):
        E.sweep(paths, gt, dict(grid, method=['wbf']))
