"""Exact-answer tests of the ensemble's linear soft-NMS (csrc/ensemble.hip) on the adversarial cases of tests/softnms_cases.py: geometry that
turns an IoU into NaN (zero, underflowing, overflowing, cancelling and non-finite areas) at the top, in the middle and at the bottom of
the ranking, exact decay chains, every group size at which the dependency-free kernel changes shape or hands over to the serial one,
x-sorted chunks and the interval skip, score ties, the edges of the launch condition and a launch that mixes all of it.  Every case goes
through wt_ensemble_groups_host and wt_ensemble_groups_dev; every expectation is proven on the CPU by tests/test_softnms_cases.py; every
comparison is exact (no tolerance anywhere, NaN equals NaN, -0.0 differs from 0.0)."""
import ctypes as C

import numpy as np
import pytest
import torch

import softnms_cases as S
from waymo_2d_tracking_amd import _lib

pytestmark = pytest.mark.gpu

WT_OK, WT_ERR_CAPACITY = 0, 4
UNWRITTEN = -777.0                   # output rows are pre-filled with this: a kept row the kernel never wrote shows


def _run_host(case, method, sizes=None, k_inputs=1):
    G = len(case.offsets) - 1
    out = np.full((len(case.rows) + 1, 5), UNWRITTEN)
    cnt = np.full(G + 1, -1, dtype=np.int64)
    _lib.check(_lib.lib().wt_ensemble_groups_host(_lib.ptr(case.rows), _lib.ptr(case.offsets), _lib.ptr(sizes), C.c_int64(G), C.c_int(k_inputs),
                                                  C.c_int(method), C.c_double(case.thr), C.c_double(case.cut), _lib.ptr(out), _lib.ptr(cnt)),
               'wt_ensemble_groups_host')
    return out[:len(case.rows)], cnt[:G]


def _tp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _run_dev(case, method, sizes=None, k_inputs=1, with_workspace=True):
    """wt_ensemble_groups_dev on the default stream -> (status, rows, counts, workspace bytes the library asked for)."""
    lib = _lib.lib()
    n, G = len(case.rows), len(case.offsets) - 1
    max_rows = int(np.diff(case.offsets).max()) if G else 0
    need = int(lib.wt_ensemble_groups_workspace(C.c_int64(n), C.c_int64(G), C.c_int64(max_rows)))
    d_in = torch.from_numpy(np.ascontiguousarray(np.concatenate([case.rows, np.zeros((1, 5))]))).cuda()
    d_off = torch.from_numpy(np.array(case.offsets)).cuda()
    d_sz = None if sizes is None else torch.from_numpy(np.ascontiguousarray(sizes)).cuda()
    d_out = torch.full((n + 1, 5), UNWRITTEN, dtype=torch.float64, device='cuda')
    d_cnt = torch.full((G + 1,), -1, dtype=torch.int64, device='cuda')
    ws = torch.empty(need, dtype=torch.uint8, device='cuda') if (with_workspace and need) else None
    torch.cuda.synchronize()
    rc = lib.wt_ensemble_groups_dev(_tp(d_in), _tp(d_off), _tp(d_sz), C.c_int64(n), C.c_int64(G), C.c_int64(max_rows), C.c_int(k_inputs),
                                    C.c_int(method), C.c_double(case.thr), C.c_double(case.cut), _tp(d_out), _tp(d_cnt), _tp(ws),
                                    C.c_size_t(need if ws is not None else 0), None)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy()[:n], d_cnt.cpu().numpy()[:G], need


def _assert_exact(what, case, rows, counts, exp_rows=None, exp_counts=None):
    exp_rows = case.exp_rows if exp_rows is None else exp_rows
    exp_counts = case.exp_counts if exp_counts is None else exp_counts
    assert np.array_equal(counts, exp_counts), '%s: counts %s, expected %s' % (what, counts.tolist()[:40], exp_counts.tolist()[:40])
    for g in range(len(exp_counts)):
        a, b = int(case.offsets[g]), int(case.offsets[g]) + int(exp_counts[g])
        if not np.array_equal(rows[a:b], exp_rows[a:b], equal_nan=True):
            bad = np.nonzero(~((rows[a:b] == exp_rows[a:b]) | (np.isnan(rows[a:b]) & np.isnan(exp_rows[a:b]))).all(axis=1))[0]
            raise AssertionError('%s: group %d: %d of %d rows differ, first at rank %d: got %r, expected %r'
                                 % (what, g, bad.size, b - a, bad[0], rows[a + bad[0]].tolist(), exp_rows[a + bad[0]].tolist()))
        assert S.same_bits(rows[a:b], exp_rows[a:b]), '%s: group %d: a zero has the wrong sign' % (what, g)


def _method(case, mth=2):
    return mth | (16 if case.centre else 0)


@pytest.mark.parametrize('name', list(S.CASES))
def test_host_form(name):
    case = S.get(name)
    rows, counts = _run_host(case, _method(case))
    _assert_exact(name, case, rows, counts)


@pytest.mark.parametrize('name', list(S.CASES))
def test_device_form(name):
    """With the workspace the library asks for, and - where it asks for one - also without: the call then either reports
    WT_ERR_CAPACITY or (the groups still fit the LDS form of this method) is exact."""
    case = S.get(name)
    rc, rows, counts, need = _run_dev(case, _method(case))
    assert rc == WT_OK, _lib.lib().wt_last_error()
    _assert_exact(name, case, rows, counts)
    if need:
        rc, rows, counts, _ = _run_dev(case, _method(case), with_workspace=False)
        assert rc in (WT_OK, WT_ERR_CAPACITY), rc
        print('%s: %d workspace bytes asked for; without them: status %d' % (name, need, rc))
        if rc == WT_OK:
            _assert_exact(name + ' without workspace', case, rows, counts)


def test_sizes_beyond_the_lds_ask_for_a_workspace():
    """The with / without-workspace legs of test_device_form are not vacuous: the largest sizes need one, a small group does not."""
    lib = _lib.lib()
    assert lib.wt_ensemble_groups_workspace(C.c_int64(2048), C.c_int64(1), C.c_int64(2048)) > 0
    assert lib.wt_ensemble_groups_workspace(C.c_int64(600), C.c_int64(1), C.c_int64(600)) > 0
    assert lib.wt_ensemble_groups_workspace(C.c_int64(257), C.c_int64(1), C.c_int64(257)) == 0
    rc, rows, counts, need = _run_dev(S.get('pairs_2049'), 2, with_workspace=False)
    assert need > 0 and rc == WT_ERR_CAPACITY


def test_mixed_launch_groups_equal_their_results_alone():
    case = S.get('mixed_launch')
    rows, counts = _run_host(case, 2)
    _assert_exact('mixed', case, rows, counts)
    for g, alone in enumerate(S.single_groups(case)):
        r1, c1 = _run_host(alone, 2)
        a = int(case.offsets[g])
        assert c1[0] == counts[g], g
        assert S.same_bits(r1[:c1[0]], rows[a:a + c1[0]]), g
    # the same groups in reverse order: every group lands on another block and next to other neighbours
    G = len(counts)
    rev = S.make_case([case.rows[case.offsets[g]:case.offsets[g + 1]] for g in reversed(range(G))], case.thr, case.cut)
    rows_r, counts_r = _run_host(rev, 2)
    _assert_exact('mixed reversed', rev, rows_r, counts_r)
    assert counts_r.tolist() == counts.tolist()[::-1]


@pytest.mark.parametrize('mth', [0, 1])
@pytest.mark.parametrize('name', S.BAD_GEOMETRY)
def test_fusion_and_hard_nms_on_the_same_geometry(name, mth, oracle):
    """Weighted fusion (the group's rows split into two inputs) and hard NMS on the non-finite and non-positive geometry, against the C oracle."""
    case = S.get(name)
    sizes = S.input_sizes(case, 2)
    exp_rows, exp_counts = S.oracle_expected(oracle, case, mth, 2)
    rows, counts = _run_host(case, _method(case, mth), sizes, 2)
    _assert_exact('%s method %d host' % (name, mth), case, rows, counts, exp_rows, exp_counts)
    rc, rows, counts, _ = _run_dev(case, _method(case, mth), sizes, 2)
    assert rc == WT_OK
    _assert_exact('%s method %d dev' % (name, mth), case, rows, counts, exp_rows, exp_counts)
