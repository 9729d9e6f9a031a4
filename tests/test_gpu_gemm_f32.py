"""Exact-answer tests of the f32 MFMA GEMM (csrc/det_gemm.hip: wd_gemm_nt_f32, wd_gemm_nt_ws_f32 through the C ABI) on the integer operands
of tests/gemm_cases.py: every partial sum is an integer below 2^24, so every kernel, slice count and summation order - the atomics of the
v1 split included - must give the integer product bit for bit.  One shape per branch of the launch rules (restated in gemm_cases.py and
proved self-consistent on the CPU by tests/test_gemm_cases.py), each run twice with bit-equal results; outputs and workspaces start out as
NaN.  One float case per kernel against float64 with the derivable bound gamma_n (|A| |B|^T + |bias| + |residual|)."""
import ctypes as C
import functools

import pytest
import torch

import gemm_cases as GC
from waymo_2d_tracking_amd import _lib
from waymo_2d_tracking_amd.detnet.nn import ops

pytestmark = pytest.mark.gpu

WT_ERR_INVALID, WT_ERR_CAPACITY = 1, 4
GUARD = 64


@functools.lru_cache(maxsize=2)
def _operands(m, n, k):
    return GC.operands(m, n, k, device='cuda')


def _out(m, n):
    return torch.full((m * n + GUARD,), float('nan'), dtype=torch.float32, device='cuda')


def _v1(a, bt, bias, res, relu, m, n, k, out, a_off=0):
    rc = _lib.lib().wd_gemm_nt_f32(C.c_void_p(a.data_ptr() + a_off), ops._p(bt), ops._p(bias), ops._p(res), C.c_int(int(relu)), C.c_int(m),
                                   C.c_int(n), C.c_int(k), ops._p(out), ops._stream())
    torch.cuda.synchronize()
    return rc


def _ws(a, bt, bias, res, relu, m, n, k, out, ws, ws_bytes, ws_off=0):
    rc = _lib.lib().wd_gemm_nt_ws_f32(ops._p(a), ops._p(bt), ops._p(bias), ops._p(res), C.c_int(int(relu)), C.c_int(m), C.c_int(n), C.c_int(k),
                                      ops._p(out), None if ws is None else C.c_void_p(ws.data_ptr() + ws_off), C.c_size_t(ws_bytes),
                                      ops._stream())
    torch.cuda.synchronize()
    return rc


def _workspace(m, n, k):
    """The v2 plan of the restatement against the library's, then a NaN-filled workspace of exactly that size."""
    need = int(_lib.lib().wd_gemm_nt_workspace(C.c_int(m), C.c_int(n), C.c_int(k)))
    assert need == GC.v2_workspace(m, n, k), (m, n, k, need)
    return need, torch.full((max(need // 4, 4),), float('nan'), dtype=torch.float32, device='cuda')


def _exact(call, m, n, k, use_bias, use_res, relu):
    """One case, twice: the integer product with and without the epilogue terms, bit-equal runs, nothing written behind C."""
    a, bt, bias, res = _operands(m, n, k)
    bias, res = (bias if use_bias else None), (res if use_res else None)
    want = GC.exact_product(a, bt, bias, res, relu)
    runs = []
    for _ in range(2):
        out = _out(m, n)
        assert call(a, bt, bias, res, relu, m, n, k, out) == _lib.WT_OK, _lib.lib().wt_last_error()
        assert bool(torch.isnan(out[m * n:]).all())
        runs.append(out[:m * n].view(m, n))
    what = 'M=%d N=%d K=%d bias=%s residual=%s relu=%s' % (m, n, k, use_bias, use_res, relu)
    bad = torch.nonzero(~(runs[0].double() == want))
    assert bad.numel() == 0, '%s: %d wrong, first at %s: got %r, want %r' % (
        what, bad.shape[0], bad[0].tolist(), runs[0][tuple(bad[0].tolist())].item(), want[tuple(bad[0].tolist())].item())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), what + ': two runs differ'


@pytest.mark.parametrize('m,n,k,residual,plan', GC.V1_SHAPES)
def test_v1_exact(m, n, k, residual, plan):
    """wd_gemm_nt_f32.  gemm_nt_kernel<2,2> in one slice (ragged M, N and K: the `gm < M && gk < K` loads, the `col >= N` / `row >= M`
    stores, one to 64 slabs through the double buffer); in two atomic slices (hipMemsetAsync + atomicAdd, `s_end` of the short second
    slice, the last slab 4 wide, then wd_bias_relu_f32 in its four bias / ReLU forms - none, bias, ReLU, both); on either side of each limit
    that switches the split (N % 4, K >= 2048, 512 tiles, a residual); gemm_nt_kernel<4,4> from 192 tiles of 128 x 128 with ragged M, N, K."""
    assert GC.v1_plan(m, n, k, residual) == plan
    for use_bias in (False, True):
        for relu in (False, True):
            _exact(_v1, m, n, k, use_bias, residual, relu)


@pytest.mark.parametrize('m,n,k,slices,runs', GC.V2_SHAPES)
def test_v2_exact(m, n, k, slices, runs):
    """wd_gemm_nt_ws_f32.  gemm_nt_v2_kernel with 1, 2, 4 and 16 slices (`kz = block % splitk`), slices of unequal length with odd and even
    slab counts (the tail loop's `s + 1 < nslab` / `s + 2 < nslab` guards, the short last slice), a last tile with one valid row and four
    valid columns (row_off clamps the loads to the last row, `row < M && col < N` masks the stores) and gemm_reduce_kernel summing the
    slices; shapes the workspace rule refuses (`need == 0`) fall through to v1."""
    need, ws = _workspace(m, n, k)
    assert GC.v2_slices(m, n, k) == slices and (not slices or GC.slab_runs(k, slices) == runs)

    def call(a, bt, bias, res, relu, m, n, k, out):
        ws.fill_(float('nan'))
        return _ws(a, bt, bias, res, relu, m, n, k, out, ws if need else None, need)
    _exact(call, m, n, k, False, False, False)
    _exact(call, m, n, k, True, True, True)


@pytest.mark.parametrize('use_bias,use_res,relu', GC.EPILOGUES)
def test_v2_reduce_epilogues(use_bias, use_res, relu):
    """gemm_reduce_kernel: every bias / residual / ReLU combination on (257, 260, 1056) - `bias[i % n4]` with n4 = 65 columns of float4 (a
    width no power of two, so an index taken from another width shifts the bias), the residual at `i`, two slices summed in slice order."""
    m, n, k = 257, 260, 1056
    need, ws = _workspace(m, n, k)
    assert need == 2 * m * n * 4
    _exact(lambda a, bt, bias, res, relu, m, n, k, out: _ws(a, bt, bias, res, relu, m, n, k, out, ws, need), m, n, k, use_bias, use_res, relu)


def test_v2_refusals():
    """wd_gemm_nt_ws_f32 refuses a workspace one byte short, and one 4 bytes off a 16-byte boundary, with WT_ERR_CAPACITY before any launch
    (C keeps its NaN); a valid call afterwards is exact."""
    m, n, k = 256, 256, 1024
    a, bt, bias, res = _operands(m, n, k)
    need, _ = _workspace(m, n, k)
    ws = torch.full((need // 4 + 8,), float('nan'), dtype=torch.float32, device='cuda')
    out = _out(m, n)
    assert _ws(a, bt, bias, res, True, m, n, k, out, ws, need - 1) == WT_ERR_CAPACITY
    assert _ws(a, bt, bias, res, True, m, n, k, out, ws, need, ws_off=4) == WT_ERR_CAPACITY
    assert _ws(a, bt, bias, res, True, m, n, k, out, None, need) == WT_ERR_CAPACITY
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())
    _exact(lambda a, bt, bias, res, relu, m, n, k, out: _ws(a, bt, bias, res, relu, m, n, k, out, ws, need), m, n, k, True, True, True)


def test_v1_refusals():
    """wd_gemm_nt_f32 refuses K = 0, K = 6 and an A 4 bytes off a 16-byte boundary with WT_ERR_INVALID; M = 0 or N = 0 is WT_OK and writes
    nothing; a valid call afterwards is exact."""
    m, n, k = 64, 64, 64
    a, bt, bias, res = _operands(m, n, k)
    out = _out(m, n)
    assert _v1(a, bt, bias, res, True, m, n, 0, out) == WT_ERR_INVALID
    assert _v1(a, bt, bias, res, True, m, n, 6, out) == WT_ERR_INVALID
    assert _v1(a, bt, bias, res, True, m, n, k - 4, out, a_off=4) == WT_ERR_INVALID
    assert _v1(a, bt, bias, res, True, 0, n, k, out) == _lib.WT_OK
    assert _v1(a, bt, bias, res, True, m, 0, k, out) == _lib.WT_OK
    assert bool(torch.isnan(out).all())
    _exact(_v1, m, n, k, True, True, True)


@pytest.mark.parametrize('m,n,k', GC.FLOAT_SHAPES)
def test_float_within_the_derived_bound(m, n, k):
    """One float case per kernel - gemm_nt_kernel<2,2> in two atomic slices (130, 68, 2052), gemm_nt_kernel<4,4> (12200, 130, 68),
    gemm_nt_v2_kernel + gemm_reduce_kernel (257, 260, 1056) - against float64, elementwise within gamma_n (|A| |B|^T + |bias| + |residual|),
    n = 2 K + splitk + 3, u = 2^-24: derived from the operation count, not measured."""
    g = torch.Generator().manual_seed(m + n + k)
    a = torch.randn((m, k), generator=g).cuda()
    bt = (torch.randn((n, k), generator=g) / k ** 0.5).cuda()
    bias, res = torch.randn(n, generator=g).cuda(), torch.randn((m, n), generator=g).cuda()
    need, ws = _workspace(m, n, k)
    assert GC.v1_plan(m, n, k) + (GC.v2_slices(m, n, k),) == {130: ('2x2', 2, 0), 12200: ('4x4', 1, 0), 257: ('2x2', 1, 2)}[m]
    for use_res in (False, True):
        r = res if use_res else None
        splitk = GC.v2_slices(m, n, k) or GC.v1_plan(m, n, k, use_res)[1]
        out = _out(m, n)
        rc = _ws(a, bt, bias, r, False, m, n, k, out, ws, need) if need else _v1(a, bt, bias, r, False, m, n, k, out)
        assert rc == _lib.WT_OK
        got = out[:m * n].view(m, n).double()
        err = (got - GC.exact_product(a, bt, bias, r)).abs()
        bound = GC.float_bound(a, bt, bias, r, splitk)
        worst = float((err / bound).max())
        print('M=%d N=%d K=%d residual=%s splitk=%d: max err %.3e, max err / bound %.4f' % (m, n, k, use_res, splitk, float(err.max()), worst))
        assert bool((err <= bound).all()), worst
