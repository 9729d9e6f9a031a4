"""Op-level tests of the TRAINING BACKWARD kernels (csrc/det_deform_bwd.hip, csrc/det_backward.hip, the small passes of csrc/det_misc.hip) against
float64 autograd through the CPU restatements (oracle/detector_ref.py, oracle/backward_ref.py), at the shapes and edges where such kernels go
wrong: the column-slab form at 64 channels per group (and past its 65 536-block grid cap), several ragged tiles per workgroup in deform_dw, the
persistent loop of deform_dxoff, far samples that also leave the image, hundreds of samples on one input pixel, maps smaller than a tile, samples on
exact integers, zero offsets (= a grouped convolution), ROIAlign backward over a batch / all levels / odd channel counts / degenerate boxes / the
per-sample form / footprints above 192 cells / 512 overlapping ROIs, and the exact elementwise passes.

Every "this input takes that path" claim is an assertion on values computed from the inputs on the CPU or from the library's own size queries.

Inputs: offsets are odd multiples of 1/1024 (oracle/backward_ref.exact_offsets) - base + offset is then exact in float32, both sides see the same
bilinear cell and no sample sits on a kink - except in the integer-position test, which is about exactly that.

Bounds.  The project's own: deformable gradients max|a - b| / max|b| < 2e-4, ROIAlign gradients |a - b| < 1e-4 max|b| + 1e-6 (tests/test_gpu_detops.py).
For the cases with longer sums than any older test (C = 2048, maps of thousands of pixels, 512 overlapping ROIs) the test first evaluates the
REFERENCE ITSELF in float32 on the CPU against float64; the bound is max(project bound, 4 x that error).  Measured (profiles/backward_ops_error.txt,
max|a - b| / max|b|; ROIAlign rows: absolute error / max|b|):

    case                                  tensors            float32 reference            HIP kernels                  bound
    slab C=2048 2x44x44 s1 (grid cap)     dX / dOff / dW     2.3e-6 / 3.1e-6 / 2.3e-6     2.3e-7 / 2.1e-7 / 2.4e-6     2e-4
    slab C=2048 2x18x21 s2                dX / dOff / dW     4.5e-7 / 1.5e-6 / 5.3e-7     2.8e-7 / 2.0e-7 / 5.3e-7     2e-4
    fused C=1024 1x56x40 (cg 32)          dX / dOff / dW     2.0e-6 / 2.9e-6 / 2.0e-6     2.9e-7 / 2.1e-7 / 2.5e-7     2e-4
    fused C=512 1x56x56 (cg 16)           dX / dOff / dW     2.2e-6 / 3.2e-6 / 2.7e-6     2.6e-7 / 1.4e-7 / 2.6e-7     2e-4
    512 overlapping ROIs                  dp2 / dp3 / dp4    4.5e-7 / 2.6e-7 / 2.8e-7     1.9e-6 / 1.3e-6 / 9.3e-7     1e-4

4 x the float32 error of the reference stays far below the project bound in every such case, so the project bound is the bound everywhere; the
largest error of any case in the file is 5.9e-6 (ROIAlign, p2 of the 1920 x 1280 maps).

Inputs with the ReLU epilogue: see KINK_GUARD below.

Set WD_BACKWARD_ERROR_TABLE=<file> to have the module write the table of all measured errors when it finishes.
"""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEFORM_BOUND = 2e-4            # tests/test_gpu_detops.py::test_deform_conv_backward_vs_autograd_reference
# With the ReLU epilogue the output gradient is zeroed where the float64 pre-activation lies within 1e-4 of 0 (about 1e-4 of the outputs): a float32
# forward decides the mask of such an output by its rounding, and ONE flipped mask moves a dX entry by ~1e-2 of the tensor's maximum.  On the
# millions of outputs of the large cases a few such flips are certain; they say nothing about the backward kernels.
KINK_GUARD = 1e-4
STRIDES = [4, 8, 16, 32]
SCALES = [1.0 / s for s in STRIDES]
_ROWS = []


@pytest.fixture(scope='module', autouse=True)
def _error_table():
    yield
    path = os.environ.get('WD_BACKWARD_ERROR_TABLE')
    if path:
        with open(path, 'w') as f:
            f.write('%-78s %-8s %-12s %-12s %s\n' % ('case', 'tensor', 'f32 ref', 'HIP', 'bound'))
            for row in _ROWS:
                f.write('%-78s %-8s %-12s %-12.3e %.3e\n' % row)


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _ho(h, stride):
    return (h + 2 - 3) // stride + 1


def _deform_inputs(seed, n, c, h, w, stride, osc, groups=32):
    from oracle import backward_ref as B
    g = torch.Generator().manual_seed(seed)
    ho, wo = _ho(h, stride), _ho(w, stride)
    x = torch.randn((n, c, h, w), generator=g)
    offset = B.exact_offsets(torch.randn((n, 18, ho, wo), generator=g) * osc)
    weight = torch.randn((c, c // groups, 3, 3), generator=g) / (3 * (c // groups) ** 0.5)
    gy = torch.randn((n, c, ho, wo), generator=g)
    scale = torch.rand(c, generator=g) + 0.5
    bias = torch.randn(c, generator=g) * 0.2
    return x, offset, weight, gy, scale, bias


def _hip_deform(x, offset, weight, stride, gy, scale=None, bias=None, relu=False, groups=32):
    from waymo_2d_tracking_amd.detnet.nn import ops
    xg, og, wg = _cl(x).requires_grad_(), _cl(offset).requires_grad_(), weight.cuda().requires_grad_()
    if scale is None:
        yg = ops.DeformConvFn.apply(xg, og, wg, groups, stride, 1)
    else:
        yg = ops.DeformConvFn.apply(xg, og, wg, groups, stride, 1, scale.cuda(), bias.cuda(), relu)
    yg.backward(_cl(gy))
    torch.cuda.synchronize()
    return yg.detach().cpu(), xg.grad.cpu(), og.grad.cpu(), wg.grad.cpu()


def _compare_deform(case, got, ref, ref32=None, names=('dx', 'doffset', 'dw')):
    """got / ref / ref32: (y, dX, dOffset, dW).  Prints every figure, then asserts the bound of the module docstring."""
    from oracle import backward_ref as B
    assert B.rel_err(got[0], ref[0]) < DEFORM_BOUND, (case, 'y')
    failures = []
    for i, name in enumerate(('dx', 'doffset', 'dw')):
        if name not in names:
            continue
        assert got[i + 1].shape == ref[i + 1].shape and bool(torch.isfinite(got[i + 1]).all()), (case, name)
        err = B.rel_err(got[i + 1], ref[i + 1])
        e32 = B.rel_err(ref32[i + 1], ref[i + 1]) if ref32 is not None else None
        bound = max(DEFORM_BOUND, 4 * e32) if e32 is not None else DEFORM_BOUND
        _ROWS.append((case, name, '-' if e32 is None else '%.3e' % e32, err, bound))
        print('%s %s: f32 reference %s, HIP %.3e, bound %.3e' % (case, name, e32, err, bound))
        if not err < bound:
            failures.append((case, name, err, bound))
    assert not failures, failures


def _dw_slices(n, h, w, c, groups, stride):
    from waymo_2d_tracking_amd import _lib
    cg = c // groups
    floats = _lib.lib().wd_deform_dw_scratch_floats(C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(c), C.c_int(groups), C.c_int(stride))
    assert floats % (groups * 9 * cg * cg) == 0
    return floats // (groups * 9 * cg * cg)


def _ntiles(n, h, w, stride):
    return n * ((_ho(h, stride) + 7) // 8) * ((_ho(w, stride) + 7) // 8)


# ---------------------------------------------------------------------------------------------------------------------------------
# deformable convolution backward

@pytest.mark.parametrize('n,h,w,stride,epilogue', [(1, 17, 19, 1, False), (1, 17, 19, 1, True), (2, 18, 21, 2, False), (2, 18, 21, 2, True),
                                                   (2, 44, 44, 1, True)])
def test_deform_backward_column_slab_c2048(n, h, w, stride, epilogue):
    """res5: 64 channels per group, no fused kernel - wd_deform_im2col_f32, two library GEMMs, wd_deform_col2im_f32 (dOffset pass +
    deform_col2im_dx_gather_kernel<1 / 2>), edge tiles in both directions.  The 2 x 44 x 44 case needs more than the 65 536 blocks the two
    slab kernels are capped at, so their grid-stride loops run (asserted); it runs with the epilogue (ReLU mask + scale: wd_act_bwd_f32 in front)."""
    from oracle import backward_ref as B
    from waymo_2d_tracking_amd.detnet.nn import ops
    c = 2048
    assert not ops.fused_deform_backward_supported(c, c, 32, stride, 1)
    ho, wo = _ho(h, stride), _ho(w, stride)
    assert ho % 8 and wo % 8
    if h == 44:
        assert n * ho * wo * 9 * c // 4 > 65536 * 256
    x, offset, weight, gy, scale, bias = _deform_inputs(100 + h + stride, n, c, h, w, stride, 1.3)
    ep = dict(scale=scale, bias=bias, relu=True) if epilogue else {}
    ref = B.deform_grads(x, offset, weight, 32, stride, gy, kink_guard=KINK_GUARD, **ep)
    gy = ref[4] if epilogue else gy
    ref32 = B.deform_grads(x, offset, weight, 32, stride, gy, dtype=torch.float32, **ep)
    got = _hip_deform(x, offset, weight, stride, gy, **ep)
    _compare_deform('slab C=2048 %dx%dx%d s%d%s' % (n, h, w, stride, ' epilogue' if epilogue else ''), got, ref, ref32)


@pytest.mark.parametrize('epilogue', ['none', 'pass', 'fused'])
@pytest.mark.parametrize('c,h,w', [(1024, 56, 40), (512, 56, 56)])
def test_deform_backward_fused_many_tiles_per_workgroup(c, h, w, epilogue, monkeypatch):
    """Fused kernels on a map large enough that deform_dw_kernel walks several tiles per workgroup with a ragged last round, that
    deform_dw_reduce_kernel sums many slices, and that deform_dxoff_kernel's persistent loop takes many (tile, group) items per workgroup with
    table reloads in between - all asserted from the library's own size queries.  epilogue: none / the masking pass in front (wd_act_bwd_f32) /
    folded into the kernels' dY loads (WD_FUSED_DEFORM_EPILOGUE=1)."""
    from oracle import backward_ref as B
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.detnet.nn import ops
    monkeypatch.setenv('WD_FUSED_DEFORM_EPILOGUE', '1' if epilogue == 'fused' else '0')
    assert ops.fused_deform_backward_supported(c, c, 32, 1, 1) and ops.FUSED_DEFORM_DXOFF
    ntiles, slices = _ntiles(1, h, w, 1), _dw_slices(1, h, w, c, 32, 1)
    assert slices < ntiles and ntiles % slices != 0, (ntiles, slices)          # several tiles on one workgroup, the last round ragged
    assert slices > 8                                                          # a real reduction over slices
    cus = _lib.device_info()[2]
    assert ntiles * 32 > 2 * cus, (ntiles, cus)                                # more items than persistent workgroups
    x, offset, weight, gy, scale, bias = _deform_inputs(c + h, 1, c, h, w, 1, 1.3)
    ep = dict(scale=scale, bias=bias, relu=True) if epilogue != 'none' else {}
    ref = B.deform_grads(x, offset, weight, 32, 1, gy, kink_guard=KINK_GUARD, **ep)
    gy = ref[4] if ep else gy
    ref32 = B.deform_grads(x, offset, weight, 32, 1, gy, dtype=torch.float32, **ep)
    got = _hip_deform(x, offset, weight, 1, gy, **ep)
    _compare_deform('fused C=%d 1x%dx%d epilogue %s' % (c, h, w, epilogue), got, ref, ref32)


@pytest.mark.parametrize('c,stride,s2', [(512, 1, '0'), (1024, 1, '0'), (512, 2, '0'), (512, 2, '1'), (1024, 2, '0'), (1024, 2, '1')])
def test_deform_backward_far_and_outside_samples(c, stride, s2, monkeypatch):
    """Offsets of several pixels: a real share of the samples leaves the 14 x 14 patch of its tile (deform_bwd_far_kernel<16 / 32>, second
    pass of deform_dw_kernel; at stride 2 through the column-slab form [WD_FUSED_DEFORM_S2=0] and through the fused kernels [=1]) AND a real
    share has corners outside the image (both >= 5 %, computed from the offsets on the CPU; far samples with outside corners exist too)."""
    from oracle import backward_ref as B
    from waymo_2d_tracking_amd.detnet.nn import ops
    monkeypatch.setenv('WD_FUSED_DEFORM_S2', s2)
    assert ops.fused_deform_backward_supported(c, c, 32, stride, 1) == (stride == 1 or s2 == '1')
    n, h, w = (2, 13, 18) if stride == 1 else (2, 21, 27)
    x, offset, weight, gy, scale, bias = _deform_inputs(c + stride, n, c, h, w, stride, 4.0)
    shares = B.deform_sample_shares(offset, h, w, stride)
    print(shares)
    assert shares['far'] >= 0.05 and shares['outside'] >= 0.05 and shares['far_outside'] >= 0.01, shares
    ref = B.deform_grads(x, offset, weight, 32, stride, gy)
    got = _hip_deform(x, offset, weight, stride, gy)
    _compare_deform('far C=%d s%d S2=%s' % (c, stride, s2), got, ref)


@pytest.mark.parametrize('c', [512, 1024, 2048])
@pytest.mark.parametrize('mode', ['one_cell', 'two_cells'])
def test_deform_backward_convergent_offsets(c, mode):
    """Every sample of a tile aimed at one cell (or two): the inverted sampling lists of four (eight) patch pixels hold hundreds of entries - the
    histogram clamp at 63, the list padding and the list capacity of deform_bwd_tables_kernel, the LDS lists of the slab form's gather - while
    every second tile aims all its samples outside the image (all lists empty, dX of those tiles' patches stays zero)."""
    from oracle import backward_ref as B
    n, h, w = 2, 16, 24
    g = torch.Generator().manual_seed(c)
    x, _, weight, gy, _, _ = _deform_inputs(c, n, c, h, w, 1, 1.0)
    if mode == 'one_cell':
        offset = B.convergent_offsets(n, h, w, 1, [(3.0, 4.0), None], 0.9, g)
        want_list = 576
    else:
        offset = B.convergent_offsets(n, h, w, 1, [(3.0, 4.0), (6.0, 2.0), None], 0.9, g, per_tap=True)
        want_list = 128
    shares = B.deform_sample_shares(offset, h, w, 1)
    assert shares['max_list'] >= want_list and 0.2 < shares['counts'] < 0.8 and shares['far'] == 0.0, shares
    ref = B.deform_grads(x, offset, weight, 32, 1, gy)
    got = _hip_deform(x, offset, weight, 1, gy)
    _compare_deform('convergent %s C=%d' % (mode, c), got, ref)


@pytest.mark.parametrize('c', [512, 1024, 2048])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('h,w', [(1, 1), (1, 9), (7, 7), (8, 8), (9, 8), (17, 15)])
def test_deform_backward_small_and_odd_maps(h, w, stride, c, monkeypatch):
    """Maps smaller than one 8 x 8 tile, one row, exactly one tile, one row / column more, odd sizes at stride 2; batch 1 and 3."""
    from oracle import backward_ref as B
    from waymo_2d_tracking_amd.detnet.nn import ops
    for n in (1, 3):
        x, offset, weight, gy, _, _ = _deform_inputs(h * 100 + w + n, n, c, h, w, stride, 1.3)
        # a one-pixel axis is beyond grid_sample's align_corners mapping: the floor-cell restatement is the reference there (off integers the
        # two are the same function: tests/test_oracle_backward_ref.py)
        ref = B.deform_grads(x, offset, weight, 32, stride, gy, floor_rule=(h == 1 or w == 1))
        for s2 in (('0', '1') if stride == 2 and c != 2048 else ('0',)):        # stride 2: the column-slab form and the fused kernels
            monkeypatch.setenv('WD_FUSED_DEFORM_S2', s2)
            assert ops.fused_deform_backward_supported(c, c, 32, stride, 1) == (c != 2048 and (stride == 1 or s2 == '1'))
            got = _hip_deform(x, offset, weight, stride, gy)
            _compare_deform('small C=%d %dx%dx%d s%d S2=%s' % (c, n, h, w, stride, s2), got, ref)


@pytest.mark.parametrize('c,stride', [(512, 1), (1024, 1), (2048, 1), (2048, 2)])
def test_deform_backward_integer_positions(c, stride):
    """Offsets that are exact integers (0 included): a corner weight is exactly 0 and the kernels drop that corner from their lists.  dX and dW
    are continuous there and are compared with the grid_sample reference as everywhere else.  dOffset is a one-sided derivative at such a point,
    and grid_sample's autograd is NOT on the kernels' side everywhere (its round trip through [-1, 1] can land an ulp below the integer, and it
    counts a sample at exactly -1 that detectron2's open interval drops - pinned on the CPU by
    tests/test_oracle_backward_ref.py::test_grid_sample_and_floor_rule_restatements_agree_off_integers_and_differ_on_them), so dOffset - and dX
    and dW a second time - are compared with the float64 floor-cell restatement oracle/detops_ref.deform_conv3x3 (cell = floor, as make_tap /
    fb_entry take it)."""
    from oracle import backward_ref as B
    n, h, w = 2, 12, 13
    g = torch.Generator().manual_seed(c + stride)
    x, _, weight, gy, _, _ = _deform_inputs(c + 7, n, c, h, w, stride, 1.0)
    offset = torch.randint(-3, 4, (n, 18, _ho(h, stride), _ho(w, stride)), generator=g).float()
    assert float((offset == 0).float().mean()) > 0.05
    got = _hip_deform(x, offset, weight, stride, gy)
    _compare_deform('integer C=%d s%d (grid_sample)' % (c, stride), got, B.deform_grads(x, offset, weight, 32, stride, gy), names=('dx', 'dw'))
    _compare_deform('integer C=%d s%d (floor rule)' % (c, stride), got, B.deform_grads(x, offset, weight, 32, stride, gy, floor_rule=True))


@pytest.mark.parametrize('c', [512, 1024, 2048])
@pytest.mark.parametrize('stride', [1, 2])
def test_deform_backward_zero_offsets_equal_grouped_conv_backward(c, stride):
    """Zero offsets: dX and dW are those of a grouped 3 x 3 convolution (torch conv2d backward in float64, an independent reference); dOffset
    against the floor-cell restatement (every position is an integer)."""
    from oracle import backward_ref as B
    n, h, w = 2, 11, 14
    x, _, weight, gy, _, _ = _deform_inputs(c + stride, n, c, h, w, stride, 1.0)
    offset = torch.zeros((n, 18, _ho(h, stride), _ho(w, stride)))
    got = _hip_deform(x, offset, weight, stride, gy)
    xr, wr = x.double().requires_grad_(), weight.double().requires_grad_()
    yr = torch.nn.functional.conv2d(xr, wr, None, stride, 1, 1, 32)
    yr.backward(gy.double())
    _compare_deform('zero offsets C=%d s%d (conv2d)' % (c, stride), got, (yr.detach(), xr.grad, None, wr.grad), names=('dx', 'dw'))
    _compare_deform('zero offsets C=%d s%d (floor rule)' % (c, stride), got, B.deform_grads(x, offset, weight, 32, stride, gy, floor_rule=True))


def test_deform_im2col_direct():
    """ops.deform_im2col alone: col[group][pixel][tap][channel] == the bilinear samples of the reference."""
    from oracle import backward_ref as B
    from waymo_2d_tracking_amd.detnet.nn import ops
    n, c, h, w, stride = 2, 256, 11, 14, 2
    x, offset, _, _, _, _ = _deform_inputs(1, n, c, h, w, stride, 2.0, groups=4)
    col = ops.deform_im2col(_cl(x), _cl(offset), stride, 1, 4).cpu()
    ref = B.deform_columns(x, offset, stride)                                   # (N, C, 9, Ho, Wo)
    ho, wo = _ho(h, stride), _ho(w, stride)
    ref = ref.view(n, 4, c // 4, 9, ho * wo).permute(1, 0, 4, 3, 2).reshape(4, n * ho * wo, 9, c // 4)
    assert col.shape == ref.shape
    assert B.rel_err(col, ref) < 1e-5


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_deform_col2im_direct(stride):
    """ops.deform_col2im alone on a random dcol slab: dX and dOffset == autograd of <col, dcol> through the reference columns.  Stride 3 takes the
    one-kernel scatter form (deform_col2im_kernel<true>), 1 and 2 the gather kernels."""
    from oracle import backward_ref as B
    from waymo_2d_tracking_amd.detnet.nn import ops
    n, c, h, w, groups = 2, 256, 13, 19, 4
    x, offset, _, _, _, _ = _deform_inputs(2 + stride, n, c, h, w, stride, 2.0, groups=groups)
    ho, wo = _ho(h, stride), _ho(w, stride)
    g = torch.Generator().manual_seed(3)
    dcol = torch.randn((groups, n * ho * wo, 9, c // groups), generator=g)
    dx, doff = ops.deform_col2im(dcol.cuda(), _cl(x), _cl(offset), stride, 1, groups)
    xr, orf = x.double().requires_grad_(), offset.double().requires_grad_()
    col = B.deform_columns(xr, orf, stride).view(n, groups, c // groups, 9, ho * wo).permute(1, 0, 4, 3, 2).reshape(dcol.shape)
    (col * dcol.double()).sum().backward()
    for name, a, b in (('dx', dx, xr.grad), ('doffset', doff, orf.grad)):
        err = B.rel_err(a.cpu(), b)
        _ROWS.append(('col2im direct s%d' % stride, name, '-', err, DEFORM_BOUND))
        assert err < DEFORM_BOUND, (name, err)


@pytest.mark.parametrize('c,stride', [(512, 1), (1024, 1), (512, 2)])
def test_deform_dw_and_dxoff_direct(c, stride):
    """ops.deform_dw and ops.deform_dxoff called on their own (with the epilogue arguments y_act / scale they take in the fused-epilogue
    configuration), so that a failure names the kernel."""
    from oracle import backward_ref as B
    from waymo_2d_tracking_amd.detnet.nn import ops
    n, h, w = 2, 19, 22
    x, offset, weight, gy, scale, bias = _deform_inputs(c + 3 * stride, n, c, h, w, stride, 2.0)
    ref = B.deform_grads(x, offset, weight, 32, stride, gy, scale=scale, bias=bias, relu=True)
    y_act = _cl(ref[0].float())                                                # the kernels only look at its sign
    dyn = _cl(gy).permute(0, 2, 3, 1).contiguous()
    dw = ops.deform_dw(_cl(x), _cl(offset), dyn, 32, y_act, scale.cuda(), stride)
    assert B.rel_err(dw.cpu(), ref[3]) < DEFORM_BOUND, 'deform_dw'
    dx, doff = ops.deform_dxoff(_cl(x), _cl(offset), dyn, weight.cuda(), 32, y_act, scale.cuda(), stride)
    assert B.rel_err(dx.cpu(), ref[1]) < DEFORM_BOUND, 'deform_dxoff dx'
    assert B.rel_err(doff.cpu(), ref[2]) < DEFORM_BOUND, 'deform_dxoff doffset'
    ref = B.deform_grads(x, offset, weight, 32, stride, gy)                     # and without the epilogue arguments
    dw = ops.deform_dw(_cl(x), _cl(offset), dyn, 32, None, None, stride)
    dx, doff = ops.deform_dxoff(_cl(x), _cl(offset), dyn, weight.cuda(), 32, None, None, stride)
    for name, a, b in (('dw', dw, ref[3]), ('dx', dx, ref[1]), ('doffset', doff, ref[2])):
        assert B.rel_err(a.cpu(), b) < DEFORM_BOUND, name


def test_deform_backward_argument_errors_are_refused_on_the_host():
    """8 or 64 channels per group and stride 3 to the fused entry points, C % 128 != 0 to the slab entry points: WT_ERR_INVALID with a message,
    nothing launched, and the device still works afterwards."""
    from oracle import backward_ref as B
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.detnet.nn import ops

    def refused(fn, *a):
        with pytest.raises(_lib.WaymoTrackError) as e:
            fn(*a)
        msg = str(e.value)
        assert 'WT_ERR_INVALID' in msg and '(' in msg and not msg.endswith('()'), msg

    for c, groups, stride in ((256, 32, 1), (2048, 32, 1), (512, 32, 3)):
        x = _cl(torch.zeros((1, c, 9, 9)))
        ho = _ho(9, stride)
        off = _cl(torch.zeros((1, 18, ho, ho)))
        dyn = torch.zeros((1, ho, ho, c), device='cuda')
        wt = torch.zeros((c, c // groups, 3, 3), device='cuda')
        refused(ops.deform_dw, x, off, dyn, groups, None, None, stride)
        refused(ops.deform_dxoff, x, off, dyn, wt, groups, None, None, stride)
    x = _cl(torch.zeros((1, 192, 9, 9)))
    off = _cl(torch.zeros((1, 18, 9, 9)))
    refused(ops.deform_im2col, x, off, 1, 1, 4)
    refused(ops.deform_col2im, torch.zeros((4, 81, 9, 48), device='cuda'), x, off, 1, 1, 4)
    x, offset, weight, gy, _, _ = _deform_inputs(5, 1, 512, 9, 9, 1, 1.0)
    _compare_deform('after refused calls', _hip_deform(x, offset, weight, 1, gy), B.deform_grads(x, offset, weight, 32, 1, gy))


# ---------------------------------------------------------------------------------------------------------------------------------
# ROIAlign backward

def _hip_roi(feats, rois, gout, pooled=7):
    from waymo_2d_tracking_amd.detnet.nn import ops
    fg = [_cl(f).requires_grad_() for f in feats]
    out = ops.RoiPoolFpnFn.apply(rois.cuda(), SCALES, pooled, 2, 4, 224.0, *fg)
    out.backward(_cl(gout))
    torch.cuda.synchronize()
    return out.detach().cpu(), [f.grad.cpu() for f in fg]


def _compare_roi(case, got, ref, ref32=None):
    """Project bound |a - b| < 1e-4 max|b| + 1e-6 per level (tests/test_gpu_detops.py), or 4 x the float32 reference's own error if larger."""
    out, grads = got
    assert (out.double() - ref[0]).abs().max().item() <= 1e-4 * ref[0].abs().max().item() + 2e-5, case
    failures = []
    for l, (a, b) in enumerate(zip(grads, ref[1])):
        err = (a.double() - b).abs().max().item()
        top = b.abs().max().item()
        bound = 1e-4 * (top + 1e-6) + 1e-6
        e32 = None
        if ref32 is not None:
            e32 = (ref32[1][l].double() - b).abs().max().item()
            bound = max(bound, 4 * e32)
        if top > 0:                                                             # (a level no ROI uses: the gradient must be zero within 1e-6)
            _ROWS.append((case, 'dp%d' % (l + 2), '-' if e32 is None else '%.3e' % (e32 / top), err / top, bound / top))
        print('%s level %d: max|ref| %.3e, f32 reference %s, HIP %.3e, bound %.3e' % (case, l, top, e32, err, bound))
        if not err < bound:
            failures.append((case, l, err, bound))
    assert not failures, failures


def _mixed_rois(g, n_img, h, w):
    rows = []
    for i in range(48):
        size = (8, 20, 60, 120, 250, 600)[i % 6]
        bw = size * float(torch.empty(1).uniform_(0.5, 2.0, generator=g))
        bh = size * float(torch.empty(1).uniform_(0.5, 2.0, generator=g))
        x1 = float(torch.empty(1).uniform_(-30, w - 10, generator=g))          # partly outside at every border
        y1 = float(torch.empty(1).uniform_(-30, h - 10, generator=g))
        rows.append([float((i * 7) % n_img), x1, y1, x1 + bw, y1 + bh])
    rows += [[1.0, 0.0, 0.0, float(w), float(h)],                               # whole image
             [2.0, -40.0, -40.0, w + 40.0, h + 40.0],                           # larger than the image
             [0.0, w + 50.0, h + 50.0, w + 150.0, h + 120.0],                   # fully outside (lower right)
             [1.0, -300.0, -200.0, -100.0, -90.0],                              # fully outside (upper left)
             [2.0, 33.0, 40.0, 33.0, 90.0],                                     # empty: x1 == x2
             [0.0, 50.0, 20.0, 50.0, 20.0],                                     # empty: a point
             [1.0, 70.0, 30.0, 71.0, 130.0],                                    # one pixel wide
             [2.0, 10.0, 60.0, 200.0, 61.0],                                    # one pixel high
             [0.0, 4.0 * (w // 4) - 2.0, 10.0, 4.0 * (w // 4) + 30.0, 40.0],    # footprint of one column (clamped at the right border)
             [1.0, 42.0, 42.0, 43.0, 43.0],                                     # 2 x 2 footprint
             [2.0, 41.0, 41.0, 45.0, 45.0],                                     # 3 x 3 footprint
             [0.0, 10.5, 2.25, 120.0, 90.0]]
    return torch.tensor(rows, dtype=torch.float32)


@pytest.mark.parametrize('c', [64, 72, 256, 320])
def test_roi_backward_batch_levels_channels_and_degenerate_boxes(c):
    """Batch 3 with mixed image indices, 60 ROIs on all four levels (asserted), channel counts that are / are not multiples of 64 and 256, boxes
    partly and fully outside, empty, one pixel wide, whole-image, and footprints of 1, 2 and 3 columns (fewer than the 4-way column split)."""
    from oracle import backward_ref as B
    g = torch.Generator().manual_seed(c)
    h, w, n = 192, 256, 3
    feats = [torch.randn((n, c, h // s, w // s), generator=g) for s in STRIDES]
    rois = _mixed_rois(g, n, h, w)
    lvl, nr, nc = B.roi_geometry(rois, SCALES, [(h // s, w // s) for s in STRIDES])
    assert set(lvl.tolist()) == {0, 1, 2, 3} and set(rois[:, 0].tolist()) == {0.0, 1.0, 2.0}
    assert {1, 2, 3} <= set(nc.tolist()), sorted(set(nc.tolist()))
    gout = torch.randn((len(rois), c, 7, 7), generator=g)
    _compare_roi('roi mixed C=%d' % c, _hip_roi(feats, rois, gout), B.roi_grads(feats, rois, SCALES, gout))


def test_roi_backward_512_overlapping_rois():
    """A training batch: 512 ROIs clustered on six objects over two images (p2 of a 320 x 480 image is 80 x 120), C = 256 - the float atomics
    under contention; their order varies from run to run, the bound (4 x the float32 reference's own error, at least the project bound) allows it."""
    from oracle import backward_ref as B
    g = torch.Generator().manual_seed(8)
    h, w, n, c = 320, 480, 2, 256
    feats = [torch.randn((n, c, h // s, w // s), generator=g) for s in STRIDES]
    obj = torch.tensor([[60.0, 80.0, 40.0], [200.0, 150.0, 90.0], [400.0, 100.0, 150.0], [120.0, 250.0, 30.0], [300.0, 220.0, 260.0], [440.0, 290.0, 60.0]])
    pick = torch.randint(0, 6, (512,), generator=g)
    ctr = obj[pick, :2] + torch.randn((512, 2), generator=g) * obj[pick, 2:3] * 0.08
    wh = obj[pick, 2:3] * torch.exp(torch.randn((512, 2), generator=g) * 0.15)
    rois = torch.cat(((pick % 2).float().view(-1, 1), ctr - wh / 2, ctr + wh / 2), 1)
    lvl, _, _ = B.roi_geometry(rois, SCALES, [(h // s, w // s) for s in STRIDES])
    assert len(set(lvl.tolist())) >= 3
    gout = torch.randn((512, c, 7, 7), generator=g)
    ref = B.roi_grads(feats, rois, SCALES, gout)
    ref32 = B.roi_grads(feats, rois, SCALES, gout, dtype=torch.float32)
    _compare_roi('roi 512 overlapping', _hip_roi(feats, rois, gout), ref, ref32)


@pytest.mark.parametrize('pooled', [14, 3])
def test_roi_backward_other_pooled_sizes_take_the_per_sample_form(pooled):
    """pooled != 7: roi_pool_fpn_bwd_kernel<0> -> roi_bwd_samples for every ROI, against the reference with the same pooled size."""
    from oracle import backward_ref as B
    g = torch.Generator().manual_seed(pooled)
    h, w, n, c = 128, 192, 2, 72
    feats = [torch.randn((n, c, h // s, w // s), generator=g) for s in STRIDES]
    rois = _mixed_rois(g, n, h, w)[::2].contiguous()
    gout = torch.randn((len(rois), c, pooled, pooled), generator=g)
    _compare_roi('roi pooled=%d' % pooled, _hip_roi(feats, rois, gout, pooled), B.roi_grads(feats, rois, SCALES, gout, pooled))


def test_roi_backward_footprints_above_the_separable_tables():
    """Feature maps of a 1920 x 1280 image: a 1900 x 20 box lands on p3 with 240 footprint columns, a 9 x 1270 box on p2 with 320 rows - more than
    the 192 the separable kernel's LDS tables hold, so those ROIs take roi_bwd_samples inside the <7> kernel; one box with exactly 192 columns (the
    last separable one) and one with 193.  All asserted from the level rule and the scales in the kernel's float32 arithmetic."""
    from oracle import backward_ref as B
    g = torch.Generator().manual_seed(4)
    h, w, c = 1280, 1920, 64
    feats = [torch.randn((1, c, h // s, w // s), generator=g) for s in STRIDES]
    rois = torch.tensor([[0.0, 10.0, 100.0, 1910.0, 120.0], [0.0, 100.0, 5.0, 109.0, 1275.0], [0.0, 84.0, 40.0, 1608.0, 60.0],
                         [0.0, 84.0, 40.0, 1616.0, 60.0], [0.0, 300.0, 300.0, 420.0, 380.0], [0.0, 0.0, 0.0, 1920.0, 1280.0],
                         [0.0, 1000.0, 700.0, 1900.0, 1270.0]])
    lvl, nr, nc = B.roi_geometry(rois, SCALES, [(h // s, w // s) for s in STRIDES])
    assert lvl.tolist()[:4] == [1, 0, 1, 1]
    assert nc.tolist()[0] > 192 and nr.tolist()[1] > 192 and nc.tolist()[2] == 192 and nc.tolist()[3] == 193, (nr.tolist(), nc.tolist())
    gout = torch.randn((len(rois), c, 7, 7), generator=g)
    _compare_roi('roi footprint > 192', _hip_roi(feats, rois, gout), B.roi_grads(feats, rois, SCALES, gout))


def test_roi_backward_ignores_rows_with_an_image_index_out_of_range():
    """Image index -1 and N: no gradient, no error, and the other ROIs' gradients are what they are without those rows."""
    from oracle import backward_ref as B
    g = torch.Generator().manual_seed(6)
    h, w, n, c = 96, 128, 2, 64
    feats = [torch.randn((n, c, h // s, w // s), generator=g) for s in STRIDES]
    rois = torch.tensor([[0.0, 3.0, 5.0, 40.0, 33.0], [-1.0, 10.5, 2.25, 120.0, 90.0], [1.0, 60.0, 40.0, 75.0, 58.0], [2.0, 0.0, 0.0, 127.0, 95.0],
                         [1.0, 20.0, 30.0, 90.0, 44.0]])
    gout = torch.randn((5, c, 7, 7), generator=g)
    out, grads = _hip_roi(feats, rois, gout)
    assert not out[1].any() and not out[3].any()
    _compare_roi('roi bad index', (out, grads), B.roi_grads(feats, rois, SCALES, gout))
    keep = torch.tensor([0, 2, 4])
    _compare_roi('roi bad index (rows removed)', (out[keep], grads), B.roi_grads(feats, rois[keep], SCALES, gout[keep]))
    only_bad = _hip_roi(feats, rois[[1, 3]].contiguous(), gout[:2])[1]
    assert all(not a.any() for a in only_bad)


def test_roi_backward_without_rois_returns_zero_gradients():
    g = torch.Generator().manual_seed(6)
    feats = [torch.randn((2, 64, 96 // s, 128 // s), generator=g) for s in STRIDES]
    out, grads = _hip_roi(feats, torch.zeros((0, 5)), torch.zeros((0, 64, 7, 7)))
    assert out.shape == (0, 64, 7, 7)
    for f, a in zip(feats, grads):
        assert a.shape == f.shape and not a.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the elementwise passes (exact in float32)

def _misaligned(m, n):
    return torch.zeros(m * n + 1, device='cuda')[1:].view(m, n)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('with_scale', [False, True])
def test_act_bwd_is_exact(relu, with_scale):
    """wd_act_bwd_f32: g = dy * (y > 0 if relu) * scale[col], bit for bit the torch expression in float32, for all four (mask, scale)
    combinations; y == 0 exactly and -0.0 give 0; N = 4, a ragged M, and a matrix above the 4096-block grid cap (its stride loop runs)."""
    from waymo_2d_tracking_amd.detnet.nn import ops
    g = torch.Generator().manual_seed(1)
    for m, n in ((7, 4), (1037, 260), (2100, 2048)):
        if m == 2100:
            assert m * n > 4096 * 256 * 4
        dy = torch.randn((m, n), generator=g)
        y = torch.randn((m, n), generator=g)
        y.view(-1)[::5] = 0.0
        y.view(-1)[1::7] = -0.0
        scale = (torch.rand(n, generator=g) + 0.5) if with_scale else None
        want = torch.where(y > 0, dy, torch.zeros_like(dy)) if relu else dy.clone()
        if with_scale:
            want = want * scale
        got = ops.act_bwd(dy.cuda(), y.cuda(), scale.cuda() if with_scale else None, relu)
        assert torch.equal(got.cpu(), want), (m, n)


@pytest.mark.parametrize('relu', [False, True])
def test_bias_relu_is_exact(relu):
    """wd_bias_relu_f32: y = act(y + bias[col]) in place, bit for bit; N = 4, a ragged M, a matrix above the 2048-block grid cap."""
    from waymo_2d_tracking_amd.detnet.nn import ops
    g = torch.Generator().manual_seed(2)
    for m, n in ((7, 4), (1037, 260), (1100, 2048)):
        if m == 1100:
            assert m * n > 2048 * 256 * 4
        y = torch.randn((m, n), generator=g)
        bias = torch.randn(n, generator=g)
        y[::3] = -bias                                                          # y + bias == 0 exactly
        want = torch.relu(y + bias) if relu else y + bias
        yg = y.cuda()
        got = ops.bias_relu_(yg, bias.cuda(), relu)
        assert got.data_ptr() == yg.data_ptr() and torch.equal(got.cpu(), want), (m, n)


def test_elementwise_passes_refuse_what_their_float4_lanes_cannot_take():
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.detnet.nn import ops
    ok = torch.ones((5, 8), device='cuda')
    cases = [lambda: ops.act_bwd(torch.ones((5, 6), device='cuda'), torch.ones((5, 6), device='cuda'), None, True),       # N % 4 != 0
             lambda: ops.act_bwd(_misaligned(5, 8), ok, None, True),
             lambda: ops.act_bwd(ok, _misaligned(5, 8), None, True),
             lambda: ops.act_bwd(ok, ok, _misaligned(1, 8).view(8), False),
             lambda: ops.bias_relu_(torch.ones((5, 6), device='cuda'), torch.ones(6, device='cuda')),
             lambda: ops.bias_relu_(_misaligned(5, 8), torch.ones(8, device='cuda')),
             lambda: ops.bias_relu_(ok.clone(), _misaligned(1, 8).view(8))]
    for i, fn in enumerate(cases):
        with pytest.raises(_lib.WaymoTrackError) as e:
            fn()
        assert 'WT_ERR_INVALID' in str(e.value) and 'multiple of 4' in str(e.value), (i, str(e.value))
    assert torch.equal(ops.act_bwd(ok, ok, None, True), ok)                     # the device still works
