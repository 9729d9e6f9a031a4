"""Op-level tests of the INFERENCE FORWARD kernels (csrc/det_gconv.hip, csrc/det_deform.hip, csrc/det_deform_pp.hip, the GroupNorm and tap
shift-add kernels of csrc/det_misc.hip) against float64 references, at the shapes tests/test_gpu_detops.py never enters: several tiles per
persistent workgroup (sized from the card's CU count: tests/forward_shapes.py restates the two launch rules and every multi-tile test asserts
its conditions before it launches), the fused epilogues of the grouped conv, C = 128 and 384 there, maps smaller than a tile or one pixel wide on
every deformable kernel, 8 channels per group with offsets, stride 2 at C = 1024, what dispatch reroutes (modulation mask, pad != 1), all four
GroupNorm widths with a second channel trip, and the grid-stride loop of the tap shift-add.

Which kernel ran is an assertion in every deformable / grouped case: ops.EVENT_LOG carries the name the launcher recorded for the launch
(wd_deform_conv3x3_last_kernel), next to the wd_deform_conv3x3_variant query the older tests use.

References: oracle.detops_ref.deform_conv3x3 (float64; on the device for the large cases), torch conv2d in float64, torch group_norm (+ relu) in
float64 with autograd.  Bounds are the project's own: rtol = atol = 1e-4 for the deformable and grouped convs (test_deform_conv_vs_reference),
rtol 1e-4 / atol 1e-5 for the GroupNorm forward (test_groupnorm_relu_vs_torch), max|a - b| / max|b| < 1e-4 for its gradients
(test_groupnorm_relu_autograd_function_vs_torch), 1e-4 of max(1, max|b|) for the offset conv (test_conv3x3_few_vs_conv2d); equalities are
bit-exact.

Inputs chosen by reasoning, not by what the kernels give:
  * the ping-pong steady-state cases round their offsets to odd multiples of 1/1024 (oracle.backward_ref.exact_offsets).  The kernels add base
    and offset in float32; on maps of a hundred pixels that rounds the position by up to 8e-6 px, and over the millions of outputs of these
    cases the largest resulting difference (bounded by ~5 sigma of 8e-6 x |dx/dpx| x |w| x sqrt(288), some 1e-5) would eat into atol with no
    kernel at fault.  With exact positions kernel and reference blend the same cell with the same fractions, and what is measured is the
    kernel's arithmetic alone.  The small maps use the raw normal offsets.
  * the "stale patch" grouped-conv case uses integer inputs (|x| <= 1000 inside, +-1 on the two outermost rows / columns) and weights that are
    multiples of 1/64: every float32 product and sum is exact (< 2^24 / 64), so the expected error is 0 and a slot left over from the previous
    tile shows as an error of order 1e3 x |w| at an output of order 1.
  * GroupNorm: see forward_shapes.gn_inputs / gn_reference (the ReLU-mask guard and why |beta| >= 0.1), and
    test_groupnorm_group_with_constant_input for why the constant of a variance-0 group is 2^-6 and not of order 1.

Set WD_FORWARD_ERROR_TABLE=<file> to have the module write the table of all measured errors (profiles/forward_ops_error.txt) when it finishes.
"""
import ctypes as C
import os

import pytest
import torch

from forward_shapes import (GN_CONFIGS, GN_GUARD_SHARE, GN_ROIS, GN_SPATIAL, GCONV_MIN_TILES, MAX_INPUT_BYTES, PP_MIN_TILES, gconv_conditions,
                            gconv_launch, gconv_shape, gn_inputs, gn_reference, out_size, pp_conditions, pp_launch, pp_shape, pp_work_order, tiles)

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-4          # tests/test_gpu_detops.py::test_deform_conv_vs_reference
_ROWS = []
_CACHE = {}
_RAN = set()                     # kernel names the launcher reported


@pytest.fixture(scope='module', autouse=True)
def _module_state():
    yield
    _CACHE.clear()
    path = os.environ.get('WD_FORWARD_ERROR_TABLE')
    if path:
        with open(path, 'w') as f:
            f.write('CUs %d\n' % _cus())
            f.write('kernels reported by the launcher: %s\n' % ', '.join(sorted(_RAN)))
            f.write('%-86s %-12s %-12s %s\n' % ('case', 'error', 'bound', 'error / bound'))
            for row in _ROWS:
                f.write('%-86s %-12.3e %-12.3e %.3e\n' % row)


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _cus():
    from waymo_2d_tracking_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == _lib.device_info()[2], (cus, _lib.device_info())          # the launch rules read the library's count
    return cus


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _query(c, groups, stride, pad, has_offset):
    from waymo_2d_tracking_amd import _lib
    fn = _lib.lib().wd_deform_conv3x3_variant
    fn.restype = C.c_char_p
    return fn(C.c_int(c), C.c_int(groups), C.c_int(stride), C.c_int(pad), C.c_int(1 if has_offset else 0)).decode()


def _conv(expect, *args, **kw):
    """ops.deform_conv3x3 under the event log; asserts that the launcher reports kernel `expect`."""
    from waymo_2d_tracking_amd.detnet.nn import ops
    ops.EVENT_LOG = []
    try:
        y = ops.deform_conv3x3(*args, **kw)
        names = [t[0].split(':')[0] for t in ops.EVENT_LOG]
    finally:
        ops.EVENT_LOG = None
    assert names == [expect], (names, expect)
    _RAN.add(expect)
    return y


def _check(case, got, exp, rtol=RTOL, atol=ATOL):
    """numpy.testing.assert_allclose's rule |a - b| <= atol + rtol |b| on every element (on the device the reference lives on); records the
    largest error and the bound at that element."""
    assert got.shape == exp.shape, (case, got.shape, exp.shape)
    got = got.to(exp.device).double()
    assert bool(torch.isfinite(got).all()), case
    err = (got - exp).abs()
    bound = atol + rtol * exp.abs()
    ratio = err / bound
    i = int(ratio.argmax()) if ratio.numel() else None
    worst = (float(err.reshape(-1)[i]), float(bound.reshape(-1)[i]), float(ratio.reshape(-1)[i])) if i is not None else (0.0, atol, 0.0)
    _ROWS.append((case,) + worst)
    print('%s: error %.3e, bound %.3e, ratio %.3e' % ((case,) + worst))
    assert worst[2] <= 1.0, (case,) + worst


def _affine(exp, scale, bias, relu):
    out = exp
    if scale is not None:
        out = out * scale.to(exp.device).double().view(1, -1, 1, 1)
    if bias is not None:
        out = out + bias.to(exp.device).double().view(1, -1, 1, 1)
    return torch.relu(out) if relu else out


EPILOGUES = {'none': (False, False, False), 'full': (True, True, True), 'scale': (True, False, False), 'bias': (False, True, False),
             'relu': (False, False, True)}


def _epilogue_args(name, scale, bias):
    s, b, r = EPILOGUES[name]
    return (scale if s else None), (bias if b else None), r


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. grouped conv, 8 channels per group (grouped_conv3x3_c8_kernel)

def _gconv_inputs(c, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, c, h, w), generator=g)
    weight = torch.randn((c, 8, 3, 3), generator=g) / (3 * 8 ** 0.5)
    scale = torch.rand(c, generator=g) + 0.5
    bias = torch.randn(c, generator=g)
    return x, weight, scale, bias


def _gconv_case(case, c, x, weight, scale, bias, epilogues, device_ref):
    from waymo_2d_tracking_amd.detnet.nn import ops
    groups = c // 8
    assert _query(c, groups, 1, 1, False) == 'grouped_conv3x3_c8_kernel'
    xg = _cl(x)
    if device_ref:
        exp = _cached(case, lambda: torch.nn.functional.conv2d(xg.double(), weight.cuda().double(), None, 1, 1, 1, groups))
    else:
        exp = torch.nn.functional.conv2d(x.double(), weight.double(), None, 1, 1, 1, groups)
    packed = ops.deform_pack_weight(weight.cuda(), groups)
    for name in epilogues:
        s, b, r = _epilogue_args(name, scale, bias)
        got = _conv('grouped_conv3x3_c8_kernel', xg, None, packed, groups, 1, 1, scale=None if s is None else s.cuda(),
                    bias=None if b is None else b.cuda(), relu=r)
        _check('%s epilogue %s' % (case, name), got, _affine(exp, s, b, r))


def _assert_gconv_multi_tile(c, n, h, w):
    cus = _cus()
    assert not gconv_conditions(cus, c, n, h, w), gconv_conditions(cus, c, n, h, w)
    ntiles, per_half, lo, hi = gconv_launch(cus, c, n, h, w)
    assert lo >= GCONV_MIN_TILES and hi == lo + 1 and 4 * n * c * h * w <= MAX_INPUT_BYTES, (ntiles, per_half, lo, hi)
    return 'CUs %d: %d tiles on %d workgroups per half (%d-%d each)' % (cus, ntiles, per_half, lo, hi)


@pytest.mark.parametrize('c,epilogues', [(128, ('none', 'full')), (256, ('none', 'full', 'scale', 'bias', 'relu')), (384, ('none', 'full'))])
def test_grouped_conv_several_tiles_per_workgroup(c, epilogues):
    """The persistent loop of grouped_conv3x3_c8_kernel takes 3 - 4 trips per workgroup, the last one ragged: the barrier in front of the next
    patch fill, zero-fill over a previous tile's data, the prefetch wrap at the last pixel, inner and border tiles in turn, image boundaries
    inside a workgroup's tile list; one (C = 128), two and three (blockIdx % halves) channel halves; every epilogue combination."""
    n, h, w = gconv_shape(_cus(), c)
    how = _assert_gconv_multi_tile(c, n, h, w)
    print(how)
    x, weight, scale, bias = _gconv_inputs(c, n, h, w, c)
    _gconv_case('gconv C=%d %dx%dx%d [%s]' % (c, n, h, w, how), c, x, weight, scale, bias, epilogues, True)


def test_grouped_conv_stale_patch_slots_show_at_full_size():
    """Integer inputs of magnitude 1e3 inside the image and +-1 on its two outermost rows / columns, weights on a 1/64 grid: float32 is exact
    (module docstring), so the error is 0 unless a border tile's zero-filled halo or a ragged tile keeps data of the workgroup's previous tile."""
    c = 256
    n, h, w = gconv_shape(_cus(), c)
    how = _assert_gconv_multi_tile(c, n, h, w)
    g = torch.Generator().manual_seed(77)
    x = torch.randint(-1000, 1001, (n, c, h, w), generator=g).float()
    edge = torch.ones((h, w), dtype=torch.bool)
    edge[2:h - 2, 2:w - 2] = False
    x = torch.where(edge, torch.randint(0, 2, x.shape, generator=g).float() * 2 - 1, x)
    weight = torch.randint(-64, 65, (c, 8, 3, 3), generator=g).float() / 64
    assert float(x[:, :, 2:-2, 2:-2].abs().max()) == 1000.0 and float(x[:, :, :2].abs().max()) == 1.0
    _gconv_case('gconv stale patch C=256 %dx%dx%d [%s]' % (n, h, w, how), c, x, weight, None, None, ('none',), True)
    assert _ROWS[-1][1] == 0.0, _ROWS[-1]                                    # exact arithmetic on both sides


@pytest.mark.parametrize('h,w', [(1, 1), (1, 9), (9, 1), (2, 2), (7, 7), (8, 8), (9, 8), (17, 15), (27, 30)])
def test_grouped_conv_small_and_odd_maps(h, w):
    """Maps below one tile, one pixel wide, exactly a tile, a row more: no tile is `inner` and every LDS-DMA pair of the patch fill straddles a
    border (half-waves split between the DMA and the zero-fill); 27 x 30 has one fully inner tile surrounded by border tiles."""
    c, n = 256, 2
    if (h, w) == (27, 30):
        assert tiles(h) == 4 and tiles(w) == 4 and 1 * 8 - 1 >= 0 and 2 * 8 - 1 + 10 <= h            # tiles (1..2, 1..2) are inner
    x, weight, scale, bias = _gconv_inputs(c, n, h, w, 100 * h + w)
    _gconv_case('gconv C=256 %dx%dx%d' % (n, h, w), c, x, weight, scale, bias, ('none', 'full'), False)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. deformable forward: small and odd maps on every kernel, and what dispatch reroutes

def _deform_inputs(seed, n, c, h, w, stride, pad, osc, groups=32):
    g = torch.Generator().manual_seed(seed)
    ho, wo = (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1
    x = torch.randn((n, c, h, w), generator=g)
    offset = torch.randn((n, 18, ho, wo), generator=g) * osc
    weight = torch.randn((c, c // groups, 3, 3), generator=g) / (3 * (c // groups) ** 0.5)
    mask = torch.rand((n, 9, ho, wo), generator=g)
    scale = torch.rand(c, generator=g) + 0.5
    bias = torch.randn(c, generator=g)
    return x, offset, weight, mask, scale, bias


def _deform_compare(case, expect, x, offset, weight, mask, scale, bias, stride, pad, exp, groups=32):
    """Plain and with the fused affine + ReLU, on the kernel `expect`."""
    from waymo_2d_tracking_amd.detnet.nn import ops
    packed = ops.deform_pack_weight(weight.cuda(), groups)
    m = None if mask is None else _cl(mask)
    got = _conv(expect, _cl(x), _cl(offset), packed, groups, stride, pad, mask=m)
    _check('%s %s' % (case, expect), got, exp)
    got = _conv(expect, _cl(x), _cl(offset), packed, groups, stride, pad, scale=scale.cuda(), bias=bias.cuda(), relu=True, mask=m)
    _check('%s %s epilogue' % (case, expect), got, _affine(exp, scale, bias, True))


@pytest.mark.parametrize('c', [256, 512, 1024, 2048])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('h,w', [(1, 1), (1, 9), (9, 1), (7, 7), (8, 8), (9, 8), (17, 15)])
def test_deform_forward_small_and_odd_maps_on_every_kernel(h, w, stride, c, monkeypatch):
    """Default dispatch and every kernel WD_DEFORM_PATCH can force for the (channels per group, stride): the gather kernel (8 channels per group
    with offsets: deform_conv3x3_kernel<8,true>), the patch kernel, the LDS kernel, the ping-pong kernel (stride 1 and 2, <16> and <32>) - on maps
    below one tile, one pixel wide, exactly one tile and a row more; with and without the epilogue; with a modulation mask where the kernel takes
    one (the ping-pong kernel does not: dispatch reroutes, next tests)."""
    from oracle import detops_ref as R
    n = 2
    x, offset, weight, mask, scale, bias = _deform_inputs(c + 100 * h + 10 * w + stride, n, c, h, w, stride, 1, 1.5)
    exp = R.deform_conv3x3(x, offset, weight, 32, stride, 1, None)
    exp_m = None
    seen = set()
    for mode in (None, 'lds', 'all', 'none'):
        if mode is None:
            monkeypatch.delenv('WD_DEFORM_PATCH', raising=False)
        else:
            monkeypatch.setenv('WD_DEFORM_PATCH', mode)
        kernel = _query(c, 32, stride, 1, True)
        if kernel in seen:
            continue
        seen.add(kernel)
        case = 'small C=%d %dx%dx%d s%d' % (c, n, h, w, stride)
        _deform_compare(case, kernel, x, offset, weight, None, scale, bias, stride, 1, exp)
        if 'pp_kernel' not in kernel:
            if exp_m is None:
                exp_m = R.deform_conv3x3(x, offset, weight, 32, stride, 1, mask)
            _deform_compare(case + ' mask', kernel, x, offset, weight, mask, scale, bias, stride, 1, exp_m)
    cg = c // 32
    want = {8: {'deform_conv3x3_kernel<8,true>'},
            64: {'deform_conv3x3_patch_kernel<64>', 'deform_conv3x3_kernel<64,true>'} if stride == 1 else {'deform_conv3x3_kernel<64,true>'}}.get(cg)
    if want is None:
        want = {'deform_conv3x3_pp_kernel<%d>' % cg, 'deform_conv3x3_kernel<%d,true>' % cg}
        if stride == 1:
            want |= {'deform_conv3x3_lds_kernel<%d>' % cg, 'deform_conv3x3_patch_kernel<%d>' % cg}
    assert seen == want, (seen, want)


@pytest.mark.parametrize('c', [512, 1024])
@pytest.mark.parametrize('stride', [1, 2])
def test_deform_forward_mask_reroutes_the_pingpong_shapes(c, stride, monkeypatch):
    """The shapes the ping-pong kernel owns, WITH a modulation mask, under the default dispatch: stride 1 goes to the LDS kernel, stride 2 to the
    gather kernel (the shape-only query still names the ping-pong kernel; the launcher's record is what is asserted)."""
    from oracle import detops_ref as R
    monkeypatch.delenv('WD_DEFORM_PATCH', raising=False)
    cg = c // 32
    assert _query(c, 32, stride, 1, True) == 'deform_conv3x3_pp_kernel<%d>' % cg
    expect = ('deform_conv3x3_lds_kernel<%d>' if stride == 1 else 'deform_conv3x3_kernel<%d,true>') % cg
    n, h, w = 2, 21, 30
    x, offset, weight, mask, scale, bias = _deform_inputs(c + stride, n, c, h, w, stride, 1, 1.5)
    exp = R.deform_conv3x3(x, offset, weight, 32, stride, 1, mask)
    _deform_compare('mask reroute C=%d s%d' % (c, stride), expect, x, offset, weight, mask, scale, bias, stride, 1, exp)


@pytest.mark.parametrize('c', [512, 2048])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('pad', [0, 2])
def test_deform_forward_other_paddings_take_the_gather_kernel(pad, stride, c, monkeypatch):
    """pad 0 and 2 (the ABI accepts them; only pad 1 fits the patch kernels): the gather kernel, output grid (H + 2 pad - 3) / stride + 1."""
    from oracle import detops_ref as R
    monkeypatch.delenv('WD_DEFORM_PATCH', raising=False)
    expect = 'deform_conv3x3_kernel<%d,true>' % (c // 32)
    assert _query(c, 32, stride, pad, True) == expect
    n, h, w = 2, 13, 18
    x, offset, weight, mask, scale, bias = _deform_inputs(c + 10 * pad + stride, n, c, h, w, stride, pad, 1.5)
    assert offset.shape[2:] == ((h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1)
    exp = R.deform_conv3x3(x, offset, weight, 32, stride, pad, None)
    assert exp.shape[2:] == offset.shape[2:]
    _deform_compare('pad %d C=%d s%d' % (pad, c, stride), expect, x, offset, weight, None, scale, bias, stride, pad, exp)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. ping-pong kernel in steady state

def _tile_scale_map(n, ho, wo, every=3, big=10.0):
    """(n, 1, ho, wo) factor: `big` on every third 8 x 8 tile in the kernel's work order, 1 elsewhere."""
    f = torch.ones((n, 1, ho, wo))
    for t, (tn, ty, tx) in enumerate(pp_work_order(n, ho, wo)):
        if t % every == 0:
            f[tn, 0, ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = big
    return f


def _assert_pp_multi_tile(c, n, h, w, stride):
    cus = _cus()
    assert not pp_conditions(cus, c, n, h, w, stride), pp_conditions(cus, c, n, h, w, stride)
    ntiles, nsplit, lo, hi = pp_launch(cus, c, n, h, w, stride)
    assert lo[1] >= PP_MIN_TILES and 4 * n * c * h * w <= MAX_INPUT_BYTES, (ntiles, nsplit, lo, hi)
    return 'CUs %d: %d tiles on %d workgroups per item (teams %d+%d .. %d+%d)' % (cus, ntiles, nsplit, lo[0], lo[1], hi[0], hi[1])


@pytest.mark.parametrize('c,stride', [(1024, 1), (1024, 2), (512, 2)])
def test_pingpong_kernel_steady_state(c, stride, monkeypatch):
    """Every team of deform_conv3x3_pp_kernel works through 4 or more tiles, so both patch / table buffers are refilled more than once while the
    other is read; workgroups of two sizes, a dummy item on team 1 of the odd ones, image boundaries inside a tile range.  Offsets: N(0, 0.6^2)
    with every third tile (work order) drawn from N(0, 6^2), so consecutive tiles of a team alternate between the in-patch fast path and the
    far path (shares asserted).  <32> at stride 1 and 2, <16> at stride 2; with and without the epilogue.  Reference on the device."""
    from oracle import backward_ref as B
    from oracle import detops_ref as R
    monkeypatch.delenv('WD_DEFORM_PATCH', raising=False)
    n, h, w = pp_shape(_cus(), c, stride)
    how = _assert_pp_multi_tile(c, n, h, w, stride)
    print(how)
    expect = 'deform_conv3x3_pp_kernel<%d>' % (c // 32)
    assert _query(c, 32, stride, 1, True) == expect
    x, offset, weight, _, scale, bias = _deform_inputs(c + stride, n, c, h, w, stride, 1, 0.6)
    ho, wo = out_size(h, stride), out_size(w, stride)
    big = _tile_scale_map(n, ho, wo)
    offset = B.exact_offsets(offset * big)
    far = (offset.abs() > 2.0).reshape(n, 9, 2, ho, wo).any(dim=2).float()                   # beyond the patch's 2-pixel halo (stride 1)
    wild, calm = (big[:, 0] > 1).unsqueeze(1).expand_as(far), (big[:, 0] == 1).unsqueeze(1).expand_as(far)
    assert float(far[wild].mean()) > 0.8 and float(far[calm].mean()) < 0.01, (float(far[wild].mean()), float(far[calm].mean()))
    xg, og = _cl(x), _cl(offset)
    exp = R.deform_conv3x3(xg, og, weight.cuda(), 32, stride, 1, None)
    assert exp.is_cuda
    case = 'pp steady C=%d %dx%dx%d s%d [%s]' % (c, n, h, w, stride, how)
    _deform_compare(case, expect, x, offset, weight, None, scale, bias, stride, 1, exp)


def test_pingpong_kernel_steady_state_with_the_prepass_table():
    """The stride-1 steady-state shape with the sampling table of the offset conv's gather launch (conv3x3_few(..., deform_table=True)) against
    the table the launcher builds itself: bit-equal outputs.  The offsets are what the offset conv computes; every third tile (work order) of
    the input is scaled by 10, so those tiles' offsets are wide (far path) and the others stay inside the patch."""
    from waymo_2d_tracking_amd.detnet.nn import ops
    c = 1024
    n, h, w = pp_shape(_cus(), c, 1)
    _assert_pp_multi_tile(c, n, h, w, 1)
    g = torch.Generator().manual_seed(5)
    x = _cl(torch.randn((n, c, h, w), generator=g) * _tile_scale_map(n, h, w))
    packed = ops.deform_pack_weight((torch.randn((c, 32, 3, 3), generator=g) * 0.05).cuda(), 32)
    w_off = (torch.randn((18, c, 3, 3), generator=g) * (0.6 / 96.0)).cuda()
    b_off = (torch.randn(18, generator=g) * 0.06).cuda()
    w2 = ops.tap_gemm_weight(w_off)
    off_a = ops.conv3x3_few(x, w2, b_off, 18, 1)
    off_b, table = ops.conv3x3_few(x, w2, b_off, 18, 1, deform_table=True)
    assert torch.equal(off_a, off_b)
    share = float((off_a.abs() > 2.0).float().mean())
    assert 0.05 < share < 0.6, share                                                          # both paths are busy
    ya = _conv('deform_conv3x3_pp_kernel<32>', x, off_a, packed, 32, 1, 1)
    yb = _conv('deform_conv3x3_pp_kernel<32>', x, off_b, packed, 32, 1, 1, table=table)
    assert torch.equal(ya, yb)
    _ROWS.append(('pp steady C=1024 %dx%dx%d pre-pass table vs in-kernel table (bit-equal)' % (n, h, w), 0.0, 0.0, 0.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. GroupNorm + ReLU, forward and backward

def _hip_groupnorm(x, gamma, beta, groups, relu, gy):
    from waymo_2d_tracking_amd.detnet.nn import ops
    xg, wg, bg = _cl(x).requires_grad_(), gamma.cuda().requires_grad_(), beta.cuda().requires_grad_()
    yg = ops.GroupNormReluFn.apply(xg, wg, bg, groups, 1e-5, relu)
    yg.backward(_cl(gy))
    inplace = ops.groupnorm_relu_(_cl(x).clone(memory_format=torch.channels_last), gamma.cuda(), beta.cuda(), groups, 1e-5, relu)
    assert torch.equal(inplace, yg.detach())                                  # in place == into a second buffer, bit for bit
    return yg.detach().cpu(), xg.grad.cpu(), wg.grad.cpu(), bg.grad.cpu()


def _groupnorm_case(case, x, gamma, beta, groups, relu, gy):
    ref = gn_reference(x, gamma, beta, groups, relu, gy)
    assert ref[5] <= GN_GUARD_SHARE, (case, ref[5])
    got = _hip_groupnorm(x, gamma, beta, groups, relu, ref[4])
    _check(case + ' y', got[0], ref[0], rtol=1e-4, atol=1e-5)                # test_groupnorm_relu_vs_torch
    failures = []
    for name, a, e in (('dx', got[1], ref[1]), ('dgamma', got[2], ref[2]), ('dbeta', got[3], ref[3])):
        assert a.shape == e.shape and bool(torch.isfinite(a).all()), (case, name)
        err = (a.double() - e).abs().max().item() / (e.abs().max().item() + 1e-12)      # test_groupnorm_relu_autograd_function_vs_torch
        _ROWS.append(('%s %s' % (case, name), err, 1e-4, err / 1e-4))
        if not err < 1e-4:
            failures.append((case, name, err))
    assert not failures, failures


@pytest.mark.parametrize('r', GN_ROIS)
@pytest.mark.parametrize('c,groups', GN_CONFIGS)
def test_groupnorm_relu_forward_and_backward(c, groups, r):
    """All four template widths (4, 8, 16, 32 channels per group), C = 320 (one wave on the second channel trip) and 512 (all four), HW = 1, 2,
    49, 63 and 64 (the register array's bound), 1, 5 and 64 ROIs (the dgamma / dbeta atomics), with and without the ReLU; forward in place and
    into a second buffer."""
    assert {cc // gg for cc, gg in GN_CONFIGS} == {4, 8, 16, 32} and c // groups in (4, 8, 16, 32)
    for h, w in GN_SPATIAL:
        for relu in (False, True):
            x, gamma, beta, gy = gn_inputs(c, groups, r, h, w)
            _groupnorm_case('groupnorm C=%d G=%d R=%d %dx%d relu=%d' % (c, groups, r, h, w, relu), x, gamma, beta, groups, relu, gy)


@pytest.mark.parametrize('c,groups', [(256, 32), (320, 20)])
def test_groupnorm_group_with_constant_input(c, groups):
    """One group of every ROI (and the last group of one ROI) holds a constant: variance 0, rstd = eps^-1/2 = 316 in both directions.
    The constants are 2^-6 and -2^-5, not of order 1.  With variance 0 the output moves by 316 gamma times any perturbation of one input
    element, so at |x| = 0.75 a single float32 ulp of x (6e-8) is 1.9e-5 gamma of output - beyond the forward bound's atol of 1e-5 before any
    arithmetic is done.  The forward kernel (x g + (beta - mean g), g = gamma rstd) and float32 torch.nn.functional.group_norm, which
    evaluates the same form, both miss the bound there by the same 5e-5 to 6e-5 (1.2 - 1.6 x the bound) against float64 on identical
    float32 data: the input is ill-conditioned for this bound, the kernel is not wrong.  At 2^-6 an ulp of x is worth 6e-7 gamma, 6 % of
    the bound, and a kernel that mishandled variance 0 (rstd, the mean, a NaN) would still be off by the size of gamma xh."""
    cpg = c // groups
    for relu in (False, True):
        x, gamma, beta, gy = gn_inputs(c, groups, 5, 7, 7)
        x[:, 3 * cpg:4 * cpg] = 2.0 ** -6
        x[2, (groups - 1) * cpg:] = -2.0 ** -5
        _groupnorm_case('groupnorm constant group C=%d G=%d relu=%d' % (c, groups, relu), x, gamma, beta, groups, relu, gy)


def test_groupnorm_without_rois_launches_nothing_and_returns_zero_gradients():
    from waymo_2d_tracking_amd.detnet.nn import ops
    x = torch.zeros((0, 256, 7, 7), device='cuda').contiguous(memory_format=torch.channels_last)
    gamma, beta = torch.ones(256, device='cuda'), torch.ones(256, device='cuda')
    assert ops.groupnorm_relu_(x, gamma, beta, 32).shape == (0, 256, 7, 7)
    wg, bg = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    xg = x.clone().requires_grad_()
    y = ops.GroupNormReluFn.apply(xg, wg, bg, 32, 1e-5, True)
    assert y.shape == (0, 256, 7, 7)
    y.backward(torch.zeros_like(y))
    assert xg.grad.shape == x.shape and not wg.grad.any() and not bg.grad.any()
    # the backward entry on its own: dgamma / dbeta are overwritten with zeros
    from waymo_2d_tracking_amd import _lib
    dg, db = torch.full((256,), 7.0, device='cuda'), torch.full((256,), 7.0, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().wd_groupnorm_relu_bwd_nhwc_f32(p(x), p(x), p(gamma), p(beta), C.c_int(0), C.c_int(49), C.c_int(256), C.c_int(32),
                                                         C.c_float(1e-5), C.c_int(1), p(x), p(dg), p(db), ops._stream()), 'bwd')
    assert not dg.any() and not db.any()


def test_groupnorm_refuses_unsupported_shapes_on_the_host():
    """HW = 65, 2 channels per group and C = 96: WT_ERR_INVALID with the documented message from the forward (both forms) and the backward entry,
    nothing launched, and the device still works."""
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.detnet.nn import ops
    p = lambda t: C.c_void_p(t.data_ptr())
    for (c, groups, h, w, words) in ((256, 32, 5, 13, 'hw <= 64'), (64, 32, 7, 7, 'channels per group'), (96, 12, 7, 7, 'C % 64 == 0')):
        x = torch.ones((3, c, h, w), device='cuda').contiguous(memory_format=torch.channels_last)
        gamma, beta = torch.ones(c, device='cuda'), torch.ones(c, device='cuda')
        dx, dg, db = torch.empty_like(x), torch.empty(c, device='cuda'), torch.empty(c, device='cuda')
        calls = [lambda: ops.groupnorm_relu_(x, gamma, beta, groups),
                 lambda: ops.GroupNormReluFn.apply(x, gamma, beta, groups, 1e-5, True),
                 lambda: _lib.check(_lib.lib().wd_groupnorm_relu_bwd_nhwc_f32(p(x), p(x), p(gamma), p(beta), C.c_int(3), C.c_int(h * w), C.c_int(c),
                                                                               C.c_int(groups), C.c_float(1e-5), C.c_int(1), p(dx), p(dg), p(db),
                                                                               ops._stream()), 'wd_groupnorm_relu_bwd_nhwc_f32')]
        for i, fn in enumerate(calls):
            with pytest.raises(_lib.WaymoTrackError) as e:
                fn()
            assert 'WT_ERR_INVALID' in str(e.value) and words in str(e.value), (c, groups, h, w, i, str(e.value))
        assert bool((x == 1).all())                                            # nothing was written
    x, gamma, beta, gy = gn_inputs(256, 32, 5, 7, 7)
    _groupnorm_case('groupnorm after refused calls', x, gamma, beta, 32, True, gy)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. grid-stride loops
# (wd_bias_relu_f32 above 2048 workgroups and wd_act_bwd_f32 above 4096, with a ragged last round, are covered - and asserted - by
#  tests/test_gpu_backward_ops.py::test_bias_relu_is_exact / test_act_bwd_is_exact: 1100 x 2048 and 2100 x 2048 matrices.)

@pytest.mark.parametrize('n,c,h,w,stride', [(1, 64, 250, 240, 1), (2, 32, 345, 341, 2)])
def test_conv3x3_few_above_the_grid_cap(n, c, h, w, stride):
    """tap_shift_add_kernel launches at most 4096 workgroups = 1 048 576 threads: with more output elements its stride loop takes a second,
    ragged trip (asserted).  Against conv2d in float64, the bound of test_conv3x3_few_vs_conv2d."""
    from waymo_2d_tracking_amd.detnet.nn import ops
    ho, wo = out_size(h, stride), out_size(w, stride)
    total = n * ho * wo * 18
    assert 4096 * 256 < total < 2 * 4096 * 256 and total % 256 != 0, total
    g = torch.Generator().manual_seed(c + h)
    x = _cl(torch.randn(n, c, h, w, generator=g))
    wt = torch.randn(18, c, 3, 3, generator=g) * 0.05
    b = torch.randn(18, generator=g)
    got = ops.conv3x3_few(x, ops.tap_gemm_weight(wt.cuda()), b.cuda(), 18, stride)
    want = torch.nn.functional.conv2d(x.cpu().double(), wt.double(), b.double(), stride, 1)
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    err = (got.cpu().double() - want).abs().max().item() / max(1.0, want.abs().max().item())
    _ROWS.append(('conv3x3_few C=%d %dx%dx%d s%d (%d elements)' % (c, n, h, w, stride, total), err, 1e-4, err / 1e-4))
    assert err < 1e-4, err
