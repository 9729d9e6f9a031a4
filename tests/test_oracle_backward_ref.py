"""CPU checks of the references behind tests/test_gpu_backward_ops.py (oracle/detector_ref.py, oracle/backward_ref.py): no GPU needed.
A reference that is wrong makes every kernel test above it worthless, so the restatements are pinned to each other, to torch's own
finite-difference gradcheck and to conv2d."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import backward_ref as B
from oracle import detector_ref as R
from oracle import detops_ref as D

STRIDES = [4, 8, 16, 32]
SCALES = [1.0 / s for s in STRIDES]


def _rois(g, n_img, h, w, count):
    rows = []
    for i in range(count):
        size = (8, 20, 60, 120, 250, 600)[i % 6]
        bw = size * float(torch.empty(1).uniform_(0.5, 2.0, generator=g))
        bh = size * float(torch.empty(1).uniform_(0.5, 2.0, generator=g))
        x1 = float(torch.empty(1).uniform_(-20, w - 10, generator=g))
        y1 = float(torch.empty(1).uniform_(-20, h - 10, generator=g))
        rows.append([float(i % n_img), x1, y1, x1 + bw, y1 + bh])
    return torch.tensor(rows, dtype=torch.float32)


@pytest.mark.parametrize('pooled', [7, 3])
def test_batched_roi_reference_equals_per_image_calls_and_the_loop_restatement(pooled):
    g = torch.Generator().manual_seed(pooled)
    h, w, c, n = 128, 192, 12, 3
    feats = [torch.randn((n, c, h // s, w // s), generator=g).double() for s in STRIDES]
    rois = _rois(g, n, h, w, 24)
    rois[5, 0] = -1.0                                       # outside [0, N): zeros
    rois[6, 0] = float(n)
    got = R.roi_pool_fpn_batched(feats, rois, SCALES, pooled)
    assert got.shape == (24, c, pooled, pooled)
    assert not got[5].any() and not got[6].any()
    valid = torch.ones(24, dtype=torch.bool)
    valid[5] = valid[6] = False
    for b in range(n):                                      # the old single-image form on a one-image batch
        sel = torch.nonzero(valid & (rois[:, 0] == b)).flatten()
        one = R.roi_pool_fpn([f[b:b + 1] for f in feats], rois[sel, 1:], SCALES, pooled)
        assert torch.equal(got[sel], one)
    loop, lv = D.roi_pool_fpn(feats, rois[valid], SCALES, pooled)       # the scalar loop restatement (float32 coordinates, float64 sums)
    assert len(set(lv.tolist())) == 4
    # the vectorised form multiplies its bilinear weights in float32 like the kernel (2^-24 relative each), the loop in float64
    np.testing.assert_allclose(got[valid].numpy(), loop.numpy(), rtol=0, atol=4 * 2.0 ** -24 * float(loop.abs().max()))
    lvl, nr, nc = B.roi_geometry(rois[valid], SCALES, [(h // s, w // s) for s in STRIDES])
    assert torch.equal(lvl + 2, lv) and int(nr.min()) >= 1 and int(nc.min()) >= 1


def test_batched_roi_reference_sends_no_gradient_for_bad_indices():
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn((2, 4, 64 // s, 96 // s), generator=g) for s in STRIDES]
    rois = torch.tensor([[0.0, 4.0, 6.0, 40.0, 30.0], [2.0, 4.0, 6.0, 40.0, 30.0], [-1.0, 1.0, 1.0, 90.0, 60.0], [1.0, 10.0, 3.0, 50.0, 44.0]])
    gout = torch.randn((4, 4, 7, 7), generator=g)
    _, grads = B.roi_grads(feats, rois, SCALES, gout)
    gout2 = gout.clone()
    gout2[1] = 7.0
    gout2[2] = -3.0
    _, grads2 = B.roi_grads(feats, rois, SCALES, gout2)
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)
    assert any(bool(a[0].any()) for a in grads) and any(bool(a[1].any()) for a in grads)


def test_roi_reference_gradcheck():
    """float64 finite differences through the batched ROIAlign restatement; box corners chosen so that no sample sits on an integer."""
    g = torch.Generator().manual_seed(2)
    feats = [torch.randn((2, 2, 32 // s, 48 // s), generator=g).double().requires_grad_() for s in (4, 8)]
    rois = torch.tensor([[0.0, 3.3, 2.1, 20.7, 17.9], [1.0, -2.2, 5.3, 30.1, 40.9], [1.0, 8.1, 1.7, 11.3, 4.9]])
    for pooled in (2, 3):
        assert torch.autograd.gradcheck(lambda a, b: R.roi_pool_fpn_batched([a, b], rois, [0.25, 0.125], pooled, 2, 4, 56.0), feats, eps=1e-6,
                                        atol=1e-7)


@pytest.mark.parametrize('stride', [1, 2])
def test_deform_reference_gradcheck(stride):
    g = torch.Generator().manual_seed(stride)
    h, w = 5, 6
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = torch.randn((2, 4, h, w), generator=g).double().requires_grad_()
    off = B.exact_offsets(torch.randn((2, 18, ho, wo), generator=g) * 1.5).double().requires_grad_()       # off integers, some outside the image
    wt = torch.randn((4, 2, 3, 3), generator=g).double().requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b, c: R.deform_conv3x3(a, b, c, 2, stride, 1), (x, off, wt), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda a, b, c: D.deform_conv3x3(a, b, c, 2, stride, 1), (x, off, wt), eps=1e-6, atol=1e-7)
    # a one-pixel axis (the floor-cell restatement only: grid_sample's align_corners mapping cannot express it)
    x1 = torch.randn((1, 4, 1, 5), generator=g).double().requires_grad_()
    off1 = B.exact_offsets(torch.randn((1, 18, 1, (5 - 1) // stride + 1), generator=g) * 0.8).double().requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b, c: D.deform_conv3x3(a, b, c, 2, stride, 1), (x1, off1, wt), eps=1e-6, atol=1e-7)


@pytest.mark.parametrize('cg,stride', [(16, 1), (32, 2), (64, 1)])
def test_zero_offset_deform_backward_equals_conv2d_backward(cg, stride):
    g = torch.Generator().manual_seed(cg)
    c, h, w = 2 * cg, 7, 9
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = torch.randn((2, c, h, w), generator=g)
    wt = torch.randn((c, cg, 3, 3), generator=g)
    gy = torch.randn((2, c, ho, wo), generator=g)
    _, dx, _, dw = B.deform_grads(x, torch.zeros((2, 18, ho, wo)), wt, 2, stride, gy)
    xr, wr = x.double().requires_grad_(), wt.double().requires_grad_()
    F.conv2d(xr, wr, None, stride, 1, 1, 2).backward(gy.double())
    np.testing.assert_allclose(dx.numpy(), xr.grad.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(dw.numpy(), wr.grad.numpy(), rtol=1e-10, atol=1e-10)


def test_grid_sample_and_floor_rule_restatements_agree_off_integers_and_differ_on_them():
    """Off integer positions the two restatements are the same function.  ON them the value (dX, dW) is still the same, but dOffset is a one-sided
    derivative: the floor-cell rule (detectron2, the kernels) always takes the cell [floor, floor + 1); grid_sample maps the position to [-1, 1]
    and back first, and that round trip can land an ulp below the integer (the other side), and it counts a sample at exactly -1 that
    detectron2's open interval drops.  This test records that the sides do differ - the reason the GPU test compares dOffset at integer
    positions with the floor-rule restatement."""
    g = torch.Generator().manual_seed(7)
    h, w = 9, 11
    x = torch.randn((1, 8, h, w), generator=g)
    wt = torch.randn((8, 4, 3, 3), generator=g)
    gy = torch.randn((1, 8, h, w), generator=g)
    off = B.exact_offsets(torch.randn((1, 18, h, w), generator=g) * 2.0)
    a = B.deform_grads(x, off, wt, 2, 1, gy)
    b = B.deform_grads(x, off, wt, 2, 1, gy, floor_rule=True)
    for u, v in zip(a, b):
        np.testing.assert_allclose(u.numpy(), v.numpy(), rtol=1e-9, atol=1e-9)
    ioff = torch.randint(-3, 4, (1, 18, h, w), generator=g).float()
    a = B.deform_grads(x, ioff, wt, 2, 1, gy)
    b = B.deform_grads(x, ioff, wt, 2, 1, gy, floor_rule=True)
    for k in (0, 1, 3):                                     # y, dX, dW: continuous in the position
        np.testing.assert_allclose(a[k].numpy(), b[k].numpy(), rtol=1e-9, atol=1e-9)
    assert B.rel_err(a[2], b[2]) > 1e-3                     # dOffset: not the same side everywhere


def test_sample_shares_and_offset_builders():
    g = torch.Generator().manual_seed(3)
    z = torch.zeros((1, 18, 16, 16))
    s = B.deform_sample_shares(z, 16, 16, 1)
    assert s['far'] == 0.0 and abs(s['counts'] - (46 / 48) ** 2) < 1e-12 and s['max_list'] == 9      # an interior pixel of a 3 x 3 convolution is read by 9 samples
    # per axis 4 of the 48 (pixel, tap) positions are -1, 15 or 16: no count, or the lower / right corner is row / column 16
    assert abs(s['outside'] - (1 - (44 / 48) ** 2)) < 1e-12
    s2 = B.deform_sample_shares(torch.zeros((1, 18, 8, 8)), 16, 16, 2)
    # stride 2, one tile: positions -1 .. 15 per axis (24 of them); -1 does not count, 0, 14 and 15 lie outside the patch cells 1 .. 13
    assert abs(s2['far'] - ((23 / 24) ** 2 - (20 / 24) ** 2)) < 1e-12
    big = B.exact_offsets(torch.randn((1, 18, 16, 16), generator=g) * 6.0)
    s3 = B.deform_sample_shares(big, 16, 16, 1)
    assert s3['far'] > 0.1 and s3['outside'] > 0.2 and s3['far_outside'] > 0.0
    frac = (big.double() * 1024) % 2
    assert bool((frac == 1).all())                                             # odd multiples of 1/1024: never an integer
    conv = B.convergent_offsets(1, 16, 16, 1, [(3.0, 4.0), None], 0.5, g)       # tiles (0,0), (1,1): cell (3, 4) of the tile; the others: outside
    hi, wi = B.deform_positions(conv, 1)
    cells = set(zip(torch.floor(hi).flatten().tolist(), torch.floor(wi).flatten().tolist()))
    assert cells == {(3.0, 4.0), (11.0, 12.0), (-6.0, -9.0)}
    s4 = B.deform_sample_shares(conv, 16, 16, 1)
    assert s4['max_list'] == 576 and abs(s4['counts'] - 0.5) < 1e-12 and s4['far'] == 0.0
    two = B.convergent_offsets(1, 16, 16, 1, [(3.0, 4.0), (6.0, 2.0)], 0.5, g, per_tap=True)
    assert B.deform_sample_shares(two, 16, 16, 1)['max_list'] in (256, 320)      # 4 or 5 of the 9 taps on each of the two cells


def test_roi_geometry_matches_hand_computed_footprints():
    sizes = [(320, 480), (160, 240), (80, 120), (40, 60)]
    rois = torch.tensor([[0.0, 10.0, 100.0, 1910.0, 120.0],        # 1900 x 20: sqrt(38000) = 195 -> p3; columns floor(0.75) .. floor(238.25) + 1 = 0 .. 239
                         [0.0, 100.0, 5.0, 109.0, 1275.0],         # 9 x 1270: sqrt(11430) = 107 -> p2; rows floor(0.75) .. floor(318.25) + 1 = 0 .. 319
                         [0.0, 84.0, 40.0, 1608.0, 60.0],          # p3, columns 10 .. 201: 192 (the largest the separable kernel holds)
                         [0.0, 84.0, 40.0, 1616.0, 60.0]])         # columns 10 .. 202: 193
    lvl, nr, nc = B.roi_geometry(rois, SCALES, sizes)
    assert lvl.tolist() == [1, 0, 1, 1]
    assert nc.tolist()[0] == 240 and nr.tolist()[1] == 320 and nc.tolist()[2:] == [192, 193]
