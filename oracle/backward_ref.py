"""TEST INFRASTRUCTURE ONLY - CPU helpers of the op-level backward tests (tests/test_gpu_backward_ops.py, tests/test_oracle_backward_ref.py).

  * reference gradients of the deformable convolution and of ROIAlign by torch autograd through the restatements in oracle/detector_ref.py
    (grid_sample based) and oracle/detops_ref.py (explicit floor-cell gather), in float64 or - to measure what float32 itself costs - float32;
  * the sampling geometry of the fused backward kernels restated from the offsets alone (which samples leave the 14 x 14 patch of their tile,
    which touch pixels outside the image), and the level / footprint of a ROI in the kernels' float32 arithmetic: the tests assert from these
    that an input really takes the code path it is meant for;
  * builders of offset fields (exactly representable, convergent, integer).
Never imported by the product package.
"""
import torch

from . import detector_ref, detops_ref


def exact_offsets(offset, on_grid=False):
    """Round an offset field to ODD multiples of 1/1024 (on_grid: to multiples of 1/1024).  With |offset| < 64 and maps below 8192 pixels the
    sampling position base + offset is then exact in float32, so kernel (float32) and reference (float64) see the same position, the same cell
    and the same fractions, and an odd multiple is never an integer: the position stays off the kinks of the bilinear surface."""
    q = torch.round(offset.double() * 512)
    q = q * 2 if on_grid else q * 2 + 1
    return (q / 1024).to(offset.dtype)


def deform_positions(offset, stride, pad=1):
    """(h_im, w_im), each (N, 9, Ho, Wo) float64: the sampling position of every (output pixel, tap)."""
    off = offset.detach().double()
    n, _, ho, wo = off.shape
    ys = torch.arange(ho, dtype=torch.float64).view(1, 1, ho, 1) * stride - pad
    xs = torch.arange(wo, dtype=torch.float64).view(1, 1, 1, wo) * stride - pad
    kh = (torch.arange(9) // 3).double().view(1, 9, 1, 1)
    kw = (torch.arange(9) % 3).double().view(1, 9, 1, 1)
    return ys + kh + off[:, 0::2], xs + kw + off[:, 1::2]


def deform_sample_shares(offset, h, w, stride):
    """Shares of the (output pixel, tap) samples, by the rules of the fused backward kernels (fb_entry in csrc/det_deform_bwd.hip):
      far      the sample counts (inside (-1, H) x (-1, W)) and the cell of its upper-left corner is not inside 0 .. 12 of the tile's 14 x 14 patch
               (origin = image pixel 8 S t - 3 for stride 1, 16 t + 1 for stride 2): it goes through the far passes;
      outside  the sample has at least one corner outside the image (a sample that does not count at all included);
      far_outside  both at once (a far sample with a corner outside the image);
      max_list the largest number of (sample, corner) pairs with a non-zero weight on one input pixel from one tile (length of an inverted list).
    """
    hi, wi = deform_positions(offset, stride)
    n, _, ho, wo = hi.shape
    counts = (hi > -1) & (wi > -1) & (hi < h) & (wi < w)
    hl, wl = torch.floor(hi), torch.floor(wi)
    org = 3 if stride == 1 else -1
    ty = (torch.arange(ho) // 8).double().view(1, 1, ho, 1)
    tx = (torch.arange(wo) // 8).double().view(1, 1, 1, wo)
    ph, pw = hl - (stride * 8 * ty - org), wl - (stride * 8 * tx - org)
    in_patch = (ph >= 0) & (ph <= 12) & (pw >= 0) & (pw <= 12)
    corner_out = (hl < 0) | (hl + 1 > h - 1) | (wl < 0) | (wl + 1 > w - 1)
    far = counts & ~in_patch
    outside = ~counts | corner_out
    total = float(counts.numel())
    # inverted lists: per tile and input pixel the number of corners with a non-zero weight
    lh, lw = hi - hl, wi - wl
    tiles_x = (wo + 7) // 8
    tile = (torch.arange(n).view(n, 1, 1, 1) * ((ho + 7) // 8) + ty.long()) * tiles_x + tx.long()
    longest = 0
    for dy, dx, wgt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        yy, xx = (hl + dy).long(), (wl + dx).long()
        ok = counts & (wgt != 0) & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        if ok.any():
            key = (tile.expand_as(yy)[ok] * h + yy[ok]) * w + xx[ok]
            longest = max(longest, int(torch.bincount(key).max()))
    return {'far': float(far.sum()) / total, 'outside': float(outside.sum()) / total, 'far_outside': float((far & corner_out).sum()) / total,
            'counts': float(counts.sum()) / total, 'max_list': longest}


def convergent_offsets(n, h, w, stride, targets, jitter, generator, per_tap=False):
    """Offsets that aim EVERY sample of an 8 x 8 output tile (ty, tx) at one bilinear cell: targets[(ty + tx) % len(targets)] = (a, b) means the
    input position (8 S ty + a, 8 S tx + b), None a position outside the image (-6, -9: the sample does not count, every inverted list of such
    a tile is empty); plus a fractional jitter in (0, jitter).  per_tap: the target also cycles with the tap index, so a tile piles its samples
    on len(targets) cells."""
    ho, wo = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
    base_h, base_w = deform_positions(torch.zeros((n, 18, ho, wo)), stride)
    ty = (torch.arange(ho) // 8).view(1, 1, ho, 1)
    tx = (torch.arange(wo) // 8).view(1, 1, 1, wo)
    which = (ty + tx + (torch.arange(9).view(1, 9, 1, 1) if per_tap else 0)) % len(targets)
    which = which.expand(n, 9, ho, wo)
    rel = torch.tensor([0.0 if t is None else 1.0 for t in targets], dtype=torch.float64)[which]
    ta = torch.tensor([-6.0 if t is None else t[0] for t in targets], dtype=torch.float64)[which] + rel * (8 * stride * ty)
    tb = torch.tensor([-9.0 if t is None else t[1] for t in targets], dtype=torch.float64)[which] + rel * (8 * stride * tx)
    off = torch.zeros((n, 18, ho, wo), dtype=torch.float64)
    off[:, 0::2] = ta - base_h + torch.rand((n, 9, ho, wo), generator=generator).double() * jitter
    off[:, 1::2] = tb - base_w + torch.rand((n, 9, ho, wo), generator=generator).double() * jitter
    return exact_offsets(off.float())


def deform_columns(x, offset, stride, dtype=torch.float64):
    """(N, C, 9, Ho, Wo): the sampled value of every (channel, tap, output pixel) - the im2col slab, by grid_sample like detector_ref."""
    import torch.nn.functional as F
    n, c, h, w = x.shape
    hi, wi = deform_positions(torch.zeros_like(offset), stride)
    taps = []
    for k in range(9):
        py, px = hi[:, k].to(dtype) + offset[:, 2 * k].to(dtype), wi[:, k].to(dtype) + offset[:, 2 * k + 1].to(dtype)
        grid = torch.stack((2 * px / max(w - 1, 1) - 1, 2 * py / max(h - 1, 1) - 1), dim=-1)
        taps.append(F.grid_sample(x.to(dtype), grid, mode='bilinear', padding_mode='zeros', align_corners=True))
    return torch.stack(taps, dim=2)


def deform_grads(x, offset, weight, groups, stride, gy, scale=None, bias=None, relu=False, dtype=torch.float64, floor_rule=False, kink_guard=None):
    """(y, dX, dOffset, dW) of y = [relu](DeformConv(x, offset; weight) [* scale + bias]) for the output gradient gy, by autograd in `dtype`.
    floor_rule=False: oracle/detector_ref.deform_conv3x3 (grid_sample); True: oracle/detops_ref.deform_conv3x3 - the explicit restatement of
    detectron2's rule (the sample counts inside the OPEN interval (-1, size), cell = floor(position), derivative taken inside that cell), which is
    what the kernels implement where a position is an exact integer (float64 only).  It is also the reference for maps with H = 1 or W = 1,
    which grid_sample's align_corners mapping cannot express (2 p / max(size - 1, 1) - 1 sends every position of a one-pixel axis to pixel 0).
    kink_guard (with relu): gy is set to zero wherever the pre-activation lies within kink_guard of 0 - there the ReLU mask of a float32 forward
    is a coin toss and one flipped mask moves a gradient entry by a finite step; the gy actually used is returned as a fifth element, to be fed
    to the code under test (and to a second run of this function) in place of gy."""
    xr = x.detach().to(dtype).clone().requires_grad_()
    orf = offset.detach().to(dtype).clone().requires_grad_()
    wr = weight.detach().to(dtype).clone().requires_grad_()
    if floor_rule:
        assert dtype == torch.float64
        y = detops_ref.deform_conv3x3(xr, orf, wr, groups, stride, 1)
    else:
        y = detector_ref.deform_conv3x3(xr, orf, wr, groups, stride, 1)
    if scale is not None:
        y = y * scale.to(dtype).view(1, -1, 1, 1) + bias.to(dtype).view(1, -1, 1, 1)
    if relu and kink_guard is not None:
        gy = gy * (y.detach().abs() >= kink_guard).to(gy.dtype)
    if relu:
        y = torch.relu(y)
    y.backward(gy.to(dtype))
    return (y.detach(), xr.grad, orf.grad, wr.grad) + ((gy,) if kink_guard is not None else ())


def roi_grads(feats, rois, scales, gout, pooled=7, dtype=torch.float64):
    """(out, [dFeat per level]) of the batch-aware ROIAlign restatement; a level that no ROI uses gets a zero gradient."""
    fr = [f.detach().to(dtype).clone().requires_grad_() for f in feats]
    out = detector_ref.roi_pool_fpn_batched(fr, rois, scales, pooled)
    out.backward(gout.to(dtype))
    return out.detach(), [f.grad if f.grad is not None else torch.zeros_like(f) for f in fr]


def roi_geometry(rois, scales, sizes, min_level=2, canonical_level=4, canonical_size=224.0):
    """Level index (0-based) and footprint (rows, columns) of every ROI in the float32 arithmetic of roi_pool_fpn_bwd_kernel; sizes = [(H, W)] per
    level.  The separable kernel holds footprints up to 192 x 192 cells, larger ones take the per-sample form."""
    r = rois.float()
    size = torch.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2]))
    lvl = torch.floor(canonical_level + torch.log2(size / canonical_size + 1e-8)).clamp(min_level, min_level + len(scales) - 1).long() - min_level
    sc = torch.tensor([float(s) for s in scales], dtype=torch.float32)[lvl]
    hh = torch.tensor([s[0] for s in sizes])[lvl]
    ww = torch.tensor([s[1] for s in sizes])[lvl]
    rsw, rsh = r[:, 1] * sc - 0.5, r[:, 2] * sc - 0.5
    roi_w, roi_h = (r[:, 3] * sc - 0.5) - rsw, (r[:, 4] * sc - 0.5) - rsh
    zero = torch.zeros_like(hh)
    r0 = torch.maximum(zero, torch.minimum(hh - 1, torch.floor(rsh).long()))
    c0 = torch.maximum(zero, torch.minimum(ww - 1, torch.floor(rsw).long()))
    r1 = torch.maximum(r0, torch.minimum(hh - 1, torch.floor(rsh + roi_h).long() + 1))
    c1 = torch.maximum(c0, torch.minimum(ww - 1, torch.floor(rsw + roi_w).long() + 1))
    return lvl, r1 - r0 + 1, c1 - c0 + 1


def rel_err(a, b):
    """max|a - b| / max|b| (the measure of the existing deformable backward test)."""
    return (a.double() - b.double()).abs().max().item() / (b.double().abs().max().item() + 1e-12)
