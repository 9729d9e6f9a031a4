"""Pure-Python helpers of tests/test_gpu_forward_ops.py (no device needed: tests/test_forward_shapes.py runs them on the CPU).

1. The launch rules of the two persistent forward kernels, restated, and a search for the smallest input that makes every workgroup walk
   several tiles.  The kernels size their grids from the device's CU count, so a fixed shape would stop covering their tile loops on a
   differently partitioned card.  If a launch rule changes, the restatement here changes with it (the GPU tests assert the conditions
   before every launch).

     grouped_conv3x3_c8_kernel (csrc/det_gconv.hip):  halves = C / 128, per_half = min(ceil(2 CUs / halves), ntiles) workgroups per half,
         workgroup i of a half takes tiles i, i + per_half, ...
     deform_conv3x3_pp_kernel (csrc/det_deform_pp.hip): items = C / 32, nsplit = min(max(CUs // items, 1), ceil(ntiles / 2)) workgroups per
         item, workgroup s takes a contiguous range of ntiles // nsplit (+ 1 for the first ntiles % nsplit) tiles in WORK ORDER (bands of
         two tile rows, pp_work_order); its two teams take alternate tiles of that range.

2. The inputs of the GroupNorm cases and the guard that keeps a rounding-decided ReLU mask out of the gradients.
"""
import torch

GCONV_MIN_TILES = 3          # tiles per workgroup the grouped-conv cases ask for
PP_MIN_TILES = 4             # tiles per TEAM the ping-pong cases ask for
MAX_INPUT_BYTES = 64 << 20
CU_COUNTS = (32, 64, 128, 256, 304)


def out_size(h, stride):
    return (h + 2 - 3) // stride + 1


def tiles(n):
    return (n + 7) // 8


def gconv_launch(cus, c, batch, h, w):
    """-> (ntiles, per_half, fewest tiles of a workgroup, most tiles of a workgroup)"""
    halves = c // 128
    ntiles = batch * tiles(h) * tiles(w)
    per_half = min((2 * cus + halves - 1) // halves, ntiles)
    per_half = max(per_half, 1)
    return ntiles, per_half, ntiles // per_half, (ntiles + per_half - 1) // per_half


def gconv_conditions(cus, c, batch, h, w):
    """The conditions of the multi-tile grouped-conv cases; a list of the ones that do not hold."""
    ntiles, per_half, lo, hi = gconv_launch(cus, c, batch, h, w)
    bad = []
    if h % 8 == 0 or w % 8 == 0:
        bad.append('H or W is a multiple of the tile')
    if tiles(h) < 3 or tiles(w) < 3:
        bad.append('no inner tile (fewer than 3 tile rows or columns)')
    if batch < 2:                # (tiles i, i + per_half, ...: with 3 of them a workgroup starts in the first image and ends in the last)
        bad.append('no workgroup crosses an image boundary')
    if lo < GCONV_MIN_TILES:
        bad.append('%d tiles per workgroup' % lo)
    if ntiles % per_half == 0:
        bad.append('tiles divide evenly over the workgroups')
    return bad


def pp_launch(cus, c, batch, h, w, stride):
    """-> (ntiles, nsplit, [tiles of team 0, tiles of team 1] of the workgroup with the fewest tiles, ... with the most)"""
    items = c // 32
    ntiles = batch * tiles(out_size(h, stride)) * tiles(out_size(w, stride))
    nsplit = min(max(cus // items, 1), (ntiles + 1) // 2)
    nsplit = max(nsplit, 1)
    lo, hi = ntiles // nsplit, (ntiles + nsplit - 1) // nsplit
    return ntiles, nsplit, ((lo + 1) // 2, lo // 2), ((hi + 1) // 2, hi // 2)


def pp_conditions(cus, c, batch, h, w, stride):
    ntiles, nsplit, lo, hi = pp_launch(cus, c, batch, h, w, stride)
    ho, wo = out_size(h, stride), out_size(w, stride)
    bad = []
    if h % 8 == 0 or w % 8 == 0 or ho % 8 == 0 or wo % 8 == 0:
        bad.append('H, W, Ho or Wo is a multiple of the tile')
    if tiles(ho) < 3 or tiles(wo) < 3:
        bad.append('no inner tile (fewer than 3 tile rows or columns)')
    per_image = tiles(ho) * tiles(wo)
    tq, trm = divmod(ntiles, nsplit)
    starts = {s * tq + min(s, trm) for s in range(nsplit)}           # first tile of every workgroup's contiguous range
    if batch < 2 or all(k * per_image in starts for k in range(1, batch)):
        bad.append('no workgroup crosses an image boundary')
    if lo[1] < PP_MIN_TILES:
        bad.append('%d tiles on team 1 of the smallest workgroup' % lo[1])
    # uneven: workgroups of two sizes; with ONE workgroup per item (few CUs) the split that can be uneven is the one between its teams
    if (ntiles % nsplit == 0) if nsplit > 1 else (ntiles % 2 == 0):
        bad.append('tiles divide evenly')
    return bad


def _search(conditions, c, stride, input_bytes):
    """Smallest (batch, H, W) by input size: batch 2 to 4, H <= W <= H + 16 (near-square maps, like the detector's)."""
    best = None
    for batch in (2, 3, 4):
        for h in range(17, 400):
            if best is not None and input_bytes(batch, h, h) >= best[0]:
                break
            for w in range(h, h + 17):
                size = input_bytes(batch, h, w)
                if best is not None and size >= best[0]:
                    break
                if not conditions(batch, h, w):
                    best = (size, batch, h, w)
                    break
    assert best is not None, (c, stride)
    return best[1:]


def gconv_shape(cus, c):
    return _search(lambda b, h, w: gconv_conditions(cus, c, b, h, w), c, 1, lambda b, h, w: 4 * b * h * w * c)


def pp_shape(cus, c, stride):
    return _search(lambda b, h, w: pp_conditions(cus, c, b, h, w, stride), c, stride, lambda b, h, w: 4 * b * h * w * c)


def pp_work_order(batch, ho, wo):
    """Work-order tile number -> (image, tile row, tile column) of the ping-pong kernel (tile_of in csrc/det_deform_pp.hip): bands of two tile rows,
    column by column inside a band; a last single row runs left to right."""
    ty_n, tx_n = tiles(ho), tiles(wo)
    order = []
    for t in range(batch * ty_n * tx_n):
        tn, rem = divmod(t, ty_n * tx_n)
        band, rb = divmod(rem, 2 * tx_n)
        if 2 * band + 1 < ty_n:
            order.append((tn, 2 * band + (rb & 1), rb >> 1))
        else:
            order.append((tn, 2 * band, rb))
    return order


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm cases

GN_CONFIGS = [(64, 16), (64, 2), (128, 8), (256, 32), (256, 16), (320, 20), (512, 32), (512, 16)]      # (C, groups): 4, 32, 16, 8, 16, 16, 16, 32 per group
GN_SPATIAL = [(1, 1), (1, 2), (7, 7), (7, 9), (8, 8)]
GN_ROIS = [1, 5, 64]
GN_GUARD_ULPS = 64
GN_GUARD_SHARE = 1e-3


def gn_inputs(c, groups, r, h, w):
    """x, gamma, beta, gy (float32, CPU) of one GroupNorm case.  |beta| >= 0.1: the pre-activation gamma xh + beta is then near zero only where
    gamma xh is of that size too, so the guard below (relative to |gamma xh| + |beta|) is at least 64 x 2^-23 x 0.1 = 7.6e-7 wide, ten times what
    float32 statistics move a pre-activation by (~2^-23 (|gamma xh| + gamma |mean| rstd), a few 1e-8 with mean 0.5 and deviation 2)."""
    g = torch.Generator().manual_seed(c * 1000 + groups * 100 + r * 10 + h * w)
    x = torch.randn((r, c, h, w), generator=g) * 2 + 0.5
    gamma = torch.rand(c, generator=g) + 0.5
    beta = (torch.rand(c, generator=g) * 0.3 + 0.1) * torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)
    gy = torch.randn((r, c, h, w), generator=g)
    return x, gamma, beta, gy


def gn_reference(x, gamma, beta, groups, relu, gy, guard=True):
    """float64 torch.nn.functional.group_norm (+ relu) with autograd -> (y, dx, dgamma, dbeta, gy used, share of gy zeroed by the guard).
    Guard (relu only): gy is zeroed where the float64 pre-activation lies within GN_GUARD_ULPS float32 ulps of |gamma xh| + |beta| of zero - the
    backward kernel decides the ReLU mask from its own float32 pre-activation, and ONE flipped mask would move dgamma / dbeta of a channel."""
    xr, wr, br = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    z = torch.nn.functional.group_norm(xr, groups, wr, br, 1e-5)
    share = 0.0
    if relu and guard and x.numel():
        zd = z.detach()
        b = beta.double().view(1, -1, 1, 1)
        tol = GN_GUARD_ULPS * 2.0 ** -23 * ((zd - b).abs() + b.abs())
        near = zd.abs() < tol
        share = float(near.double().mean())
        gy = torch.where(near, torch.zeros_like(gy), gy)
    y = torch.relu(z) if relu else z
    y.backward(gy.double())
    return y.detach(), xr.grad, wr.grad, br.grad, gy, share
