"""CPU checks of tests/forward_shapes.py: the shapes the forward op tests (tests/test_gpu_forward_ops.py) pick for a card's CU count meet the
conditions those tests assert before launching, for differently partitioned cards, and the GroupNorm ReLU-mask guard zeroes a negligible share of
the incoming gradient on every case (float64 reference alone)."""
import pytest

import forward_shapes as F


@pytest.mark.parametrize('cus', F.CU_COUNTS)
def test_multi_tile_shapes_meet_their_conditions(cus):
    for c in (128, 256, 384):
        n, h, w = F.gconv_shape(cus, c)
        assert F.gconv_conditions(cus, c, n, h, w) == []
        ntiles, per_half, lo, hi = F.gconv_launch(cus, c, n, h, w)
        assert n >= 2 and h % 8 and w % 8
        assert lo >= F.GCONV_MIN_TILES and hi == lo + 1 and ntiles % per_half          # 3 or more per workgroup, the last round ragged
        assert per_half == -(-2 * cus // (c // 128))                                    # the grid is at its CU-count cap, not at ntiles
        assert 4 * n * c * h * w <= F.MAX_INPUT_BYTES
        assert F.gconv_conditions(cus, c, n, h, w + (8 - w % 8)) and F.gconv_conditions(cus, c, 1, h, w)      # the conditions do reject
    for c, stride in ((1024, 1), (1024, 2), (512, 2)):
        n, h, w = F.pp_shape(cus, c, stride)
        assert F.pp_conditions(cus, c, n, h, w, stride) == []
        ntiles, nsplit, lo, hi = F.pp_launch(cus, c, n, h, w, stride)
        ho, wo = F.out_size(h, stride), F.out_size(w, stride)
        assert n >= 2 and h % 8 and w % 8 and ho % 8 and wo % 8
        assert min(lo) >= F.PP_MIN_TILES                                                 # both teams of the smallest workgroup
        assert nsplit == max(cus // (c // 32), 1)
        assert (ntiles % nsplit) if nsplit > 1 else (ntiles % 2)
        assert 4 * n * c * h * w <= F.MAX_INPUT_BYTES
        assert F.pp_conditions(cus, c, 1, h, w, stride)


def test_launch_rules_on_known_shapes():
    """The restated rules on shapes whose launch is known from the kernels' sources: the parent suite's 19 x 23 batch 2 grouped conv is one tile per
    workgroup on any card with 9 or more CUs; res4 at 80 x 120 on 256 CUs is 150 tiles over 8 workgroups per item."""
    assert F.gconv_launch(256, 256, 2, 19, 23) == (18, 18, 1, 1)
    assert F.gconv_launch(4, 256, 2, 19, 23) == (18, 4, 4, 5)
    assert F.pp_launch(256, 1024, 1, 80, 120, 1) == (150, 8, (9, 9), (10, 9))
    assert F.pp_launch(256, 512, 2, 21, 30, 2) == (8, 4, (1, 1), (1, 1))
    assert F.pp_launch(256, 1024, 1, 8, 8, 1) == (1, 1, (1, 0), (1, 0))


def test_pingpong_work_order_visits_every_tile_once_in_bands():
    for n, ho, wo in ((1, 8, 8), (2, 17, 33), (3, 40, 25), (2, 9, 9)):
        order = F.pp_work_order(n, ho, wo)
        assert sorted(order) == [(i, y, x) for i in range(n) for y in range(F.tiles(ho)) for x in range(F.tiles(wo))]
    # 3 tile rows x 2 columns: a band of two rows column by column, then the single last row
    assert F.pp_work_order(1, 17, 9) == [(0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (0, 2, 0), (0, 2, 1)]


@pytest.mark.parametrize('c,groups', F.GN_CONFIGS)
def test_groupnorm_guard_zeroes_a_negligible_share(c, groups):
    assert {cc // gg for cc, gg in F.GN_CONFIGS} == {4, 8, 16, 32}
    assert any(cc > 256 and cc % 256 == 64 for cc, _ in F.GN_CONFIGS) and any(cc == 512 for cc, _ in F.GN_CONFIGS)
    for r in F.GN_ROIS:
        for h, w in F.GN_SPATIAL:
            x, gamma, beta, gy = F.gn_inputs(c, groups, r, h, w)
            assert float(beta.abs().min()) >= 0.1
            share = F.gn_reference(x, gamma, beta, groups, True, gy)[5]
            assert share <= F.GN_GUARD_SHARE, (c, groups, r, h, w, share)
