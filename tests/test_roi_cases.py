"""CPU checks of tests/roi_cases.py: every class of ROI the GPU tests rely on is there, every case does what it was built for, every
expected value is exact in float32, and the restated launch rules are self-consistent."""
import numpy as np
import pytest
import torch

import roi_cases as RC


def _all_cases():
    return [c for scene in RC.SCENES for c in RC.cases(scene)]


def test_every_class_is_present():
    cs = _all_cases()
    intents = set().union(*[c.intents for c in cs])
    facts = set().union(*[c.facts for c in cs])
    assert not [t for t in RC.REQUIRED_INTENTS if t not in intents]
    assert not [t for t in RC.REQUIRED_FACTS if t not in facts]
    assert sum(len(RC.cases(s)) for s in RC.SCENES) <= 150


def test_cases_do_what_they_were_built_for():
    for c in _all_cases():
        for t in c.intents:
            if t.startswith(RC.CHECKED_INTENTS):
                assert t in c.facts, (c.name, t, sorted(c.facts))
        assert all(np.isfinite(v) and abs(v) <= 4000 for v in c.roi), c.name
    by_name = {c.name: c for c in RC.cases('main')}
    for place in ('integer', 'half'):
        g9, g10 = by_name['limit 9x9 %s' % place].geom, by_name['limit 10x10 %s' % place].geom
        assert (g9.nrows, g9.ncols, g9.path, g9.sep_path) == (64, 64, 'fold', 'table')
        assert (g10.nrows, g10.ncols, g10.path, g10.sep_path) == (71, 71, 'direct', 'flagged')
        for name, rows, cols in (('9x1', 64, 8), ('10x1', 71, 8), ('1x9', 8, 64), ('1x10', 8, 71)):
            g = by_name['limit %s %s' % (name, place)].geom
            assert (g.nrows, g.ncols) == (rows, cols) and (g.path == 'direct') == (max(rows, cols) > 64), name
    # integer placement: every sample sits on a pixel, so the footprint's last column carries no weight
    g = by_name['bins 2x2 integer'].geom
    assert g.col_pa[-1] == 7 and all(pa < 7 for pa in g.col_pa[:-1])
    assert all(pa < 7 for pa in by_name['bins 2x2 half'].geom.col_pa)
    # the tail forms come from the footprint widths the issue names: 8 | 15 | 29 | 57 | 64 columns
    assert [RC.tail_form(n) for n in (8, 15, 29, 57, 64, 4, 5)] == ['full', 'partial', 'partial', 'half', 'full', 'half', 'partial']
    assert {by_name['bins 1x%d half' % b].geom.ncols for b in (1, 2, 4, 8)} == {8, 15, 29, 57}
    # a 0.75 bin feeds exactly three bins per column at most, 0.5 and 0.25 more
    assert by_name['narrow 0.75x0.75 #0'].geom.spread == 2 and by_name['narrow 0.5x0.5 #0'].geom.spread > 2
    # level edges: the box of geometric mean exactly 112 / 224 / 448 belongs to the upper level, a slightly smaller one to the lower
    for edge, level in ((112, 1), (224, 2), (448, 3)):
        assert RC.level_index((0., 0., 0., float(edge), float(edge))) == level
        assert RC.level_index((0., 0., 0., float(edge), float(edge) - .5)) == level - 1
    # the two images give different answers for the same box, the out-of-batch indices zeros
    exp, _ = RC.expected('main')
    idx = {c.name: i for i, c in enumerate(RC.cases('main'))}
    assert not torch.equal(exp[idx['image 0']], exp[idx['image 1']])
    assert not exp[idx['image -1']].any() and not exp[idx['image 2']].any()
    assert exp[idx['image 0']].any()
    for name in ('empty box', 'zero width', 'negative width', 'negative width and height', 'outside right', 'outside below'):
        assert not exp[idx[name]].any(), name


@pytest.mark.parametrize('scene', list(RC.SCENES))
@pytest.mark.parametrize('pooled', [7, 3, 14])
def test_expected_values_are_exact_in_float32(scene, pooled):
    """The float64 reference round-trips through float32 unchanged; where gh * gw is no power of two, the undivided sum does."""
    cs = RC.cases(scene, pooled)
    assert len(cs) >= (8 if scene == 'tiny' else 40)
    exp, rounds = RC.expected(scene, pooled)
    assert exp.shape == (len(cs), 8, pooled, pooled) and torch.isfinite(exp).all()
    assert torch.equal(exp[~rounds].float().double(), exp[~rounds])
    count = torch.tensor([float(c.geom.count) for c in cs], dtype=torch.float64).view(-1, 1, 1, 1)
    total = exp * count * 64                                    # weights are multiples of 1 / 64: the undivided sum is an integer of them
    assert (total - total.round()).abs().max() < 1e-6 and total.abs().max() < 2 ** 24
    if pooled == 7 and scene == 'main':
        assert bool(rounds.any()) and bool((~rounds).any())
        assert (exp.abs().amax(dim=(1, 2, 3)) > 0).sum() >= len(cs) // 2
    # the reference assigns every valid, non-degenerate ROI to the level the restatement predicts
    from oracle import detops_ref as R
    lv = R.assign_levels(RC.rois_of(cs), RC.MIN_LEVEL, RC.MIN_LEVEL + 3, RC.CANONICAL_LEVEL, RC.CANONICAL_SIZE)
    for c, l in zip(cs, lv.tolist()):
        if 'degenerate:negative' not in c.intents:
            assert l - RC.MIN_LEVEL == c.geom.level, c.name


def test_other_pooled_sizes_keep_the_edges():
    for pooled in (3, 14):
        names = {c.name for c in RC.cases('main', pooled)}
        for want in ('first sample at -1', 'sample at W and H', 'outside right', 'empty box', 'negative width', 'image -1', 'image 2',
                     'narrow 0.75x0.75 #0', 'bins 2x4 integer'):
            assert want in names, (pooled, want)
        assert all(RC.is_dyadic(c.roi, pooled) for c in RC.cases('main', pooled))


def test_route_restatement():
    assert RC.route(63, 8, 7) == 'workgroup' and RC.route(64, 8, 7) == 'workgroup+ordered'
    assert RC.route(8192, 256, 7) == 'workgroup+ordered' and RC.route(8193, 256, 7) == 'workgroup'
    assert RC.route(100, 8, 7, out_aligned=False) == 'separable+flagged'
    assert all(RC.route(100, c, 7) == 'separable+flagged' for c in (1, 3, 6, 70, 258))
    assert all(RC.route(100, c, 7) == 'workgroup+ordered' for c in (4, 252, 256, 260, 516))
    assert RC.route(100, 8, 3) == RC.route(100, 6, 14) == 'per-sample'
    # path and separable path agree: flagged exactly where the workgroup kernel samples directly because of the footprint
    for c in _all_cases():
        g = c.geom
        if g.image_ok:
            assert (g.sep_path == 'flagged') == g.over and (g.path == 'direct') == g.over
            assert g.over == (g.nrows > 64 or g.ncols > 64 or g.nrows < 1 or g.ncols < 1)


def test_channel_source():
    src = [RC.channel_source(c) for c in range(520)]
    assert src[:8] == [(c, 1.0) for c in range(8)]
    for c in range(520):
        for d in (1, 4, 8, 64, 256):
            if c + d < 520:
                assert src[c] != src[c + d], (c, d)
    f = RC.wide_features('tiny', 70)
    assert [tuple(t.shape) for t in f] == [(2, h, w, 70) for h, w in RC.SCENES['tiny']]
    assert torch.equal(f[0][..., :8].permute(0, 3, 1, 2), RC.base_features('tiny')[0])
    assert all(float(t.abs().max()) <= 8 and torch.equal(t, t.round()) for t in f)
    e = torch.arange(2 * 8 * 9, dtype=torch.float64).view(2, 8, 3, 3)
    w = RC.widen(e, 20)
    assert w.shape == (2, 3, 3, 20) and torch.equal(w[..., 9].double(), -e[:, 2]) and torch.equal(w[..., 3].double(), e[:, 3])


def test_spread_rois_fill_every_bucket():
    maps = RC.SCENES['main']
    rois = RC.spread_rois(maps)
    assert len(rois) == RC.ORDER_BUCKETS
    assert {RC.bucket_key(r, maps) for r in rois} == set(range(RC.ORDER_BUCKETS))
    assert len({RC.bucket_key(c.roi, maps) for c in RC.cases('main')}) > 20
    idx = RC.repeated(97, 1025, 1)
    assert sorted(set(idx.tolist())) == list(range(97)) and idx.shape == (1025,)
