"""Every case of tests/smooth_cases.py is in the class its name says - shown with the plain-Python reference alone (no GPU), so
that a kernel that equals the reference on them has met the hazards they stand for."""
import ctypes as C

import pytest

import smooth_cases
import smooth_ref


@pytest.mark.parametrize('name', sorted(smooth_cases.CASES))
def test_case_is_in_its_class(name):
    offsets, result, jobs, claim = smooth_cases.CASES[name]()
    claim([smooth_ref.smooth(offsets, result, j) for j in jobs])


def test_contraction_tells_every_variant_from_the_definition():
    offsets, result, jobs, claim = smooth_cases.contraction()
    smoothed = smooth_ref.smooth(offsets, result, jobs[0])
    for variant in ('fused', 'descending', 'split'):
        changed, of = claim.differing(smoothed, variant)
        print('%s: %d of %d values differ' % (variant, changed, of))
        assert changed > 0 and of == 292
    assert claim.differing(smoothed, 'definition')[0] == 0


def test_a_row_without_a_pair_keeps_its_input_bits_and_the_quotient_would_not():
    """(k0 * v) / k0 is not v: the rule "no pair: the input itself" is not a shortcut"""
    import random
    rng = random.Random(3)
    k0 = smooth_ref.gaussian(1.5, 4)[1]
    values = [rng.uniform(0, 2000) for _ in range(1000)]
    assert sum(1 for v in values if (k0 * v) / k0 != v) > 50
    for v in values[:50]:
        assert smooth_ref.smooth_value({3: v, 4: 1.0}, 3, 3, [k0, 1.0, 1.0, 1.0]) == (v, 0)


@pytest.mark.parametrize('above', [0, 1])
def test_many_trajectories_on_either_side_of_the_lds_limit(above):
    from waymo_2d_tracking_amd import build
    build.build(verbose=False)
    from waymo_2d_tracking_amd import _lib
    limit = C.c_int32(0)
    _lib.lib().wt_smooth_tracks_limits(C.byref(limit))
    assert 64 < limit.value <= 4096
    offsets, result, jobs, claim = smooth_cases.many_trajectories(limit.value + above)
    claim([smooth_ref.smooth(offsets, result, j) for j in jobs])
