"""Every case of tests/split_cases.py is in the class its name says - shown with the reference alone (no GPU)."""
import pytest

import split_cases
import split_ref


@pytest.mark.parametrize('name', sorted(split_cases.CASES))
def test_case_is_in_its_class(name):
    offsets, result, jobs, claim = split_cases.CASES[name]()
    claim([split_ref.split(offsets, result, j) for j in jobs])


def test_contraction_tells_a_fused_extrapolation_from_the_definition():
    offsets, result, jobs, claim = split_cases.contraction()
    changed, of = claim.differing(split_ref.split(offsets, result, jobs[0]))
    print('fused: %d of %d values of out_test differ' % (changed, of))
    assert changed > 0 and of == 96


@pytest.mark.parametrize('n', [63, 64, 65, 257])
def test_many_trajectories_in_a_slot(n):
    for empty_stream in (False, True):
        offsets, result, jobs, claim = split_cases.many_in_a_slot(n, empty_stream=empty_stream)
        claim([split_ref.split(offsets, result, j) for j in jobs])
