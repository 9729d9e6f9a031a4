"""Every case of tests/refine_cases.py is in the class its name says - shown with the reference (tests/refine_ref.py) alone - and
the two families that make the bit-for-bit comparison on the GPU a real check do what they are for: among the interpolation
cases some value differs between the definition's unfused formula and a fused multiply-add, and among the mean cases some
trajectory's score sum depends on the order of the additions."""
from fractions import Fraction

import pytest

import refine_cases
import refine_ref


def run(case):
    offsets, result, jobs, claim = case
    return [refine_ref.refine(offsets, result, j) for j in jobs]


@pytest.mark.parametrize('name', sorted(refine_cases.CASES))
def test_case_is_what_it_claims(name):
    case = refine_cases.CASES[name]()
    case[3](run(case))


@pytest.mark.parametrize('n', [1024, 1025])
def test_many_trajectories_case(n):
    case = refine_cases.many_trajectories(n)
    case[3](run(case))
    assert len(set(case[1]['object_id'])) == n


def fused(va, vb, j, n):
    """(vb - va) * t + va with the product and the sum rounded ONCE (what a contracted multiply-add computes)"""
    t = float(j) / float(n)
    d = vb - va
    return float(Fraction(d) * Fraction(t) + Fraction(va))


def test_a_fused_multiply_add_would_change_some_interpolated_value():
    offsets, result, jobs, _ = refine_cases.fractional_thirds()
    r = refine_ref.refine(offsets, result, jobs[0])
    by_id = {}
    for i, oid in enumerate(result['object_id']):
        by_id.setdefault(oid, []).append(i)
    differ = total = 0
    for i, src in enumerate(r['source']):
        if src >= 0:
            continue
        b = -1 - src
        a = [k for k in by_id[result['object_id'][b]] if k != b][0]
        j, n = r['frame'][i] - result['frame'][a], result['frame'][b] - result['frame'][a]
        assert n == 3 and j in (1, 2)
        values = [(result['bbox'][a][c], result['bbox'][b][c], r['bbox'][i][c]) for c in range(4)] + [(result['score'][a], result['score'][b], r['score'][i])]
        for va, vb, got in values:
            assert got == refine_ref.interpolate(va, vb, j, n)
            total += 1
            differ += got != fused(va, vb, j, n)
    assert total == 400 and differ >= 1, (differ, total)


def test_some_mean_depends_on_the_addition_order():
    offsets, result, jobs, _ = refine_cases.mean_scores()
    scores = {}
    for f, oid, s in sorted(zip(result['frame'], result['object_id'], result['score'])):
        scores.setdefault(oid, []).append(s)
    r = refine_ref.refine(offsets, result, jobs[0])
    differ = 0
    for oid, ss in scores.items():
        total = ss[0]
        for s in ss[1:]:
            total = total + s
        backward = ss[-1]
        for s in reversed(ss[:-1]):
            backward = backward + s
        differ += total != backward
        assert r['score'][r['object_id'].index(oid)] == total / float(len(ss)) == refine_ref.mean_in_order(ss)
    assert differ >= 1
