"""Every case of tests/stitch_cases.py is in the class its name says - shown with the reference (tests/stitch_ref.py) alone - and
the properties that make the bit-for-bit comparison on the GPU a real check hold: the domino case needs as many rounds of
mutually best pairs as it has links, more than a wavefront has lanes; in the tie case the answer depends on the order of tied
pairs; in the contraction case a fused multiply-add would change accepted affinities; and on random problems full of ties the
rounds of mutually best pairs give the greedy answer."""
import random

import pytest

import stitch_cases
import stitch_ref


def run(case):
    offsets, result, jobs, claim = case
    return [stitch_ref.stitch(offsets, result, j) for j in jobs]


@pytest.mark.parametrize('name', sorted(stitch_cases.CASES))
def test_case_is_what_it_claims(name):
    case = stitch_cases.CASES[name]()
    case[3](run(case))


@pytest.mark.parametrize('n', [1024, 1025])
def test_many_trajectories_case(n):
    case = stitch_cases.many_trajectories(n)
    case[3](run(case))
    assert len(set(case[1]['object_id'])) == n


def test_a_fused_multiply_add_would_change_accepted_affinities():
    case = stitch_cases.contraction()
    linear = run(case)[0]
    count = case[3].differing(linear)
    assert count == stitch_cases.CONTRACTION_DIFFERING and 0 < count <= 40
    print('%d of %d accepted affinities differ under a fused px, py' % (count, linear['n_links'][0]))


def test_mutual_best_rounds_equal_the_greedy_walk_on_random_ties():
    """small integer boxes: few distinct affinities, many tied pairs"""
    rng = random.Random(3)
    tied = 0
    for _ in range(60):
        n = rng.randrange(4, 24)
        rows = [(rng.randrange(0, 6), 1 + rng.randrange(2), [float(rng.randrange(0, 4) * 5), 0.0, 10.0, 10.0], 0.9, i) for i in range(n)]
        rows.sort(key=lambda r: r[0])
        res = stitch_cases.result(rows)
        cands = stitch_cases.stream_candidates([0, 6], res, stitch_cases.job(max_link=rng.randrange(1, 5), link_iou=0.1))
        values = [c[0] for c in cands]
        tied += sum(1 for v in values if values.count(v) > 1)
        links, rounds = stitch_ref.match_mutual_best(cands)
        assert links == stitch_ref.match_greedy(cands) and rounds <= max(1, len(links))
    assert tied > 1000
