"""Every case of tests/xlink_cases.py is in the class its name says - shown with the reference (tests/xlink_ref.py) alone - and
the properties that make the bit-for-bit comparison on the GPU a real check hold: on every case the rounds of mutually best pairs
give the greedy answer; the domino case needs as many rounds as it has links, more than a wavefront has lanes; the winners of the
chunk cases lie in another chunk of 64 than their tails; and the tracked fixtures with injected flicker form chains of three
pieces and relabel rows under the loosest job and link nothing under the strictest."""
import os
import random

import pytest

import stitch_ref
import xlink_cases
import xlink_ref
from track_stage_support import G4, G5


def run(case, n_classes=4):
    offsets, result, jobs, claim = case
    return [xlink_ref.xlink(offsets, result, j, n_classes) for j in jobs]


@pytest.mark.parametrize('name', sorted(xlink_cases.CASES))
def test_case_is_what_it_claims(name):
    case = xlink_cases.CASES[name]()
    case[3](run(case))
    xlink_cases.greedy_equals_mutual_best(*case[:3])


def test_sixteen_classes_case():
    case = xlink_cases.sixteen_classes()
    case[3](run(case, 16))


@pytest.mark.parametrize('n', [1024, 1025])
def test_many_trajectories_case(n):
    case = xlink_cases.many_trajectories(n)
    case[3](run(case))
    assert len(set(case[1]['object_id'])) == n and all(case[1]['object_id'].count(i) == 1 for i in (0, n - 1))     # one-row trajectories


def test_one_category_per_object_id_in_every_case():
    for name in sorted(xlink_cases.CASES):
        case = xlink_cases.CASES[name]()
        for got in run(case):
            pairs = set(zip(got['object_id'], got['category']))
            assert len(pairs) == len(set(got['object_id'])), name
            assert len(got['object_id']) == len(got['category']) == len(case[1]['frame']), name


def test_mutual_best_rounds_equal_the_greedy_walk_on_random_ties_across_classes():
    """small integer boxes in three classes: few distinct affinities, many tied pairs, per-pair gaps"""
    rng = random.Random(5)
    tied = 0
    for _ in range(60):
        n = rng.randrange(4, 24)
        rows = [(rng.randrange(0, 6), rng.choice((1, 2, 4)), [float(rng.randrange(0, 4) * 5), 0.0, 10.0, 10.0], 0.9, i) for i in range(n)]
        rows.sort(key=lambda r: r[0])
        res = xlink_cases.result(rows)
        pairs = dict(((a, b), xlink_cases.pair(rng.randrange(0, 5), 0.1)) for a, b in ((1, 2), (2, 4), (1, 4), (2, 2), (4, 4)) if rng.random() < 0.8)
        cands = xlink_cases.stream_candidates([0, 6], res, xlink_cases.job(pairs))
        values = [c[0] for c in cands]
        tied += sum(1 for v in values if values.count(v) > 1)
        links, rounds = stitch_ref.match_mutual_best(cands)
        assert links == stitch_ref.match_greedy(cands) and rounds <= max(1, len(links))
    assert tied > 500


def test_diagonal_pairs_reduce_to_stitching_on_the_stitch_cases():
    """a job with only diagonal pairs carrying stitching's per-class parameters is stitching, by the two references"""
    import stitch_cases
    for name in sorted(stitch_cases.CASES):
        offsets, res, jobs, _ = stitch_cases.CASES[name]()
        for j in jobs:
            want = stitch_ref.stitch(offsets, res, j)
            got = xlink_ref.xlink(offsets, res, xlink_cases.job(diagonal(j), motion=j['motion']))
            for k in ('object_id', 'pred', 'root', 'affinity', 'row_root', 'links', 'n_links', 'traj_offsets'):
                assert got[k] == want[k], (name, k)
            assert got['category'] == res['category'] and not any(got['n_relabelled'])


def diagonal(stitch_job):
    return dict(((c + 1, c + 1), xlink_cases.pair(g, t)) for c, (g, t) in enumerate(zip(stitch_job['max_link'], stitch_job['link_iou'])))


@pytest.mark.parametrize('fixture,cfg', [('sort_g4_input.json', G4), ('sort_g5_input.json', G5)])
def test_injected_flicker_makes_the_tracked_fixtures_a_test(oracle, golden_dir, fixture, cfg):
    """The condition of the GPU test on the tracked fixtures, with the CPU oracle's SORT in the tracker's place (max_age 1)."""
    from waymo_2d_tracking_amd.tracking import utils as T
    packed = T.pack_streams(T.read_data_file(os.path.join(golden_dir, fixture), cfg['score']))
    out = oracle.track_streams(packed, 1, 0, cfg['score'], cfg['iou'])
    flick = xlink_cases.inject_flicker(out)
    pieces = min(3, xlink_cases.most_slots(packed, out))
    assert pieces == (3 if 'g4' in fixture else 2)
    if pieces == 3:
        assert len(set(flick['object_id'].tolist())) > len(set(out['object_id'].tolist())) and (flick['category'] != out['category']).any()
    refs = [xlink_ref.xlink(packed['stream_frame_offsets'], flick, j) for j in xlink_cases.FLICKER_JOBS]
    xlink_cases.flicker_condition(refs, pieces)
    print('%s: links per job %s, relabelled %s' % (fixture, [sum(r['n_links']) for r in refs], [sum(r['n_relabelled']) for r in refs]))
