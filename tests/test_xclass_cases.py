"""Every case of tests/xclass_cases.py is in the class its name says - shown with the reference (tests/xclass_ref.py) alone - and
the invariants of the reference that make the bit-for-bit comparison on the GPU a real check hold: the default job reproduces
the input, every trajectory is kept or suppressed, every suppressor is itself kept, stronger and the strongest such one, on
random problems with mixed classes and priorities the decision in rounds (the kernel's way) gives the greedy walk's answer, and
with diagonal pairs, equal priorities and the IoU the pass is the deduplication of tests/dedup_ref.py."""
import random

import pytest

import dedup_cases
import dedup_ref
import xclass_cases
import xclass_ref

C = xclass_cases.N_CLASSES


def run(case):
    offsets, result, jobs, claim = case
    return [xclass_ref.xclass(offsets, result, j, C) for j in jobs]


@pytest.mark.parametrize('name', sorted(xclass_cases.CASES))
def test_case_is_what_it_claims(name):
    case = xclass_cases.CASES[name]()
    case[3](run(case))


@pytest.mark.parametrize('n', [1024, 1025])
def test_many_trajectories_case(n):
    case = xclass_cases.many_trajectories(n)
    case[3](run(case))
    assert len(set(case[1]['object_id'])) == n


@pytest.mark.parametrize('name', sorted(xclass_cases.CASES))
def test_default_job_reproduces_the_input(name):
    offsets, result, jobs, _ = xclass_cases.CASES[name]()
    for job in ({}, xclass_cases.job({}), xclass_cases.job({(2, 4): (0, 0.0, 0.0), (1, 1): (0, 0.0, 0.0)}, prio=[3, 2, 1, 0], measure='iou')):
        ref = xclass_ref.xclass(offsets, result, job, C)
        assert ref['row_keep'] == [1] * len(result['frame']) and ref['dropped'] == [] and sum(ref['n_dropped']) == 0
        assert ref['keep'] == [1] * len(ref['keep']) and ref['by'] == [-1] * len(ref['keep']) and ref['match'] == [0] * len(ref['keep'])
        same = lambda a, b: repr(a) == repr(b)                                          # NaN coordinates compare by their text
        assert ref['frame'] == list(result['frame']) and ref['object_id'] == list(result['object_id']) and same(ref['bbox'], [[float(v) for v in b] for b in result['bbox']])


def check_invariants(offsets, result, job, ref):
    prio = xclass_ref.tables(job, C)[3]
    per_stream = dedup_ref.trajectories(offsets, result)
    for s in range(len(offsets) - 1):
        trajs = per_stream.get(s, [])
        t0, t1 = ref['traj_offsets'][s], ref['traj_offsets'][s + 1]
        assert t1 - t0 == len(trajs)
        keep, by, match = ref['keep'][t0:t1], ref['by'][t0:t1], ref['match'][t0:t1]
        pairs = xclass_ref.same_objects(trajs, job, C)
        m_of = lambda t, u: pairs.get((t, u) if t < u else (u, t))
        stronger = lambda t, u: xclass_ref.stronger(trajs, prio, t, u)
        assert set(keep) <= {0, 1} and ref['n_dropped'][s] == keep.count(0)                # suppressed and kept together are all
        for t in range(len(trajs)):
            kept_stronger = [u for u in range(len(trajs)) if keep[u] and m_of(t, u) is not None and stronger(u, t)]
            if keep[t]:
                assert by[t] == -1 and match[t] == 0 and not kept_stronger
            else:
                assert keep[by[t]] == 1 and stronger(by[t], t) and match[t] == m_of(t, by[t]) > 0
                assert all(u == by[t] or stronger(by[t], u) for u in kept_stronger)
            for slot, (_, row) in trajs[t].obs.items():
                assert ref['row_keep'][row] == keep[t]


@pytest.mark.parametrize('name', sorted(xclass_cases.CASES))
def test_reference_invariants_on_the_cases(name):
    offsets, result, jobs, _ = xclass_cases.CASES[name]()
    for job, ref in zip(jobs, run((offsets, result, jobs, None))):
        check_invariants(offsets, result, job, ref)


def test_strength_order_is_strict_and_total():
    offsets, result, jobs, _ = xclass_cases.strongest_kept_suppressor()
    trajs = dedup_ref.trajectories(offsets, result)[0]
    for job in jobs:
        prio = xclass_ref.tables(job, C)[3]
        for t in range(len(trajs)):
            assert not xclass_ref.stronger(trajs, prio, t, t)
            for u in range(t + 1, len(trajs)):
                assert xclass_ref.stronger(trajs, prio, t, u) != xclass_ref.stronger(trajs, prio, u, t)


def random_problem(rng):
    """tracks of four classes on a coarse grid of positions: many overlapping pairs, chains, equal lengths and score sums"""
    rows = []
    for i in range(rng.randrange(3, 30)):
        first = rng.randrange(0, 8)
        slots = [f for f in range(first, min(12, first + rng.randrange(1, 10))) if rng.random() < 0.85] or [first]
        rows += dedup_cases.track(i, slots, 3.0 * rng.randrange(0, 8), w=rng.choice([6.0, 10.0]), category=1 + rng.randrange(4), score=rng.choice([0.25, 0.5, 0.75]))
    return dedup_cases.result(dedup_cases.by_slot(rows))


def random_job(rng):
    pairs = {}
    for a in range(1, 5):
        for b in range(a, 5):
            if rng.random() < 0.7:
                pairs[(a, b)] = (rng.randrange(1, 4), rng.choice([0.4, 0.5, 0.7, 0.9]), rng.choice([0.0, 0.5, 1.0]))
    return xclass_cases.job(pairs, prio=[rng.randrange(0, 3) for _ in range(4)], measure=rng.choice(['iou', 'iomin']))


def test_rounds_equal_the_greedy_walk_on_random_problems():
    rng = random.Random(11)
    suppressed = deep = cross = longer = 0
    for _ in range(80):
        res, job = random_problem(rng), random_job(rng)
        prio = xclass_ref.tables(job, C)[3]
        trajs = dedup_ref.trajectories([0, 12], res).get(0, [])
        pairs = xclass_ref.same_objects(trajs, job, C)
        keep, by, match, rounds = xclass_ref.suppress_in_rounds(trajs, pairs, prio)
        assert (keep, by, match) == xclass_ref.suppress_greedy(trajs, pairs, prio) and rounds <= max(1, len(trajs))
        check_invariants([0, 12], res, job, xclass_ref.xclass([0, 12], res, job, C))
        suppressed += keep.count(0)
        deep += rounds > 2
        cross += sum(1 for t in range(len(trajs)) if not keep[t] and trajs[t].category != trajs[by[t]].category)
        longer += sum(1 for t in range(len(trajs)) if not keep[t] and trajs[t].n > trajs[by[t]].n)
    assert suppressed > 100 and deep > 10 and cross > 50 and longer > 5


def test_diagonal_pairs_equal_priorities_and_iou_are_the_deduplication():
    """the reduction: over every case job of tests/dedup_cases.py, keep, by, match and everything else equal tests/dedup_ref.py"""
    n_jobs = 0
    for name in sorted(dedup_cases.CASES):
        offsets, result, jobs, _ = dedup_cases.CASES[name]()
        for job in jobs:
            want = dedup_ref.dedup(offsets, result, job)
            got = xclass_ref.xclass(offsets, result, xclass_ref.from_dedup_job(job, C), C)
            assert repr(got) == repr(want), name                                         # NaN coordinates compare by their text
            n_jobs += 1
    assert len(dedup_cases.CASES) == 18 and n_jobs == 27
