"""Every case of tests/dedup_cases.py is in the class its name says - shown with the reference (tests/dedup_ref.py) alone - and
the invariants of the reference that make the bit-for-bit comparison on the GPU a real check hold: the default job reproduces
the input, every trajectory is kept or suppressed, every suppressor is itself kept, stronger and a duplicate, and on random
problems full of overlapping tracks the decision in rounds (the kernel's way) gives the greedy walk's answer."""
import random

import pytest

import dedup_cases
import dedup_ref


def run(case):
    offsets, result, jobs, claim = case
    return [dedup_ref.dedup(offsets, result, j) for j in jobs]


@pytest.mark.parametrize('name', sorted(dedup_cases.CASES))
def test_case_is_what_it_claims(name):
    case = dedup_cases.CASES[name]()
    case[3](run(case))


@pytest.mark.parametrize('n', [1024, 1025])
def test_many_trajectories_case(n):
    case = dedup_cases.many_trajectories(n)
    case[3](run(case))
    assert len(set(case[1]['object_id'])) == n


@pytest.mark.parametrize('name', sorted(dedup_cases.CASES))
def test_default_job_reproduces_the_input(name):
    offsets, result, jobs, _ = dedup_cases.CASES[name]()
    ref = dedup_ref.dedup(offsets, result, dedup_cases.job())
    assert ref['row_keep'] == [1] * len(result['frame']) and ref['dropped'] == [] and sum(ref['n_dropped']) == 0
    assert ref['keep'] == [1] * len(ref['keep']) and ref['by'] == [-1] * len(ref['keep']) and ref['match'] == [0] * len(ref['keep'])
    same = lambda a, b: repr(a) == repr(b)                                              # NaN coordinates compare by their text
    assert ref['frame'] == list(result['frame']) and ref['object_id'] == list(result['object_id']) and same(ref['bbox'], [[float(v) for v in b] for b in result['bbox']])


def check_invariants(offsets, result, job, ref):
    per_stream = dedup_ref.trajectories(offsets, result)
    for s in range(len(offsets) - 1):
        trajs = per_stream.get(s, [])
        t0, t1 = ref['traj_offsets'][s], ref['traj_offsets'][s + 1]
        assert t1 - t0 == len(trajs)
        keep, by, match = ref['keep'][t0:t1], ref['by'][t0:t1], ref['match'][t0:t1]
        dups = dedup_ref.duplicates(trajs, job)
        m_of = lambda t, u: dups.get((t, u) if t < u else (u, t))
        assert set(keep) <= {0, 1} and ref['n_dropped'][s] == keep.count(0)                # suppressed and kept together are all
        for t in range(len(trajs)):
            kept_stronger = [u for u in range(len(trajs)) if keep[u] and m_of(t, u) is not None and dedup_ref.stronger(trajs, u, t)]
            if keep[t]:
                assert by[t] == -1 and match[t] == 0 and not kept_stronger
            else:
                assert keep[by[t]] == 1 and dedup_ref.stronger(trajs, by[t], t) and match[t] == m_of(t, by[t]) > 0
                assert all(u == by[t] or dedup_ref.stronger(trajs, by[t], u) for u in kept_stronger)
            for slot, (_, row) in trajs[t].obs.items():
                assert ref['row_keep'][row] == keep[t]


@pytest.mark.parametrize('name', sorted(dedup_cases.CASES))
def test_reference_invariants_on_the_cases(name):
    offsets, result, jobs, _ = dedup_cases.CASES[name]()
    for job, ref in zip(jobs, run((offsets, result, jobs, None))):
        check_invariants(offsets, result, job, ref)


def random_problem(rng):
    """tracks on a coarse grid of positions: many overlapping pairs, chains of duplicates, equal lengths and score sums"""
    rows = []
    for i in range(rng.randrange(3, 30)):
        first = rng.randrange(0, 8)
        slots = [f for f in range(first, min(12, first + rng.randrange(1, 10))) if rng.random() < 0.85] or [first]
        rows += dedup_cases.track(i, slots, 3.0 * rng.randrange(0, 8), category=1 + rng.randrange(2), score=rng.choice([0.25, 0.5, 0.75]))
    return dedup_cases.result(dedup_cases.by_slot(rows))


def test_rounds_equal_the_greedy_walk_on_random_problems():
    rng = random.Random(5)
    suppressed = deep = 0
    for _ in range(80):
        res = random_problem(rng)
        job = dedup_cases.job(min_frames=rng.randrange(1, 4), dup_iou=rng.choice([0.4, 0.5, 0.7]), dup_frac=rng.choice([0.0, 0.5, 1.0]))
        trajs = dedup_ref.trajectories([0, 12], res).get(0, [])
        dups = dedup_ref.duplicates(trajs, job)
        keep, by, match, rounds = dedup_ref.suppress_in_rounds(trajs, dups)
        assert (keep, by, match) == dedup_ref.suppress_greedy(trajs, dups) and rounds <= max(1, len(trajs))
        check_invariants([0, 12], res, job, dedup_ref.dedup([0, 12], res, job))
        suppressed += keep.count(0)
        deep += rounds > 2
    assert suppressed > 100 and deep > 10
