"""The assignment cases of tests/sort_cases.py, proved on the CPU oracle alone: they are hard (step 6 runs, augmenting paths are long,
the threshold rejects matches), the oracle's answer on them is optimal, and every crowd configuration lands in the dispatch class of
the kernel it is meant for.  No GPU: tests/test_gpu_sort_assignment.py runs the same cases on the kernels."""
import functools
import itertools

import numpy as np
import pytest

import sort_cases as sc


@functools.lru_cache(maxsize=None)
def _solve(family, n, m):
    from oracle import oracle as O
    O.build()
    c = sc.cost(family, n, m)
    pairs, stats = O.linear_assignment_stats(c)
    return c, pairs, stats


@functools.lru_cache(maxsize=None)
def _trace(name, n_streams):
    from oracle import oracle as O
    O.build()
    return sc.crowd_trace(O, sc.CROWDS[name], n_streams)


def _total(c, pairs):
    return float(c[pairs[:, 0], pairs[:, 1]].astype(np.float64).sum())


def test_stats_entry_point_changes_no_result(oracle):
    for family, (n, m) in itertools.product(sc.FAMILIES, ((1, 1), (65, 64), (62, 130), (7, 7), (6, 9))):
        c, pairs, stats = _solve(family, n, m)
        assert np.array_equal(pairs, oracle.linear_assignment(c)), (family, n, m)
        assert len(pairs) == min(n, m)
        assert stats['longest_path'] <= stats['paths'] * min(n, m)
    # known counts: a 2 x 2 matrix whose rows both prefer column 0 needs one step 6 and one augmenting path; the cheaper way out
    # (row 1 moves: 0.5 lost) keeps row 0's star, so no star lies on the path
    pairs, stats = oracle.linear_assignment_stats(np.array([[-1.0, -0.25], [-1.0, -0.5]], np.float32))
    assert pairs.tolist() == [[0, 0], [1, 1]] and stats == dict(step6=1, paths=1, longest_path=0)
    # ... and here the star has to move: row 0 is starred greedily in column 0, row 1 can only live there
    pairs, stats = oracle.linear_assignment_stats(np.array([[-1.0, -0.75], [-1.0, 0.0]], np.float32))
    assert pairs.tolist() == [[0, 1], [1, 0]] and stats == dict(step6=1, paths=1, longest_path=1)
    pairs, stats = oracle.linear_assignment_stats(np.zeros((5, 9), np.float32))
    assert stats == dict(step6=0, paths=0, longest_path=0)


def test_families_are_what_they_claim():
    for n, m in sc.SHAPES + sc.SMALL_SHAPES:
        for family in sc.FAMILIES:
            c = sc.cost(family, n, m)
            assert c.dtype == np.float32 and c.shape == (n, m) and c.flags.c_contiguous
            assert np.all(np.isfinite(c)) and c.min() >= -1 and c.max() <= 0
            assert np.array_equal(c, sc.cost(family, n, m))                                  # deterministic
        d = sc.cost('dense', n, m)
        assert np.all(d != 0) and len(np.unique(d)) == d.size                               # no zero, no tie
        assert len(np.unique(sc.cost('ties', n, m))) <= 3
        assert np.all(np.diff(sc.cost('const_rows', n, m), axis=1) == 0)
        assert np.all(np.diff(sc.cost('const_cols', n, m), axis=0) == 0)
        e = sc.cost('all_equal_nonzero', n, m)
        assert np.all(e == e[0, 0]) and e[0, 0] != 0
        dc = sc.cost('dup_cols', n, m)
        assert np.array_equal(dc[:, 0:m - m % 2:2], dc[:, 1:m:2])
        z = sc.cost('neg_zero', n, m)
        assert np.all(z == 0) and (n * m < 8 or (np.signbit(z).any() and not np.signbit(z).all()))
        b = sc.cost('block', n, m)
        assert n * m < 64 or ((b == 0).any() and (b != 0).any())
        r = sc.cost('rank1_eps', n, m).astype(np.float64)
        if n > 1 and m > 1:                 # additive up to the perturbation: second differences of a few float32 ulps of values <= 1
            assert np.abs(r[1:, 1:] - r[1:, :-1] - r[:-1, 1:] + r[:-1, :-1]).max() <= 16 * 2.0 ** -24


@pytest.mark.parametrize('family', sc.FAMILIES)
def test_every_family_needs_step6_and_long_paths(family):
    for n, m in sc.SHAPES:
        _, pairs, stats = _solve(family, n, m)
        assert len(pairs) == min(n, m)
        if min(n, m) >= 8 and family not in sc.NO_STEP6_REQUIRED:
            assert stats['step6'] >= 1, (family, n, m, stats)
        if min(n, m) >= 64 and family in sc.LONG_PATH_FAMILIES:
            assert stats['longest_path'] >= 3, (family, n, m, stats)
    for family_ in ('const_rows', 'all_equal_nonzero', 'neg_zero'):       # zero everywhere after step 1 (const_rows: when not transposed)
        for n, m in sc.SHAPES:
            if n <= m:
                assert _solve(family_, n, m)[2]['step6'] == 0


def _brute_force_min(c):
    """Minimum total over all injections of the shorter side into the longer one, in float64 (sums of <= 7 float32 values: exact)."""
    c = c.astype(np.float64)
    if c.shape[0] > c.shape[1]:
        c = c.T
    n, m = c.shape
    rows = np.arange(n)
    best, count = np.inf, 0
    for cols in itertools.permutations(range(m), n):
        t = c[rows, list(cols)].sum()
        if t < best:
            best, count = t, 1
        elif t == best:
            count += 1
    return best, count


@pytest.mark.parametrize('family', sc.FAMILIES)
def test_oracle_is_optimal_on_small_instances(family):
    for n, m in sc.SMALL_SHAPES:
        c, pairs, _ = _solve(family, n, m)
        assert len(set(pairs[:, 0].tolist())) == len(set(pairs[:, 1].tolist())) == min(n, m)
        best, count = _brute_force_min(c)
        # sums of at most 7 values of at most 24 bits in [-1, 0]: exact in float64 in any order
        assert _total(c, pairs) == best, (family, n, m)
        if family == 'ties':
            assert count == 1                                            # the optimum is unique ...
            r, cc, total = sc.ties_optimum(n, m)
            o = np.argsort(r)
            assert total == best and np.array_equal(pairs[:, 0], r[o]) and np.array_equal(pairs[:, 1], cc[o])   # ... and is the hidden one


def test_ties_optimum_is_found_at_every_shape():
    for n, m in sc.SHAPES:
        c, pairs, _ = _solve('ties', n, m)
        r, cc, total = sc.ties_optimum(n, m)
        o = np.argsort(r)
        assert np.array_equal(pairs[:, 0], r[o]) and np.array_equal(pairs[:, 1], cc[o]) and _total(c, pairs) == total


@pytest.mark.parametrize('family', sc.FAMILIES)
def test_oracle_total_equals_scipy_at_64(family):
    optimize = pytest.importorskip('scipy.optimize')      # only this assertion depends on scipy
    c, pairs, _ = _solve(family, 64, 64)
    r, cc = optimize.linear_sum_assignment(c.astype(np.float64))
    want = float(c.astype(np.float64)[r, cc].sum())
    # both totals are sums of 64 float32 values in [-1, 0] accumulated in float64: exact, so optimal totals are equal bit for bit
    assert _total(c, pairs) == want, family


def test_engine_plan_matches_the_constants_of_the_engine():
    """The numbers of sort_cases.engine_plan against the sources they mirror: a change of the budgets, of the HelpJob layout or of the
    few-tracker limit has to be followed here."""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'waymo_2d_tracking_amd', 'csrc')
    eng = open(os.path.join(root, 'sort_engine.hip')).read()
    assert int(re.search(r'constexpr int kLdsCostFloats = (\d+);', eng).group(1)) == sc.LDS_COST_FLOATS
    assert int(re.search(r'constexpr int kLdsCostFloatsFew = (\d+);', eng).group(1)) == sc.LDS_COST_FLOATS_FEW
    assert 'n_streams * (int64_t)p->n_classes <= 256' in eng and 'n_trackers <= 256' in eng
    assert '((int64_t)160 * 1024 - 512 - (int64_t)mk - (int64_t)wtdev::help_lds_bytes() - 16) / 4' in eng
    single = open(os.path.join(root, 'sort_single.hip')).read()
    assert int(re.search(r'constexpr int kLdsCostFloats = (\d+);', single).group(1)) == sc.LDS_COST_FLOATS
    # few trackers, frames of 100 boxes, max_age 2: 160 KiB - 512 - 8016 (bitmaps of 100 x 400) - 10464 (HelpJob) - 16 = 144832 bytes
    assert sc.munkres_lds_bytes(100, 400) == 8016
    assert sc.engine_plan(100, 5) == (36208, True)
    assert sc.engine_plan(100, 65) == (8192, False)
    assert sc.engine_plan(8, 1) == (8 * 33, True)                         # the whole 8 x (32 | 1) matrix fits
    assert sc.engine_plan(20, 64) == (20 * 81, True) and sc.engine_plan(20, 65)[1] is False


CLASS_OF = {'a': dict(variant='<2,2>', cost='lds'), 'b': dict(variant='<2,6>', cost='lds'), 'c': dict(variant='<2,6>', cost='global'),
            'd': dict(variant='generic')}


@pytest.mark.parametrize('name', sorted(sc.CROWDS))
def test_crowd_streams_are_hard_and_land_in_their_class(name):
    cfg = sc.CROWDS[name]
    frames = sc.crowd_frames(cfg)
    assert 6 <= len(frames) <= 10 and [len(f) for f in frames] == list(cfg.counts)
    assert all(np.array_equal(a, b) for a, b in zip(frames, sc.crowd_frames(cfg)))
    integer = all(np.all(f[:, :4] == np.round(f[:, :4])) for f in frames)
    assert integer == cfg.integer
    alone = _trace(name, 1)
    assert alone[0]['helpers'] and alone[0]['dispatch'] is None and alone[0]['T'] == 0
    later = alone[1:]
    # dense cost matrices: boxes packed closer than their size
    assert np.mean([(r['cost'] != 0).mean() for r in later]) > 0.85
    hard = [r for r in later if r['stats']['step6'] >= 1 and len(r['rejected']) >= 1]
    assert 2 * len(hard) >= len(later), [(r['N'], r['T'], r['stats'], len(r['rejected'])) for r in later]
    for r in later:                                    # the raw assignment is complete; what associate drops is below the threshold
        assert len(r['raw']) == min(r['N'], r['T'])
        assert len(r['matches']) + len(r['rejected']) == len(r['raw'])
        for d, t in r['rejected']:
            assert float(-r['cost'][d, t]) < cfg.iou_thr
    # T grows to 2 - 3 N (lingering rejected tracks), and both orientations occur
    assert max(r['T'] / r['N'] for r in later) >= 2.0
    mine = [r for r in later if r['dispatch']['cls'] == name]
    assert len(mine) >= 2, [(r['N'], r['T'], r['dispatch']['cls']) for r in later]
    for r in mine:
        for k, v in CLASS_OF[name].items():
            assert r['dispatch'][k] == v
    if name in 'ab':
        assert any(r['dispatch']['transposed'] for r in mine) and any(not r['dispatch']['transposed'] for r in mine)
    assert any(r['dispatch']['transposed'] for r in later) and any(not r['dispatch']['transposed'] for r in later)
    # next to the trivial streams: more than 256 trackers, no helper waves, the 8192-float budget
    crowded = _trace(name, 1 + sc.N_TRIVIAL)
    assert (1 + sc.N_TRIVIAL) * sc.N_CLASSES > sc.FEW_TRACKERS and not crowded[0]['helpers'] and crowded[0]['lds_cost'] <= 8192
    assert [(r['N'], r['T']) for r in crowded] == [(r['N'], r['T']) for r in alone]
    variants = {(r['dispatch']['variant'], r['dispatch']['cost']) for r in crowded[1:]}
    assert (CLASS_OF[name]['variant'], 'lds' if name == 'a' else 'global') in variants      # (a)'s matrices fit 8192 floats


def test_crowd_sizes_stay_small():
    """The largest assignment of the crowd streams stays near the 128 x 384 of the largest register variant."""
    for name in sc.CROWDS:
        for r in _trace(name, 1):
            assert r['N'] <= 150 and r['T'] <= 384


def test_packed_layout_and_oracle_track_counts(oracle):
    """packed() is what tracking.utils.pack_streams would build, and oracle.track_streams on it steps the crowd class through the same
    (N, T) pairs the dispatch arithmetic was computed from (its row count per frame = matched detections + births = N)."""
    cfg = sc.CROWDS['a']
    for n_trivial in (0, sc.N_TRIVIAL):
        p = sc.packed(cfg, n_trivial)
        n_streams = len(p['stream_frame_offsets']) - 1
        assert n_streams == 1 + n_trivial and p['frame_det_offsets'][-1] == len(p['x']) == len(p['category'])
        assert p['stream_frame_offsets'][-1] == len(p['frame_det_offsets']) - 1
        assert np.all(p['category'][:sum(cfg.counts)] == sc.CROWD_CLASS) and p['category'].min() >= 1 and p['category'].max() <= sc.N_CLASSES
        ref = oracle.track_streams(p, sc.MAX_AGE, sc.MIN_HITS, [0.0] * sc.N_CLASSES, sc.iou_thresholds(cfg))
        per_frame = np.bincount(ref['frame'], minlength=len(p['frame_det_offsets']) - 1)
        assert per_frame[:len(cfg.counts)].tolist() == list(cfg.counts)              # min_hits 0: every detection's track is emitted
        assert per_frame[len(cfg.counts):].tolist() == [1] * (3 * n_trivial)
        trace = _trace('a', n_streams)
        births = sum(len(r.get('unmatched_dets', range(r['N']))) for r in trace)
        assert ref['n_births'] == births + n_trivial
