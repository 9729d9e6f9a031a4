"""TEST INFRASTRUCTURE ONLY - small adversarial layouts for the trajectory coverage table.

Every case is a ground truth, K results and a check of the property it is built to hit, stated on the output of
tests/coverage_ref.py alone (tests/test_coverage_cases.py runs those checks on the CPU; tests/test_gpu_mot_coverage.py compares
the kernels with the same reference outputs, row for row).  Boxes of different objects never overlap and a result row is a copy
of the annotation it is meant to match, so which rows are matched is decided here, not by the assignment.
"""
import coverage_ref

_REFS = {}


def ann(frame, oid, cat=1, level=1, slot=None, cam='FRONT', seg='seg'):
    slot = int(str(oid).lstrip('abcdefghijklmnopqrstuvwxyz') or 0) if slot is None else slot
    return {'image_id': '%s/%d/%s' % (seg, frame, cam), 'bbox': [60 * (slot % 20), 60 * (slot // 20) + 1000 * (cat - 1), 40, 40],
            'category_id': cat, 'object_id': str(oid), 'tracking_difficulty_level': level}


def copies(anns, keep, hyp_id=lambda a: 'h' + a['object_id']):
    """Result rows: a copy of every annotation with keep(annotation), under the id hyp_id(annotation)."""
    return [{'image_id': a['image_id'], 'bbox': list(a['bbox']), 'score': 0.9, 'category_id': a['category_id'], 'object_id': hyp_id(a)}
            for a in anns if keep(a)]


def frame_of(a):
    return int(a['image_id'].split('/')[1])


def by_pattern(patterns):
    """keep(): object id -> string of 0 / 1 per row of the object, in frame order ('1' = matched)."""
    seen = {}

    def keep(a):
        i = seen[a['object_id']] = seen.get(a['object_id'], -1) + 1
        p = patterns.get(a['object_id'], '1')
        return p[i % len(p)] == '1'
    return keep


def stats_of(ref, oid, cat=1, cam='FRONT'):
    for (key, c, o), per_level in ref['trajectories']:
        if o == str(oid) and c == cat and key[1] == cam:
            return per_level
    raise KeyError(oid)


def _frame_sizes():
    sizes = [0, 1, 63, 64, 65, 129]
    anns = [ann(f, 'z', cat=2, slot=399) for f in range(len(sizes))]            # keeps every frame alive
    for f, n in enumerate(sizes):
        anns += [ann(f, 'o%d' % i, level=2 if i % 7 == 0 else 1) for i in range(n)]
    res = copies(anns, lambda a: a['category_id'] == 1 and (int(a['object_id'][1:]) + frame_of(a)) % 3 != 0)

    def check(refs):
        per_frame = {}
        for a in anns:
            if a['category_id'] == 1:
                per_frame[frame_of(a)] = per_frame.get(frame_of(a), 0) + 1
        assert [per_frame.get(f, 0) for f in range(len(sizes))] == sizes
        row = refs[0]['table'][1][2]
        assert row['traj'] == 129 and row['frag'] > 0 and row['mt'] > 0 and row['pt'] > 0
        assert stats_of(refs[0], 'o0')[2]['len'] == 5 and stats_of(refs[0], 'o128')[2]['len'] == 1
        assert refs[0]['table'][1][1]['traj'] < 129
    return anns, [res], check


def _trajectory_counts():
    counts = {'A': 0, 'B': 1, 'C': 64, 'D': 65}
    anns = []
    for cam, n in counts.items():
        for f in range(3):
            anns.append(ann(f, 'z', cat=2, slot=399, cam=cam))
            anns += [ann(f, 'o%d' % i, cam=cam) for i in range(n)]
    res = copies(anns, lambda a: a['category_id'] == 1 and not (frame_of(a) == 1 and int(a['object_id'][1:]) % 2))

    def check(refs):
        got = [refs[0]['per_stream'][('seg', cam)][1][2]['traj'] for cam in 'ABCD']
        assert got == [0, 1, 64, 65]
        assert refs[0]['per_stream'][('seg', 'D')][1][2]['frag'] == 32 and refs[0]['per_stream'][('seg', 'C')][1][2]['frag'] == 32
        assert refs[0]['table'][2][2] == dict(traj=4, mt=0, pt=0, ml=4, frag=0, MT=0.0, ML=1.0, FM=0)
    return anns, [res], check


def _one_frame_stream():
    anns = [ann(7, 'o%d' % i, cat=1 + i % 2, level=1 + (i % 3 == 0), cam='ONE') for i in range(5)]
    anns += [ann(f, 'o0', cam='TWO') for f in range(2)]
    res = copies(anns, lambda a: a['object_id'] in ('o0', 'o1', 'o4'))

    def check(refs):
        for (key, c, o), per_level in refs[0]['trajectories']:
            if key[1] == 'ONE':
                assert per_level[2]['len'] == 1 and per_level[2]['frag'] == 0
        one = refs[0]['per_stream'][('seg', 'ONE')]
        assert one[1][2]['traj'] == 3 and one[1][2]['mt'] == 2 and one[1][2]['ml'] == 1 and one[1][1]['traj'] == 2
    return anns, [res], check


def _every_other_frame():
    anns = [ann(f, 'o1') for f in range(9)] + [ann(f, 'o2') for f in range(0, 9, 2)]
    res = copies(anns, by_pattern({'o1': '1', 'o2': '10101'}))

    def check(refs):
        st = stats_of(refs[0], 'o2')[2]
        assert st == {'len': 5, 'tracked': 3, 'frag': 2, 'idsw': 0}
        assert stats_of(refs[0], 'o1')[2] == {'len': 9, 'tracked': 9, 'frag': 0, 'idsw': 0}
    return anns, [res], check


def _level_changes():
    levels = {'o1': [1, 1, 2, 2, 1], 'o2': [1, 2, 2, 1], 'o3': [2, 2, 1, 1, 1], 'o4': [2, 2, 2]}
    anns = [ann(f, o, level=lv) for o, lvs in levels.items() for f, lv in enumerate(lvs)]
    res = copies(anns, by_pattern({'o1': '10001', 'o2': '1001', 'o3': '10101', 'o4': '101'}),
                 hyp_id=lambda a: 'h%s_%d' % (a['object_id'], frame_of(a) // 3))      # a new id from frame 3 on: a switch when matched again

    def check(refs):
        r = refs[0]
        assert stats_of(r, 'o1')[2] == {'len': 5, 'tracked': 2, 'frag': 1, 'idsw': 1}
        assert stats_of(r, 'o1')[1] == {'len': 3, 'tracked': 2, 'frag': 1, 'idsw': 1}
        assert stats_of(r, 'o2')[2]['frag'] == 1 and stats_of(r, 'o2')[1] == {'len': 2, 'tracked': 2, 'frag': 0, 'idsw': 1}
        assert stats_of(r, 'o3')[2] == {'len': 5, 'tracked': 3, 'frag': 2, 'idsw': 1}
        assert stats_of(r, 'o3')[1] == {'len': 3, 'tracked': 2, 'frag': 1, 'idsw': 1}
        assert stats_of(r, 'o4')[1]['len'] == 0 and stats_of(r, 'o4')[2]['frag'] == 1
        assert r['table'][1][1]['traj'] == 3 and r['table'][1][2]['traj'] == 4
    return anns, [res], check


def _ratio_bounds():
    spec = {'o1': (5, 4, 'mt'), 'o2': (5, 1, 'pt'), 'o3': (5, 0, 'ml'), 'o4': (10, 8, 'mt'), 'o5': (10, 7, 'pt'), 'o6': (10, 2, 'pt'),
            'o7': (10, 1, 'ml'), 'o8': (6, 1, 'ml'), 'o9': (15, 12, 'mt'), 'o10': (15, 11, 'pt'), 'o11': (15, 3, 'pt'), 'o12': (15, 2, 'ml')}
    anns = [ann(f, o) for o, (n, _, _) in spec.items() for f in range(n)]
    res = copies(anns, lambda a: frame_of(a) < spec[a['object_id']][1])

    def check(refs):
        for o, (n, k, cls) in spec.items():
            st = stats_of(refs[0], o)[2]
            assert (st['len'], st['tracked']) == (n, k) and coverage_ref.classify(st) == cls, o
        assert [refs[0]['table'][1][2][f] for f in ('traj', 'mt', 'pt', 'ml')] == [12, 3, 5, 4]
    return anns, [res], check


def _last_class_empty():
    anns = []
    for cam, cats in (('A', (1, 2)), ('B', (1,)), ('C', (2, 4)), ('D', (1, 2))):
        for f in range(4):
            anns += [ann(f, 'o%d' % (10 * c + i), cat=c, cam=cam) for c in cats for i in range(3)]
    res = copies(anns, by_pattern(dict(('o%d' % (10 * c + i), p) for c in (1, 2, 4) for i, p in enumerate(('1011', '0100', '1101')))))

    def check(refs):
        r = refs[0]
        assert [r['per_stream'][('seg', cam)][4][2]['traj'] for cam in 'ABCD'] == [0, 0, 3, 0]
        assert r['per_stream'][('seg', 'B')][2][2]['traj'] == 0
        assert r['table']['ALL'][2]['traj'] == 21 and r['table']['ALL'][2]['frag'] == 14
    return anns, [res], check


def _three_results(images_step=None):
    anns = [ann(f, 'o%d' % i, cat=(1, 2, 4)[i % 3], level=1 + ((i + f) % 5 == 0)) for f in range(8) for i in range(7) if (i + f) % 4]
    full = copies(anns, lambda a: True)
    holes = copies(anns, lambda a: (frame_of(a) + int(a['object_id'][1:])) % 3 != 1, hyp_id=lambda a: 'h%s_%d' % (a['object_id'], frame_of(a) // 4))
    stray = [dict(r, image_id='seg/%d/FRONT' % (100 + i)) for i, r in enumerate(full[:3])] + [dict(full[0], image_id='other/0/FRONT')]
    results = [full + stray, [], holes]
    gt = {'annotations': anns, 'images': [{'id': 'seg/%d/FRONT' % f} for f in range(0, 8, images_step or 1)]}

    def check(refs):
        assert len(results[0]) != len(results[2]) and refs[0]['ignored_rows'] >= 4
        t0, t1, t2 = (r['table']['ALL'][2] for r in refs)
        assert t0['traj'] == t1['traj'] == t2['traj'] == 7
        assert t0['mt'] == 7 and t0['frag'] == 0 and t1['ml'] == 7 and t2['frag'] > 0 and t2['pt'] > 0
        assert sum(st[2]['idsw'] for _, st in refs[2]['trajectories']) > 0
        if images_step:
            assert t0['frag'] == 0 and sum(st[2]['len'] for _, st in refs[0]['trajectories']) < len(anns) * 0.6
            assert refs[0]['ignored_rows'] > len(stray)
    return gt, results, check


CASES = {
    'frame_sizes': _frame_sizes,
    'trajectory_counts': _trajectory_counts,
    'one_frame_stream': _one_frame_stream,
    'every_other_frame': _every_other_frame,
    'level_changes': _level_changes,
    'ratio_bounds': _ratio_bounds,
    'last_class_empty': _last_class_empty,
    'three_results': _three_results,
    'three_results_every_other_image': lambda: _three_results(2),
}


def case(name):
    """(gt_json, [result rows, ...], check, [coverage_ref output per result]) - the reference is computed once and shared."""
    if name not in _REFS:
        gt, results, check = CASES[name]()
        _REFS[name] = (gt, results, check, [coverage_ref.evaluate(gt, r) for r in results])
    return _REFS[name]
