"""The adversarial layouts of tests/coverage_cases.py are what they claim to be: every case's property holds on the reference
(tests/coverage_ref.py) alone, and so do the sums that tie the table to CLEAR-MOT."""
import pytest

import coverage_cases


@pytest.mark.parametrize('name', sorted(coverage_cases.CASES))
def test_case_hits_its_property(name):
    gt, results, check, refs = coverage_cases.case(name)
    assert len(refs) == len(results) >= 1
    check(refs)
    for ref in refs:
        for c in (1, 2, 3, 4):
            for lv in (1, 2):
                row, mot = ref['table'][c][lv], ref['mot']['table'][c][lv]
                assert row['mt'] + row['pt'] + row['ml'] == row['traj']
                mine = [st[lv] for (_, cc, _), st in ref['trajectories'] if cc == c]
                assert sum(s['len'] for s in mine) == mot['gt'] and sum(s['tracked'] for s in mine) == mot['tp']
                assert sum(s['idsw'] for s in mine) == mot['idsw'] and sum(s['frag'] for s in mine) == row['frag']
                assert sum(1 for s in mine if s['len']) == row['traj']
