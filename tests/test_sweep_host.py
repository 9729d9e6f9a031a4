"""The host logic of tracking/evaluate.py's sweep - the enumeration order of the settings, the per-class pick, NaN-last and
grid-order ties, the defaults of classes that are not evaluated, the flag line, the table formatters and main()'s two paths -
replayed under the fakes of tests/sweep_fakes.py and compared, text for text, with tests/golden/sweep_characterization.json
(oracle/gen_golden_sweep.py).  The equality is exact: the ranking adds float64 sums in a defined order."""
import json
import os

import pytest

import sweep_fakes


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'sweep_characterization.json')) as fp:
        return json.load(fp)


@pytest.fixture(scope='module')
def replayed(tmp_path_factory):
    return sweep_fakes.run_cases(str(tmp_path_factory.mktemp('sweep')))


def test_every_recorded_item_is_replayed(golden, replayed):
    assert sorted(replayed) == sorted(golden)
    assert len(golden) == 91


CASES = (['base', 'base_with_defaults'] + ['only_' + name for name in sweep_fakes.SINGLE_PASS] +
         ['everything_by_' + rank_by for rank_by in ('mota', 'idf1', 'hota', 'mt')] +
         ['result_' + kind for kind in ('mot', 'identity', 'hota', 'coverage')] + ['main_sweep', 'main_tables'])


@pytest.mark.parametrize('case', CASES)
def test_case_equals_the_fixture(golden, replayed, case):
    names = [name for name in golden if name.split('/')[0] == case]
    assert names
    for name in names:
        assert replayed[name] == golden[name], name


def test_the_cases_cover_what_they_are_for(golden):
    assert len(json.loads(golden['base/settings'])) == 16
    assert all(set(row) == {'score', 'iou', 'max_age', 'min_hits'} for row in json.loads(golden['base_with_defaults/settings']))
    assert golden['base_with_defaults/settings'] == golden['base/settings']
    assert json.loads(golden['only_second/settings'])[2]['low_score'] == 0.3           # 0.5 clamped to the point's score
    assert golden['everything_by_mota/settings'] == golden['main_sweep/json/settings'] and golden['main_sweep/json/settings']['chars'] > 256 * 200
    for kind in ('mot', 'identity', 'hota'):                                           # a class without anything: NaN scores
        assert ' nan' in golden['result_%s/table' % kind]
    assert 'NaN' in golden['main_tables/json/tracks_b.json/table']
    log = json.loads(golden['everything_by_mota/log'])
    assert [e[0] for e in log[:10]] == ['track_packed_byte', 'split_tracks'] + ['stitch_tracks', 'dedup_tracks', 'refine_tracks', 'smooth_tracks'] * 2
    assert [e[1:3] for e in log[1:6]] == [[1, 2], [1, 2], [2, 4], [4, 8], [8, 16]]     # one split call, then per split output
