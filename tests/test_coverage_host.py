"""Host side of the trajectory coverage table (tracking/evaluate.py): the parser's new flags, the reported row, the printed table
and the JSON form.  No device is touched."""
import json
import math

import numpy as np
import pytest


def test_parser_takes_coverage_and_rank_by_mt():
    from waymo_2d_tracking_amd.tracking import evaluate as E
    parser = E.build_parser()
    args = parser.parse_args(['--annotations', 'gt.json', 'a.json', 'b.json', '--coverage'])
    assert args.coverage and args.tracks == ['a.json', 'b.json'] and args.rank_by == 'mota' and not args.identity and not args.hota
    assert not parser.parse_args(['--annotations', 'gt.json', 'a.json']).coverage
    args = parser.parse_args(['--annotations', 'gt.json', '--sweep', 'det.json', '--rank-by', 'mt'])
    assert args.rank_by == 'mt' and args.sweep == 'det.json'
    for value in ('idf1', 'hota', 'mota'):
        assert parser.parse_args(['--annotations', 'gt.json', '--rank-by', value]).rank_by == value
    with pytest.raises(SystemExit):
        parser.parse_args(['--annotations', 'gt.json', '--rank-by', 'ml'])


def test_public_names_and_defaults():
    import inspect
    from waymo_2d_tracking_amd.tracking import evaluate as E
    assert E.COV_FIELDS == ('traj', 'mt', 'pt', 'ml', 'frag')
    assert inspect.signature(E.sweep).parameters['coverage'].default is False
    assert inspect.signature(E.evaluate_coverage).parameters['per_trajectory'].default is False


def test_coverage_row():
    from waymo_2d_tracking_amd.tracking import evaluate as E
    row = E.coverage_row(8, 2, 5, 1, 13)
    assert row == {'traj': 8, 'mt': 2, 'pt': 5, 'ml': 1, 'frag': 13, 'MT': 0.25, 'ML': 0.125, 'FM': 13}
    assert all(isinstance(row[f], int) for f in E.COV_FIELDS + ('FM',))
    empty = E.coverage_row(*np.zeros(5, np.int64))
    assert empty['traj'] == 0 and math.isnan(empty['MT']) and math.isnan(empty['ML']) and empty['FM'] == 0


def _result():
    from waymo_2d_tracking_amd.tracking import evaluate as E
    counts = np.zeros((2, 4, 2, 5), np.int64)                  # two streams, four classes
    counts[0, 0] = [[3, 1, 1, 1, 2], [4, 2, 1, 1, 3]]
    counts[1, 0] = [[1, 1, 0, 0, 0], [1, 0, 0, 1, 0]]
    counts[1, 1] = [[0, 0, 0, 0, 0], [2, 0, 2, 0, 5]]
    counts[0, 2] = [[9, 9, 0, 0, 9], [9, 9, 0, 0, 9]]          # class 3 is not part of ALL
    counts[1, 3] = [[5, 0, 0, 5, 0], [5, 0, 0, 5, 0]]
    return E.CoverageResult(counts, 7, [('seg', 'A'), ('seg', 'B')])


def test_result_table_adds_streams_and_the_three_classes():
    r = _result()
    assert r.table[1][2] == {'traj': 5, 'mt': 2, 'pt': 1, 'ml': 2, 'frag': 3, 'MT': 0.4, 'ML': 0.4, 'FM': 3}
    assert r.table[1][1]['traj'] == 4 and r.table[1][1]['mt'] == 2
    assert r.table[2][1]['traj'] == 0 and math.isnan(r.table[2][1]['MT'])
    assert r.table['ALL'][2] == {'traj': 12, 'mt': 2, 'pt': 3, 'ml': 7, 'frag': 8, 'MT': 2 / 12, 'ML': 7 / 12, 'FM': 8}
    assert r.table['ALL'][1]['traj'] == 9
    assert r.mt() == 2 / 12 and r.mt(level=1, category=1) == 0.5
    assert r.traj_stats is None and r.traj_keys is None


def test_printed_table_and_json():
    from waymo_2d_tracking_amd.tracking import evaluate as E
    r = _result()
    lines = E.format_coverage_table(r, 'tracks.json').split('\n')
    assert lines[0] == 'tracks.json  coverage' and lines[1].split() == ['class', 'level', 'traj', 'mt', 'pt', 'ml', 'MT', 'ML', 'FM']
    assert len(lines) == 2 + 5 * 2
    assert lines[2].split() == ['1', 'LEVEL_1', '4', '2', '1', '1', '0.50000', '0.25000', '2']
    assert lines[-1].split() == ['ALL', 'LEVEL_2', '12', '2', '3', '7', '0.16667', '0.58333', '8']
    assert lines[4].split()[-3:] == ['nan', 'nan', '0']
    doc = json.loads(json.dumps(r.as_json()))
    assert doc['ignored_rows'] == 7 and sorted(doc['table']) == ['1', '2', '3', '4', 'ALL']
    assert doc['table']['ALL']['LEVEL_2']['frag'] == 8 and doc['table']['1']['LEVEL_2']['MT'] == 0.4
