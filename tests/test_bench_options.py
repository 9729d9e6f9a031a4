"""bench.py's command line without a GPU: a plain run leaves the checks to --full, and --dump-outputs writes float32 / float64 .npy
files within its size limit, sampling the same rows on every run.  CPU only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                                                  # noqa: E402


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + list(argv))
    return bench.parse_args()


def test_plain_run_leaves_oracle_and_cpu_baseline_to_full(monkeypatch):
    a = _args(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
    assert not a.full and a.no_verify and a.no_cpu_baseline and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None
    a = _args(monkeypatch, '--full', '--dump-outputs', 'out')
    assert a.full and not a.no_verify and not a.no_cpu_baseline and a.dump_outputs == 'out'
    a = _args(monkeypatch, '--full', '--no-verify')
    assert a.no_verify and not a.no_cpu_baseline
    with pytest.raises(SystemExit):
        _args(monkeypatch, '--steps', '0')


def test_dump_outputs_types_and_values(tmp_path):
    ids = np.array([0, 5, 2 ** 40], np.int64)
    names = bench.dump_outputs(str(tmp_path), dict(ids=ids, img=np.arange(12, dtype=np.uint8).reshape(2, 2, 3),
                                                   box=np.array([[1.5, 2.25]]), f=np.ones(3, np.float32)))
    assert names == ['box', 'f', 'ids', 'img']
    got = {n: np.load(str(tmp_path / (n + '.npy'))) for n in names}
    assert got['ids'].dtype == np.float64 and np.array_equal(got['ids'], ids)
    assert got['img'].dtype == np.float32 and np.array_equal(got['img'], np.arange(12).reshape(2, 2, 3))
    assert got['box'].dtype == np.float64 and got['f'].dtype == np.float32


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_samples_large_outputs_the_same_way_every_time(tmp_path):
    n = 3 * 2 ** 20
    rows = {'a': np.arange(n * 4, dtype=np.float64).reshape(n, 4), 'b': np.arange(n, dtype=np.int64), 'small': np.arange(10)}
    for d in ('one', 'two'):
        bench.dump_outputs(str(tmp_path / d), rows)
    files = sorted(os.listdir(str(tmp_path / 'one')))
    assert files == ['a.npy', 'b.npy', 'sample_rows_%d.npy' % n, 'small.npy']
    assert _dir_bytes(str(tmp_path / 'one')) <= 64 * 10 ** 6
    load = lambda d, f: np.load(str(tmp_path / d / f))
    for f in files:
        assert np.array_equal(load('one', f), load('two', f)), f
    idx = load('one', 'sample_rows_%d.npy' % n).astype(np.int64)
    assert np.array_equal(load('one', 'b.npy'), idx) and np.array_equal(load('one', 'a.npy')[:, 0], 4.0 * idx)
    assert np.array_equal(load('one', 'small.npy'), np.arange(10))


def test_dump_outputs_budget_counts_the_row_numbers(tmp_path):
    """several long 1-D columns of one length (the track stage's output at many segments) and a second length: the samples and their row
    numbers together stay within 64 MB, and each length's row numbers are written once"""
    n, m = 6 * 2 ** 20, 5 * 2 ** 20
    cols = {'c%d' % i: np.arange(n, dtype=np.int64) + i for i in range(4)}
    cols.update(f0=np.ones(n, np.float32), f1=np.zeros(n, np.float32), other=np.arange(m, dtype=np.int32))
    names = bench.dump_outputs(str(tmp_path), cols)
    assert [x for x in names if x.startswith('sample_rows_')] == ['sample_rows_%d' % m, 'sample_rows_%d' % n]
    total = _dir_bytes(str(tmp_path))
    assert 48 * 2 ** 20 < total <= 64 * 10 ** 6, total
    idx = np.load(str(tmp_path / ('sample_rows_%d.npy' % n))).astype(np.int64)
    assert np.array_equal(np.load(str(tmp_path / 'c3.npy')), idx + 3.0)
