"""GPU JPEG decoder (csrc/jpeg_decode.hip) on the parts of it that tests/test_gpu_jpeg.py never enters, bit-exact against PIL:
the "chain not settled" loop of wd_jpeg_decode_rgb_u8 (more synchronisation rounds, then the whole tail a second time), the
multi-pass loops of the two single-workgroup scans with a restart segment across / exactly at a pass boundary, restart segments
that end on or next to a subsequence boundary, and the range-limit arms of the inverse DCT.  tests/test_jpeg_cases.py (CPU) pins
every file to the property it is here for."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_cases as JC                                                                      # noqa: E402

pytestmark = pytest.mark.gpu

_PIL = {}


def pil(name, data):
    """PIL's decode of a case, computed once and never written to"""
    if name not in _PIL:
        _PIL[name] = JC.pil_rgb(data)
        _PIL[name].setflags(write=False)
    return _PIL[name]


def decode(data, out=None):
    """-> (image as numpy, rounds, [launches, most iterations of a workgroup, subsequence decodes, subsequences]) of this call"""
    from waymo_2d_tracking_amd import _lib
    from waymo_2d_tracking_amd.detnet.nn import ops
    got, rounds = ops.jpeg_decode(data, return_rounds=True, out=out)
    st = (ctypes.c_int32 * 4)()
    assert _lib.lib().wd_jpeg_last_stats(st) == 0
    return got.cpu().numpy(), rounds, list(st)


def ids(cases):
    return [name for name, _ in cases]


SLOW = JC.slow_sync_cases()
FAST = ('fast_241x323', JC.encode(JC.synth(241, 323, 2, seed=241), quality=75, subsampling=2))


@pytest.mark.parametrize('prefill', [False, True], ids=['fresh', 'into_out'])
def test_context_reuse_around_the_extra_round_loop(prefill):
    """one thread = one scratch context: fast, slow, fast, a larger slow file, grayscale, fast.  The larger file needs more than
    the 25 % of slack the context allocates, so a context that has seen nothing larger grows there (this test is the first of the
    file for that reason)."""
    by_name = dict(SLOW)
    small, large, gray = 'tiled_gray_256x256_q100', 'tiled_rgb_384x384_q100_s2', 'tiled_gray_384x384_q100'
    assert len(by_name[large]) > 2 * len(by_name[small]) > 4 * len(FAST[1])
    order = [FAST, (small, by_name[small]), FAST, (large, by_name[large]), (gray, by_name[gray]), FAST]
    for step, (name, data) in enumerate(order):
        exp = pil(name, data)
        out = torch.full(exp.shape, 0xAB, dtype=torch.uint8, device='cuda') if prefill else None
        got, rounds, stats = decode(data, out=out)
        assert np.array_equal(got, exp), (step, name)
        if prefill:
            assert np.array_equal(out.cpu().numpy(), exp), (step, name)
        assert (rounds == 2) if name == FAST[0] else (rounds > 2), (step, name, rounds)
        assert stats[0] == rounds and stats[3] == JC.subsequence_layout(data)[1], (step, name, stats)


@pytest.mark.parametrize('name,data', SLOW, ids=ids(SLOW))
def test_unsettled_chain_takes_more_rounds_and_the_second_tail_is_exact(name, data):
    nsub = JC.subsequence_layout(data)[1]
    got, rounds, stats = decode(data)
    print(name, 'bytes', len(data), 'subsequences', nsub, 'rounds', rounds, 'bound', JC.round_bound(nsub), 'stats', stats)
    assert np.array_equal(got, pil(name, data))
    assert 2 < rounds <= JC.round_bound(nsub) and (rounds - 2) % 4 == 0, (rounds, JC.round_bound(nsub))
    assert stats[0] == rounds and stats[3] == nsub, stats


def test_image_loader_with_slow_files_among_fast_ones(tmp_path):
    from waymo_2d_tracking_amd.detnet.inference import ImageLoader
    by_name = dict(SLOW)
    files = [JC.encode(JC.synth(120 + 16 * i, 200 + 24 * i, 2, seed=i), quality=70 + 5 * i, subsampling=(2, 1, 0)[i % 3]) for i in range(5)]
    for at, name in ((1, 'tiled_gray_640x640_q75'), (4, 'tiled_rgb_256x256_q100_s0'), (5, 'tiled_rgb_384x384_q100_s2_r400')):
        files.insert(at, by_name[name])
    assert len(files) == 8
    items = []
    for i, data in enumerate(files):
        path = str(tmp_path / ('%02d.jpg' % i))
        with open(path, 'wb') as f:
            f.write(data)
        items.append((i, path))
    gpu = list(ImageLoader(items, workers=4, depth=6, decoder='gpu'))
    host = list(ImageLoader(items, workers=4, depth=6, decoder='pil'))
    assert [g[0] for g in gpu] == list(range(8)) == [h[0] for h in host]
    for (ia, ta, sa), (ib, tb, sb) in zip(gpu, host):
        assert sa == sb and ta.is_cuda and ta.dtype == torch.uint8 and torch.equal(ta.cpu(), tb.cpu()), ia


def test_truncated_slow_file_raises_and_the_whole_file_decodes_afterwards():
    from waymo_2d_tracking_amd._lib import WaymoTrackError
    from waymo_2d_tracking_amd.detnet.nn import ops
    name, data = SLOW[4]
    with pytest.raises(WaymoTrackError, match='truncated|ends before'):
        ops.jpeg_decode(data[:len(data) // 2])
    got, rounds, stats = decode(data)
    assert np.array_equal(got, pil(name, data)) and rounds > 2


SCAN = JC.scan_pass_cases()


def test_scan_pass_family_is_complete():
    assert [n.split('_640x648')[0] for n in ids(SCAN)] == ['spans', 'starts_at_4096', 'starts_at_8192'], ids(SCAN)


@pytest.mark.parametrize('name,data', SCAN, ids=ids(SCAN))
def test_restart_segment_across_or_at_a_pass_boundary_of_the_scans(name, data):
    first, nsub = JC.subsequence_layout(data)
    assert nsub > JC.RESOLVE_PASS
    got, rounds, stats = decode(data)
    print(name, 'bytes', len(data), 'segments', len(first) - 1, 'subsequences', nsub, 'rounds', rounds, 'stats', stats)
    assert np.array_equal(got, pil(name, data))
    assert rounds == 2 and stats[0] == 2 and stats[3] == nsub, (rounds, stats)


def test_restart_segments_ending_on_or_next_to_a_subsequence_boundary():
    cases = JC.segment_edge_cases()
    assert len(cases) == 9, ids(cases)
    bad = []
    for name, data in cases:
        got, rounds, stats = decode(data)
        print(name, 'bytes', len(data), 'segment bytes', JC.segment_byte_counts(data), 'rounds', rounds, 'stats', stats)
        if got.shape != pil(name, data).shape or not np.array_equal(got, pil(name, data)) or rounds != 2 or \
                stats[3] != JC.subsequence_layout(data)[1]:
            bad.append((name, rounds, stats))
    assert not bad, bad


def test_saturated_content_at_very_low_quality():
    cases = JC.low_quality_cases()
    assert len(cases) == 12
    bad = []
    for name, data in cases:
        got, rounds, stats = decode(data)
        print(name, 'bytes', len(data), 'rounds', rounds, 'stats', stats)
        if not np.array_equal(got, pil(name, data)):
            bad.append(name)
    assert not bad, bad
