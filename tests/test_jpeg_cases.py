"""CPU side of tests/test_gpu_jpeg_edges.py: every case family of tests/jpeg_cases.py is pinned to what its name claims - the
slow-sync files really take the extra synchronisation rounds (emulated thread by thread, tests/native/jpeg_sync_emul.cpp), the
segment-edge files really end on / next to a subsequence boundary, the scan-pass files really put a restart segment across /
exactly at a pass boundary of the two single-workgroup scans - and on every file the emulated parallel decode gives the
coefficients of the sequential restatement (oracle/jpeg_ref.py).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_cases as JC                                                                      # noqa: E402
from oracle import jpeg_ref as J                                                             # noqa: E402


@pytest.fixture(scope='module')
def emul(tmp_path_factory):
    return JC.emulator(tmp_path_factory.mktemp('jpeg_cases'))


def ids(cases):
    return [name for name, _ in cases]


SLOW = JC.slow_sync_cases()
# emulated rounds every slow-sync file needs at least: 10 (7 to 9 workgroups), but for the one file of 4 workgroups
MIN_ROUNDS = {'tiled_gray_256x256_q100': 6}


def test_layout_helpers_on_known_streams():
    assert JC.round_bound(1) == 2 and JC.round_bound(512) == 2 and JC.round_bound(513) == 6 and JC.round_bound(785) == 6
    assert JC.round_bound(1536) == 6 and JC.round_bound(1537) == 10 and JC.round_bound(2560) == 10 and JC.round_bound(2561) == 14
    assert JC.round_bound(12545) == 50
    # a hand-made scan: 3 bytes + a stuffed FF, RST0, 130 bytes, RST1, one byte, a fill FF in front of EOI
    head = JC.encode(JC.synth(8, 8, 0), quality=50)
    head = head[:head.find(b'\xff\xda')]
    sos = b'\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00'
    scan = b'\x01\x02\x03\xff\x00' + b'\xff\xd0' + bytes([7]) * 130 + b'\xff\xd1' + b'\x09' + b'\xff\xff\xd9'
    assert JC.segment_byte_counts(head + sos + scan) == [4, 130, 1]
    assert JC.subsequence_layout(head + sos + scan) == ([0, 1, 3, 4], 4)
    assert JC.tiled(20, 40, 1).shape == (20, 40) and JC.tiled(20, 40, 3).shape == (20, 40, 3)
    t = JC.tiled(48, 48, 3)
    assert np.array_equal(t[:16, :16], t[16:32, 32:48]) and len(np.unique(t)) > 100


def test_slow_sync_family_is_complete():
    names = ids(SLOW)
    assert names[:7] == ['tiled_gray_256x256_q100', 'tiled_gray_384x384_q100', 'tiled_gray_640x640_q75', 'tiled_rgb_256x256_q100_s0',
                         'tiled_rgb_384x384_q100_s2', 'tiled_rgb_250x390_q100_s1', 'tiled_rgb_384x384_q100_s2_r400']
    assert len(names) == len(set(names)) == 8 and names[7].endswith('_opt'), names   # this encoder gives an optimised one as well
    info = J.parse(SLOW[7][1])
    assert info['width'] <= 400 and info['height'] <= 400
    assert info['dc'][0] != J.parse(SLOW[4][1])['dc'][0]                              # its tables are its own, not Annex K's


@pytest.mark.parametrize('name,data', SLOW, ids=ids(SLOW))
def test_slow_sync_file_takes_the_extra_rounds(emul, name, data):
    exp = JC.sequential_coefficients(data)
    nsub = JC.subsequence_layout(data)[1]
    got, rounds, geo = emul(data, 256)
    print(name, 'bytes', len(data), 'subsequences', nsub, 'emulated rounds', rounds, 'bound', JC.round_bound(nsub))
    assert geo[6] == nsub
    assert got.shape == exp.shape and np.array_equal(got, exp)
    assert rounds >= MIN_ROUNDS.get(name, 10) and (rounds - 2) % 4 == 0 and rounds == JC.round_bound(nsub), (rounds, nsub)
    small, rounds4, _ = emul(data, 4)
    assert np.array_equal(small, exp) and rounds4 > rounds


def test_segment_edge_search_finds_all_nine_classes(emul):
    cases = JC.segment_edge_cases()
    assert [n.split('_')[:2] for n, _ in cases] == [['seg%d' % r, p] for r in JC.EDGE_RESIDUES for p in JC.EDGE_POSITIONS]
    compared = 0
    for name, data in cases:
        residue, position = int(name.split('_')[0][3:]), name.split('_')[1]
        counts = JC.segment_byte_counts(data)
        hits = [s for s, b in enumerate(counts) if b % 128 == residue]
        if position == 'only':
            assert len(counts) == 1 and hits == [0], (name, counts)
        elif position == 'last':
            assert len(counts) > 2 and len(counts) - 1 in hits, (name, counts)
        else:
            assert len(counts) > 2 and any(0 < s < len(counts) - 1 for s in hits), (name, counts)
        info = J.parse(data)
        assert [len(s) for s in info['segments']] == counts, name                      # the restatement's own unstuffing agrees
        if info['width'] * info['height'] <= 5000:
            assert np.array_equal(J.decode_rgb(data), JC.pil_rgb(data)), name
            compared += 1
        got, rounds, geo = emul(data, 256)
        assert geo[6] == JC.subsequence_layout(data)[1] and geo[7] == len(counts), name
        assert np.array_equal(got, JC.sequential_coefficients(data)), name
        assert np.array_equal(emul(data, 4)[0], got), name
        assert rounds == 2, (name, rounds)
    assert compared >= 7                                                              # the search prefers files of that size


SCAN = JC.scan_pass_cases()


def test_scan_pass_family_is_complete():
    assert [n.split('_640x648')[0] for n in ids(SCAN)] == ['spans', 'starts_at_4096', 'starts_at_8192'], ids(SCAN)


@pytest.mark.parametrize('name,data', SCAN, ids=ids(SCAN))
def test_scan_pass_file_puts_a_segment_where_it_says(emul, name, data):
    first, nsub = JC.subsequence_layout(data)
    assert nsub > JC.RESOLVE_PASS
    starts = set(first[:-1])
    if name.startswith('spans'):
        assert len(first) - 1 == 3 and JC.SCAN_PASS not in starts and JC.RESOLVE_PASS not in starts
        # the segment around 4096 began in the first pass of jpeg_scan_kernel, the one around 8192 inside the first pass of both
        # scans and behind another segment: what either scan carries into its next pass is a live segmented value
        seg_start = lambda at: max(f for f in first[:-1] if f <= at)
        assert seg_start(JC.SCAN_PASS) < JC.SCAN_PASS and 0 < seg_start(JC.RESOLVE_PASS) < JC.RESOLVE_PASS
    else:
        at = int(name.split('_')[2])
        assert len(first) - 1 == 81 and at in starts and at in (JC.SCAN_PASS, JC.RESOLVE_PASS)
    got, rounds, geo = emul(data, 256)
    assert geo[6] == nsub and geo[7] == len(first) - 1 and rounds == 2
    assert np.array_equal(got, JC.sequential_coefficients(data))


def unlimited_samples(coef, quant):
    """oracle/jpeg_ref.py idct_islow without its last step: the signed samples (level shift not yet added) in front of the range limit"""
    x = coef.astype(np.int64) * quant.astype(np.int64)
    x = x.reshape(x.shape[:-1] + (8, 8))
    ws = np.stack(J._pass(*[x[..., r, :] for r in range(8)], 13, 13 - 2), axis=-2)
    return np.stack(J._pass(*[ws[..., :, c] for c in range(8)], 13, 13 + 2 + 3), axis=-1)


def test_low_quality_files_saturate_and_equal_pil(emul):
    cases = JC.low_quality_cases()
    assert len(cases) == len(set(ids(cases))) == 12
    for name, data in cases:
        info = J.parse(data)
        assert (info['width'], info['height']) == (56, 40)
        assert np.array_equal(J.decode_rgb(data), JC.pil_rgb(data)), name
        # full-swing content under coarse quantisation rings: samples in front of the range limit leave 0 .. 255 on both sides (the
        # 255 arm and the 0 arm of jpeg_idct_kernel).  With the green channel inverted the swing is in the chroma planes (magenta
        # against green); luma stays between 105 and 150.
        planes = J.decode_coefficients(info)
        v = [unlimited_samples(p, info['qt'][c['tq']]) + 128 for p, c in zip(planes, info['comps'])]
        lo, hi = min(int(x.min()) for x in v), max(int(x.max()) for x in v)
        print(name, 'samples before the range limit: %d .. %d' % (lo, hi))
        assert lo < 0 and hi > 255, (name, lo, hi)
        got, rounds, geo = emul(data, 256)
        assert geo[6] == JC.subsequence_layout(data)[1] and rounds == 2, (name, rounds)
