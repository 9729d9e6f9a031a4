"""What the tracking-metric GPU tests (tests/test_gpu_mot*.py) and the sweep tests of the track post-passes share: the tracker
settings, the tracked rows, and the comparators of a result with its plain-Python restatement.

The HOTA comparator: hota_counts (gt, hyp, tp[19]) must be EQUAL to the restatement for every stream, class and level.  Of
hota_sums, loc is added in the restatement's order and must be equal too; ass / assre / asspr are sums of non-negative terms that
are bit-equal on both sides and differ only in the order they are added in, so they may differ by the standard bound for such a
sum, relative 2 n 2^-53 with n its number of terms; the table values get the same bound with 64 added to n (the module text of
tests/test_gpu_mot_hota.py).

This module is not rewritten by pytest: every assert carries what it compared as its message."""
import json
import math

import hota_ref
import mot_ref
from track_stage_support import predictions_of

SETTINGS = [                       # (max_age, min_hits, score thresholds, tracker IoU thresholds): three different results
    (2, 0, [0.3, 0.2, 1.0, 0.1], [0.01, 0.01, 1.0, 0.0]),
    (1, 1, [0.6, 0.6, 1.0, 0.6], [0.3, 0.3, 1.0, 0.3]),
    (3, 0, [0.0, 0.0, 0.0, 0.0], [0.1, 0.1, 0.1, 0.1]),
]
EPS = 2.0 ** -53


def _track(dets, max_age, min_hits, score_thr, iou_thr):
    """Detections list -> the rows tracking/track.py would write, through a JSON round trip like a file."""
    from waymo_2d_tracking_amd.tracking import utils as T
    packed = T.pack_streams(predictions_of(dets))
    out, _ = T.track_packed(packed, iou_thr, max_age, min_hits, score_thr)
    return json.loads(json.dumps(T.format_tracks(packed, out)))


def _copy_as_result(gt_json):
    return [{'image_id': a['image_id'], 'bbox': a['bbox'], 'score': 1.0, 'category_id': a['category_id'], 'object_id': a['object_id']}
            for a in gt_json['annotations'] if a['bbox'][2] >= 1 and a['bbox'][3] >= 1]


def same_number(a, b, rel=0.0):
    """equal, or both NaN, or - where a bound is given - within rel of b"""
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b or (rel > 0.0 and abs(a - b) <= rel * abs(b))


def assert_mot_equals_reference(got, ref, n_classes=4):
    """MotResult (per_row=True) == mot_ref.evaluate() output: everything, exactly."""
    assert got.stream_keys == ref['stream_keys'], 'stream_keys'
    for s, key in enumerate(got.stream_keys):
        for c in range(1, n_classes + 1):
            for li, lv in enumerate((1, 2)):
                exp = ref['per_stream'][key][c][lv]
                assert got.counts[s, c - 1, li].tolist() == [exp[f] for f in mot_ref.FIELDS], (key, c, lv)
                assert got.iou_sum[s, c - 1, li] == exp['iou_sum'], (key, c, lv, got.iou_sum[s, c - 1, li], exp['iou_sum'])
    assert got.hyp_match.tolist() == ref['hyp_match'], 'hyp_match'
    assert got.hyp_switch.tolist() == ref['hyp_switch'], 'hyp_switch'
    assert got.ignored_rows == ref['ignored_rows'], 'ignored_rows'
    for c, rows in ref['table'].items():
        for lv, row in rows.items():
            for name, v in row.items():
                assert same_number(got.table[c][lv][name], v), (c, lv, name, got.table[c][lv][name], v)


def assert_hota_equals_reference(got, ref, n_classes=4):
    """HotaResult == hota_ref.evaluate() output: counts, sums (see the module text), table and ignored rows."""
    assert got.stream_keys == ref['stream_keys'], 'stream_keys'
    most_terms = 0
    for s, key in enumerate(got.stream_keys):
        for c in range(1, n_classes + 1):
            for li, lv in enumerate((1, 2)):
                exp = ref['per_stream'][key][c][lv]
                assert got.hota_counts[s, c - 1, li].tolist() == [exp['gt'], exp['hyp']] + exp['tp'], (key, c, lv)
                sums = got.hota_sums[s, c - 1, li]
                assert sums[:, 3].tolist() == exp['loc'], (key, c, lv)
                for a in range(19):
                    n = exp['terms'][a]
                    most_terms = max(most_terms, n)
                    for q, name in enumerate(('ass', 'assre', 'asspr')):
                        assert same_number(float(sums[a, q]), exp[name][a], 2 * n * EPS), (key, c, lv, a, name, float(sums[a, q]), exp[name][a])
    assert got.ignored_rows == ref['ignored_rows'], 'ignored_rows'
    assert set(got.table) == set(ref['table']), 'table classes'
    rel = 2 * (most_terms * len(got.stream_keys) * n_classes + 64) * EPS
    for c, rows in ref['table'].items():
        for lv, row in rows.items():
            mine = got.table[c][lv]
            assert (mine['gt'], mine['hyp'], mine['tp']) == (row['gt'], row['hyp'], row['tp']), (c, lv, 'gt / hyp / tp')
            for name in hota_ref.NAMES + ('HOTA(0)', 'LocA(0)'):
                assert same_number(mine[name], row[name], rel), (c, lv, name, mine[name], row[name])
            for name in hota_ref.NAMES:
                assert all(same_number(x, y, rel) for x, y in zip(mine['per_alpha'][name], row['per_alpha'][name])), (c, lv, name)
