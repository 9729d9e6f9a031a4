"""TEST INFRASTRUCTURE ONLY - plain Python restatement of the trajectory coverage table.

The matching is ``mot_ref.evaluate`` (CLEAR-MOT, frame by frame); everything else is derived here with dicts and lists: what
became of every ground-truth trajectory (rows, matched rows, fragmentations, identity switches) at both difficulty levels and the
mostly tracked / partially tracked / mostly lost counts.  Nothing is shared with waymo_2d_tracking_amd/tracking/evaluate.py or
csrc/mot_coverage.hip, which the GPU tests compare against this file.
"""
import math

import mot_ref

DEFAULT_IOU_THRESHOLD = mot_ref.DEFAULT_IOU_THRESHOLD
ALL_CLASSES = (1, 2, 4)
COV_FIELDS = ('traj', 'mt', 'pt', 'ml', 'frag')
TRAJ_FIELDS = ('len', 'tracked', 'frag', 'idsw')


def fragmentations(flags):
    """Runs of 0 with a 1 somewhere before and somewhere after."""
    ones = [i for i, v in enumerate(flags) if v]
    if not ones:
        return 0
    inner = flags[ones[0]:ones[-1] + 1]
    return sum(1 for a, b in zip(inner, inner[1:]) if a and not b)


def trajectory_stats(rows):
    """rows: (matched, switch) of a trajectory's rows at one level, in frame order."""
    flags = [1 if m else 0 for m, _ in rows]
    return {'len': len(rows), 'tracked': sum(flags), 'frag': fragmentations(flags), 'idsw': sum(1 for m, s in rows if m and s)}


def classify(stats):
    """'mt', 'pt' or 'ml' by the 0.8 / 0.2 bounds, in integers."""
    if 5 * stats['tracked'] >= 4 * stats['len']:
        return 'mt'
    if 5 * stats['tracked'] < stats['len']:
        return 'ml'
    return 'pt'


def finish(c):
    out = dict(c)
    out['MT'] = c['mt'] / c['traj'] if c['traj'] else math.nan
    out['ML'] = c['ml'] / c['traj'] if c['traj'] else math.nan
    out['FM'] = c['frag']
    return out


def evaluate(gt_json, result_rows, iou_threshold=DEFAULT_IOU_THRESHOLD):
    """Returns a dict:
        per_stream[(segment, camera)][category][level] -> traj, mt, pt, ml, frag
        table[category or 'ALL'][level]                -> the same added, + MT, ML, FM
        trajectories   list of ((stream key, category, object id), {1: stats, 2: stats}), stats = len, tracked, frag, idsw:
                       streams in order of first appearance, classes ascending, object ids as sorted strings
        ignored_rows, stream_keys."""
    n_classes = len(iou_threshold)
    mot = mot_ref.evaluate(gt_json, result_rows, iou_threshold)
    matched = {}                                     # annotation index -> switch
    for m, s in zip(mot['hyp_match'], mot['hyp_switch']):
        if m >= 0:
            assert m not in matched
            matched[m] = s
    annotations = gt_json['annotations'] if isinstance(gt_json, dict) else gt_json
    images = gt_json.get('images') if isinstance(gt_json, dict) else None
    frames = {}
    for item in (images if images is not None else annotations):
        key, fr = mot_ref._split(item['id'] if images is not None else item['image_id'])
        frames.setdefault(key, set()).add(fr)
    trajs = {}                                       # (stream key, category, object id) -> [(frame, annotation index, level)]
    for idx, a in enumerate(annotations):
        key, fr = mot_ref._split(a['image_id'])
        if key not in frames or fr not in frames[key] or a['bbox'][2] < 1 or a['bbox'][3] < 1:
            continue
        if not (1 <= a['category_id'] <= n_classes):
            continue
        level = 2 if a.get('tracking_difficulty_level', 1) == 2 else 1
        trajs.setdefault((key, a['category_id'], str(a['object_id'])), []).append((fr, idx, level))
    stream_pos = dict((key, i) for i, key in enumerate(frames))
    per_stream = dict((key, dict((c, {1: dict((f, 0) for f in COV_FIELDS), 2: dict((f, 0) for f in COV_FIELDS)})
                                 for c in range(1, n_classes + 1))) for key in frames)
    trajectories = []
    for tkey in sorted(trajs, key=lambda k: (stream_pos[k[0]], k[1], k[2])):
        rows = sorted(trajs[tkey])
        assert len(set(fr for fr, _, _ in rows)) == len(rows), 'object twice in a frame: %r' % (tkey,)
        per_level = {}
        for lv in (1, 2):
            mine = [(idx in matched, matched.get(idx, 0)) for fr, idx, level in rows if lv == 2 or level != 2]
            st = trajectory_stats(mine)
            per_level[lv] = st
            if st['len']:
                cnt = per_stream[tkey[0]][tkey[1]][lv]
                cnt['traj'] += 1
                cnt[classify(st)] += 1
                cnt['frag'] += st['frag']
        trajectories.append((tkey, per_level))
    table = {}
    for c in list(range(1, n_classes + 1)) + ['ALL']:
        table[c] = {}
        for lv in (1, 2):
            tot = dict((f, 0) for f in COV_FIELDS)
            for cc in ([c] if c != 'ALL' else [x for x in ALL_CLASSES if x <= n_classes]):
                for key in frames:
                    for f in COV_FIELDS:
                        tot[f] += per_stream[key][cc][lv][f]
            table[c][lv] = finish(tot)
    return {'per_stream': per_stream, 'table': table, 'trajectories': trajectories, 'ignored_rows': mot['ignored_rows'],
            'stream_keys': list(frames), 'mot': mot}
