"""TEST INFRASTRUCTURE ONLY - plain Python / numpy restatement of the tracking metric ("Tracking metric").

CLEAR-MOT per (stream, class) and Waymo difficulty level, frame by frame, with dicts and lists: nothing is shared with
waymo_2d_tracking_amd/tracking/evaluate.py or csrc/mot_eval.hip, which the GPU tests compare against this file.
The assignment is ``oracle.thirdparty_restated.linear_assignment`` (the Munkres SORT uses, same tie-breaks).
"""
import math

import numpy as np

from oracle.thirdparty_restated import linear_assignment

DEFAULT_IOU_THRESHOLD = (0.7, 0.5, 0.5, 0.5)
ALL_CLASSES = (1, 2, 4)
FIELDS = ('gt', 'tp', 'fn', 'fp', 'idsw')


def iou(a, b):
    """tracking/sort/sort.py:34-47 on Python floats (IEEE double, one rounding per operation); boxes [x1, y1, x2, y2]."""
    xx1 = max(a[0], b[0])
    yy1 = max(a[1], b[1])
    xx2 = min(a[2], b[2])
    yy2 = min(a[3], b[3])
    w = xx2 - xx1
    w = w if w > 0. else 0.
    h = yy2 - yy1
    h = h if h > 0. else 0.
    wh = w * h
    return wh / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - wh)


def xyxy(bbox):
    x, y, w, h = (float(v) for v in bbox)
    return [x, y, x + w, y + h]


def gated_matrix(gboxes, hboxes, thr):
    G = np.zeros((len(gboxes), len(hboxes)), dtype=np.float32)
    for i, g in enumerate(gboxes):
        for j, h in enumerate(hboxes):
            v = iou(g, h)
            if v >= thr:
                G[i, j] = np.float32(v)
    return G


def assign(G):
    """Pairs (i, j) the Hungarian keeps on -G, entries with G > 0 only."""
    if G.shape[0] == 0 or G.shape[1] == 0:
        return []
    return [(int(i), int(j)) for i, j in linear_assignment(-G) if G[i, j] > 0]


def _split(image_id):
    segment, frame, camera = image_id.split('/')
    return (segment, camera), int(frame)


def _zero():
    return {'gt': 0, 'tp': 0, 'fn': 0, 'fp': 0, 'idsw': 0, 'iou_sum': 0.0}


def finish(c):
    """MOTA / MOTP of a count dict (NaN when the denominator is 0)."""
    out = dict(c)
    out['MOTA'] = 1.0 - (c['fn'] + c['fp'] + c['idsw']) / c['gt'] if c['gt'] else math.nan
    out['MOTP'] = c['iou_sum'] / c['tp'] if c['tp'] else math.nan
    return out


def evaluate(gt_json, result_rows, iou_threshold=DEFAULT_IOU_THRESHOLD):
    """gt_json: the ground-truth file's content (dict with 'annotations' [+ 'images'] or a bare list); result_rows: the
    tracking JSON's content.  Returns a dict:
        per_stream[(segment, camera)][category][level] -> counts + iou_sum          (level 1 or 2)
        table[category or 'ALL'][level]                 -> counts + iou_sum + MOTA + MOTP
        hyp_match / hyp_switch (one entry per result row, file order; match = index into the annotation list, -1, -2)
        ignored_rows, stream_keys."""
    n_classes = len(iou_threshold)
    annotations = gt_json['annotations'] if isinstance(gt_json, dict) else gt_json
    images = gt_json.get('images') if isinstance(gt_json, dict) else None
    frames = {}                                     # stream -> set of frame ids, streams in order of first appearance
    if images is not None:
        for im in images:
            key, fr = _split(im['id'])
            frames.setdefault(key, set()).add(fr)
    else:
        for a in annotations:
            key, fr = _split(a['image_id'])
            frames.setdefault(key, set()).add(fr)
    gt_rows = {}
    for idx, a in enumerate(annotations):
        key, fr = _split(a['image_id'])
        if key not in frames or fr not in frames[key]:
            continue
        if a['bbox'][2] < 1 or a['bbox'][3] < 1:
            continue
        gt_rows.setdefault((key, fr), []).append(
            (idx, xyxy(a['bbox']), a['category_id'], 2 if a.get('tracking_difficulty_level', 1) == 2 else 1, a['object_id']))
    hyp_rows = {}
    hyp_match = [-2] * len(result_rows)
    hyp_switch = [0] * len(result_rows)
    for idx, r in enumerate(result_rows):
        key, fr = _split(r['image_id'])
        if key not in frames or fr not in frames[key] or not (1 <= r['category_id'] <= n_classes):
            continue
        hyp_rows.setdefault((key, fr), []).append((idx, xyxy(r['bbox']), r['category_id'], r['object_id']))
    per_stream = {}
    for key in frames:
        per_stream[key] = {}
        for c in range(1, n_classes + 1):
            thr = iou_threshold[c - 1]
            cnt = {1: _zero(), 2: _zero()}
            prev = {}                               # object -> hypothesis id, matches of the previous frame
            last = {}                               # object -> hypothesis id it was last matched to
            for fr in sorted(frames[key]):
                G = [g for g in gt_rows.get((key, fr), []) if g[2] == c]
                H = [h for h in hyp_rows.get((key, fr), []) if h[2] == c]
                hids = [h[3] for h in H]
                assert len(set(hids)) == len(hids), 'duplicate hypothesis id in %s/%d/%s' % (key[0], fr, key[1])
                hpos = {hid: j for j, hid in enumerate(hids)}
                match = {}                          # ground-truth position -> hypothesis position
                taken = set()
                for i, g in enumerate(G):           # 1. carry over
                    hid = prev.get(g[4])
                    if hid is not None and hid in hpos:
                        j = hpos[hid]
                        if iou(g[1], H[j][1]) >= thr:
                            match[i] = j
                            taken.add(j)
                rest_g = [i for i in range(len(G)) if i not in match]
                rest_h = [j for j in range(len(H)) if j not in taken]
                M = gated_matrix([G[i][1] for i in rest_g], [H[j][1] for j in rest_h], thr)
                for a, b in assign(M):              # 2. assign the rest
                    match[rest_g[a]] = rest_h[b]
                    taken.add(rest_h[b])
                prev = {}
                for i, g in enumerate(G):           # 3. count
                    levels = (1, 2) if g[3] != 2 else (2,)
                    for lv in levels:
                        cnt[lv]['gt'] += 1
                    if i in match:
                        h = H[match[i]]
                        v = iou(g[1], h[1])
                        switch = g[4] in last and last[g[4]] != h[3]
                        for lv in levels:
                            cnt[lv]['tp'] += 1
                            cnt[lv]['iou_sum'] = cnt[lv]['iou_sum'] + v
                            cnt[lv]['idsw'] += int(switch)
                        last[g[4]] = h[3]
                        prev[g[4]] = h[3]
                        hyp_match[h[0]] = g[0]
                        hyp_switch[h[0]] = int(switch)
                    else:
                        for lv in levels:
                            cnt[lv]['fn'] += 1
                for j, h in enumerate(H):
                    if j not in taken:
                        cnt[1]['fp'] += 1
                        cnt[2]['fp'] += 1
                        hyp_match[h[0]] = -1
            per_stream[key][c] = cnt
    table = {}
    for c in list(range(1, n_classes + 1)) + ['ALL']:
        table[c] = {}
        for lv in (1, 2):
            tot = _zero()
            for cc in ([c] if c != 'ALL' else [x for x in ALL_CLASSES if x <= n_classes]):
                for key in frames:                  # the order of this sum is part of the definition: class, then stream
                    for f in FIELDS:
                        tot[f] += per_stream[key][cc][lv][f]
                    tot['iou_sum'] = tot['iou_sum'] + per_stream[key][cc][lv]['iou_sum']
            table[c][lv] = finish(tot)
    return {'per_stream': per_stream, 'table': table, 'hyp_match': hyp_match, 'hyp_switch': hyp_switch,
            'ignored_rows': sum(1 for m in hyp_match if m == -2), 'stream_keys': list(frames)}
