"""TEST INFRASTRUCTURE ONLY - plain Python restatement of the HOTA metric.

HOTA / DetA / AssA / LocA (Luiten et al., IJCV 2021) per (stream, class) and Waymo difficulty level with dicts and lists:
nothing is shared with waymo_2d_tracking_amd/tracking/evaluate.py or csrc/mot_hota.hip, which the GPU tests compare against this
file.  The assignment is ``oracle.thirdparty_restated.linear_assignment`` on the negated float32 matrix, as tests/mot_ref.py uses
it.  Every order of operations below is part of the definition.
"""
import math

import numpy as np

from oracle.thirdparty_restated import linear_assignment

DEFAULT_IOU_THRESHOLD = (0.7, 0.5, 0.5, 0.5)
ALL_CLASSES = (1, 2, 4)
ALPHAS = [(a + 1) / 20.0 for a in range(19)]
NAMES = ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA')


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


def _split(image_id):
    segment, frame, camera = image_id.split('/')
    return (segment, camera), int(frame)


def level_rows(G, H, level, thr):
    """One frame and class.  G: [(box, level, id, tag)], H: [(box, id, tag)] in file order -> the rows of `level`."""
    if level == 2:
        return G, H
    keep = []
    for h in H:
        counted = dont_care = False
        for g in G:
            if iou(g[0], h[0]) >= thr:
                if g[1] != 2:
                    counted = True
                else:
                    dont_care = True
        if not (dont_care and not counted):
            keep.append(h)
    return [g for g in G if g[1] != 2], keep


def score_problem(frames):
    """frames: [(G, H)] of one (stream, class, level) in frame order, rows already filtered.
    Returns gt, hyp, tp[19], ass[19], assre[19], asspr[19], loc[19], terms[19], matches (list of (g tag, h tag))."""
    cg, ch = {}, {}
    P = {}
    scores = []
    for G, H in frames:
        for g in G:
            cg[g[2]] = cg.get(g[2], 0) + 1
        for h in H:
            ch[h[1]] = ch.get(h[1], 0) + 1
        S = [[iou(g[0], h[0]) for h in H] for g in G]
        scores.append(S)
        row = []
        for i in range(len(G)):
            t = 0.
            for j in range(len(H)):
                t = t + S[i][j]
            row.append(t)
        col = []
        for j in range(len(H)):
            t = 0.
            for i in range(len(G)):
                t = t + S[i][j]
            col.append(t)
        for i, g in enumerate(G):
            for j, h in enumerate(H):
                if S[i][j] > 0.:
                    key = (g[2], h[1])
                    P[key] = P.get(key, 0.) + S[i][j] / ((row[i] + col[j]) - S[i][j])
    A = dict((key, v / (float(cg[key[0]] + ch[key[1]]) - v)) for key, v in P.items())
    tp = [0] * 19
    loc = [0.] * 19
    cnt = [dict() for _ in range(19)]
    matches = []
    for (G, H), S in zip(frames, scores):
        if not G or not H:
            continue
        M = np.zeros((len(G), len(H)), dtype=np.float32)
        for i, g in enumerate(G):
            for j, h in enumerate(H):
                M[i, j] = np.float32(A.get((g[2], h[1]), 0.) * S[i][j])
        if not M.any():
            continue
        for i, j in linear_assignment(-M):              # sorted by ground-truth row
            i, j = int(i), int(j)
            if not M[i, j] > 0:
                continue
            matches.append((G[i][3], H[j][2]))
            key = (G[i][2], H[j][1])
            for a in range(19):
                if S[i][j] >= ALPHAS[a]:
                    tp[a] += 1
                    loc[a] = loc[a] + S[i][j]
                    cnt[a][key] = cnt[a].get(key, 0) + 1
    ass, assre, asspr, terms = [0.] * 19, [0.] * 19, [0.] * 19, [0] * 19
    for a in range(19):
        for (o, t), c in cnt[a].items():
            c = float(c)
            ass[a] = ass[a] + c * (c / (float(cg[o] + ch[t]) - c))
            assre[a] = assre[a] + c * (c / float(cg[o]))
            asspr[a] = asspr[a] + c * (c / float(ch[t]))
            terms[a] += 1
    return {'gt': sum(len(G) for G, _ in frames), 'hyp': sum(len(H) for _, H in frames), 'tp': tp, 'ass': ass, 'assre': assre,
            'asspr': asspr, 'loc': loc, 'terms': terms, 'matches': matches}


def _div(a, b):
    return a / b if b else math.nan


def finish(gt, hyp, tp, ass, assre, asspr, loc):
    """Added counts and sums -> the per-threshold arrays and the averaged row."""
    per = dict((n, []) for n in NAMES)
    for a in range(19):
        t = tp[a]
        per['DetA'].append(_div(t, gt + hyp - t))
        per['DetRe'].append(_div(t, gt))
        per['DetPr'].append(_div(t, hyp))
        per['AssA'].append(ass[a] / t if t else 0.)
        per['AssRe'].append(assre[a] / t if t else 0.)
        per['AssPr'].append(asspr[a] / t if t else 0.)
        per['LocA'].append(_div(loc[a], t))
        per['HOTA'].append(math.sqrt(per['DetA'][a] * per['AssA'][a]) if per['DetA'][a] == per['DetA'][a] else math.nan)
    row = {'gt': gt, 'hyp': hyp, 'tp': list(tp)}
    for n in NAMES:
        vals = per[n] if n != 'LocA' else [v for v, t in zip(per[n], tp) if t > 0]
        tot = 0.
        for v in vals:
            tot = tot + v
        row[n] = tot / len(vals) if vals else math.nan
    row['HOTA(0)'] = per['HOTA'][0]
    row['LocA(0)'] = per['LocA'][0]
    row['per_alpha'] = per
    return row


def evaluate(gt_json, result_rows, iou_threshold=DEFAULT_IOU_THRESHOLD):
    """gt_json: the ground-truth file's content (dict with 'annotations' [+ 'images'] or a bare list); result_rows: the
    tracking JSON's content.  Returns a dict:
        per_stream[(segment, camera)][category][level] -> score_problem() output
        table[category or 'ALL'][level]                 -> finish() output
        ignored_rows, stream_keys, matches[level] = {result row index: annotation index}, part = result rows that took part, removed[1] = result rows left out of LEVEL_1."""
    n_classes = len(iou_threshold)
    annotations = gt_json['annotations'] if isinstance(gt_json, dict) else gt_json
    images = gt_json.get('images') if isinstance(gt_json, dict) else None
    frames = {}
    for item in (images if images is not None else annotations):
        key, fr = _split(item['id'] if images is not None else item['image_id'])
        frames.setdefault(key, set()).add(fr)
    gt_rows, hyp_rows = {}, {}
    for n, a in enumerate(annotations):
        key, fr = _split(a['image_id'])
        if key not in frames or fr not in frames[key]:
            continue
        if a['bbox'][2] < 1 or a['bbox'][3] < 1:
            continue
        gt_rows.setdefault((key, fr), []).append(
            (xyxy(a['bbox']), 2 if a.get('tracking_difficulty_level', 1) == 2 else 1, a['object_id'], n, a['category_id']))
    ignored = 0
    part = set()
    for n, r in enumerate(result_rows):
        key, fr = _split(r['image_id'])
        if key not in frames or fr not in frames[key] or not (1 <= r['category_id'] <= n_classes):
            ignored += 1
            continue
        part.add(n)
        hyp_rows.setdefault((key, fr), []).append((xyxy(r['bbox']), r['object_id'], n, r['category_id']))
    per_stream = {}
    matches = {1: {}, 2: {}}
    kept = {1: set(), 2: set()}
    for key in frames:
        per_stream[key] = {}
        for c in range(1, n_classes + 1):
            per_stream[key][c] = {}
            for lv in (1, 2):
                fl = []
                for fr in sorted(frames[key]):
                    G = [g[:4] for g in gt_rows.get((key, fr), []) if g[4] == c]
                    H = [h[:3] for h in hyp_rows.get((key, fr), []) if h[3] == c]
                    assert len(set(h[1] for h in H)) == len(H) and len(set(g[2] for g in G)) == len(G), (key, fr)
                    G, H = level_rows(G, H, lv, iou_threshold[c - 1])
                    kept[lv].update(h[2] for h in H)
                    fl.append((G, H))
                res = score_problem(fl)
                for g_tag, h_tag in res['matches']:
                    matches[lv][h_tag] = g_tag
                per_stream[key][c][lv] = res
    table = {}
    for c in list(range(1, n_classes + 1)) + ['ALL']:
        table[c] = {}
        for lv in (1, 2):
            gt = hyp = 0
            tp = [0] * 19
            sums = dict((n, [0.] * 19) for n in ('ass', 'assre', 'asspr', 'loc'))
            for cc in ([c] if c != 'ALL' else [x for x in ALL_CLASSES if x <= n_classes]):         # class by class, stream by stream
                for key in frames:
                    r = per_stream[key][cc][lv]
                    gt += r['gt']
                    hyp += r['hyp']
                    for a in range(19):
                        tp[a] += r['tp'][a]
                        for n in sums:
                            sums[n][a] = sums[n][a] + r[n][a]
            table[c][lv] = finish(gt, hyp, tp, sums['ass'], sums['assre'], sums['asspr'], sums['loc'])
            table[c][lv]['sums'] = sums
    return {'per_stream': per_stream, 'table': table, 'ignored_rows': ignored, 'stream_keys': list(frames), 'matches': matches,
            'part': part, 'removed': {1: part - kept[1], 2: part - kept[2]}}
