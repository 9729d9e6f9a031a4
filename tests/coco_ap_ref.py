"""The COCO detection metric (bbox, useCats) restated in plain numpy / Python on one thread: the definition of DESIGN.md section 28
that csrc/det_coco_eval.hip is held equal to.  It is this project's own restatement of the published algorithm, pinned by the
hand-worked cases of tests/coco_cases.py; the pycocotools package is not a dependency (tools/check_coco_eval.py compares with it
where it is installed).  No cleverness: the matching is the sequential scan, the curve uses numpy's cumsum and searchsorted."""
import json

import numpy as np

THR = np.linspace(.5, .95, 10)
REC = np.linspace(0, 1, 101)
AREAS = np.asarray([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64)
MAX_DETS = np.asarray([1, 10, 100], np.int32)
EPS = 2.0 ** -52
STAT_NAMES = ('mAP', 'AP50', 'AP75', 'mAPs', 'mAPm', 'mAPl', 'AR1', 'AR10', 'AR', 'ARs', 'ARm', 'ARl')


# ---------------------------------------------------------------------------------------------------------------
# packing: rows in image order, inside an image in input order
def ground_truth(annotations):
    if not isinstance(annotations, dict):
        with open(annotations) as fp:
            annotations = json.load(fp)
    image_ids = sorted(im['id'] for im in annotations['images'])
    cat_ids = sorted(c['id'] for c in annotations['categories'])
    names = {c['id']: c.get('name', str(c['id'])) for c in annotations['categories']}
    index = {str(k): i for i, k in enumerate(image_ids)}
    per_image = [[] for _ in image_ids]
    for a in annotations['annotations']:
        x, y, w, h = (float(v) for v in a['bbox'])
        crowd = int(a.get('iscrowd', 0))
        per_image[index[str(a['image_id'])]].append((x, y, w, h, float(a['area']) if 'area' in a else w * h, cat_ids.index(a['category_id']), crowd))
    rows = [r for rows in per_image for r in rows]
    col = lambda j, dt: np.asarray([r[j] for r in rows], dt)
    offsets = np.zeros(len(image_ids) + 1, np.int64)
    offsets[1:] = np.cumsum([len(r) for r in per_image])
    return dict(image_ids=image_ids, index=index, cat_ids=cat_ids, names=[names[c] for c in cat_ids], x=col(0, np.float64), y=col(1, np.float64),
                w=col(2, np.float64), h=col(3, np.float64), area=col(4, np.float64), cat=col(5, np.int32), crowd=col(6, np.uint8),
                image_gt_offsets=offsets)


def result(gt, rows):
    """Wire rows [{image_id, category_id, bbox, score}] -> columns in image order (input order inside an image); rows of a
    category the ground truth does not define are left out; source_row = the row's index in the input."""
    kept = []
    has_rows = np.zeros(len(gt['image_ids']), bool)     # every row counts here, also one of a category that is not defined
    for i, r in enumerate(rows):
        if str(r['image_id']) not in gt['index']:
            raise ValueError('row %d is on image %s, which the ground truth does not list' % (i, r['image_id']))
        vals = [float(r['score'])] + [float(v) for v in r['bbox']]
        if not all(np.isfinite(vals)):
            raise ValueError('row %d: the score or a coordinate is not finite' % i)
        has_rows[gt['index'][str(r['image_id'])]] = True
        if r['category_id'] in gt['cat_ids']:
            kept.append((gt['index'][str(r['image_id'])], i, gt['cat_ids'].index(r['category_id']), vals))
    kept.sort(key=lambda t: t[0])                       # stable
    col = lambda j: np.asarray([t[3][j] for t in kept], np.float64)
    image = np.asarray([t[0] for t in kept], np.int64)
    return dict(image=image, source_row=np.asarray([t[1] for t in kept], np.int64), cat=np.asarray([t[2] for t in kept], np.int32),
                score=col(0), x=col(1), y=col(2), w=col(3), h=col(4), has_rows=has_rows,
                image_det_offsets=np.searchsorted(image, np.arange(len(gt['image_ids']) + 1)).astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------
def iou(d, g, crowd):
    """d, g = (x, y, w, h) floats."""
    xa = d[0] + d[2] if d[0] + d[2] < g[0] + g[2] else g[0] + g[2]
    xb = d[0] if d[0] > g[0] else g[0]
    ya = d[1] + d[3] if d[1] + d[3] < g[1] + g[3] else g[1] + g[3]
    yb = d[1] if d[1] > g[1] else g[1]
    iw, ih = xa - xb, ya - yb
    if iw <= 0:
        iw = 0.0
    if ih <= 0:
        ih = 0.0
    i = iw * ih
    u = d[2] * d[3] if crowd else (d[2] * d[3] + g[2] * g[3]) - i
    return 0.0 if i == 0 else i / u


def match_problem(D, G, thr, areas, witness):
    """D: [(x, y, w, h)] by descending score; G: [(x, y, w, h, area, crowd)] in annotation order.
    Returns match (A, T, |D|) index into G or -1, ign (A, T, |D|) bool, g_ign (A, |G|) bool."""
    A, T = len(areas), len(thr)
    ious = [[iou(d, g, g[5]) for g in G] for d in D]
    match = np.full((A, T, len(D)), -1, np.int64)
    ign = np.zeros((A, T, len(D)), bool)
    g_ign_all = np.zeros((A, len(G)), bool)
    for a, (lo, hi) in enumerate(areas):
        g_ign = [bool(g[5]) or g[4] < lo or g[4] > hi for g in G]
        g_ign_all[a] = g_ign
        order = [j for j in range(len(G)) if not g_ign[j]] + [j for j in range(len(G)) if g_ign[j]]
        for t, tv in enumerate(thr):
            taken = [False] * len(G)
            for di, d in enumerate(D):
                best = min(tv, 1 - 1e-10)
                m = None
                tie = False
                for j in order:
                    if taken[j] and not G[j][5]:
                        continue
                    if m is not None and not g_ign[m] and g_ign[j]:
                        break
                    if ious[di][j] < best:
                        continue
                    tie = m is not None and ious[di][j] == best
                    best, m = ious[di][j], j
                if m is not None:
                    match[a, t, di], ign[a, t, di] = m, g_ign[m]
                    taken[m] = True
                    witness['match'] += 1
                    witness['crowd_match'] += int(bool(G[m][5]))
                    witness['order_tie'] += int(tie)
                elif d[2] * d[3] < lo or d[2] * d[3] > hi:
                    ign[a, t, di] = True
                    witness['ignored_unmatched'] += 1
    return match, ign, g_ign_all


def evaluate(gt, sets, dt_images=False, thr=THR, rec=REC, areas=AREAS, max_dets=MAX_DETS, image_mask=None):
    """gt = ground_truth(...), sets = [result(...)].  Returns dict(precision (K, T, R, C, A, M), recall (K, T, C, A, M),
    npig (K, C, A), per set rank (n,), match_gt (n, A, T) (packed ground-truth row), ignore (n, A, T), witness (counts of the
    events the random cases must show))."""
    K, T, R, C, A, M = len(sets), len(thr), len(rec), len(gt['cat_ids']), len(areas), len(max_dets)
    n_images = len(gt['image_ids'])
    cap = int(max_dets[-1])
    precision = -np.ones((K, T, R, C, A, M))
    recall = -np.ones((K, T, C, A, M))
    npig = np.zeros((K, C, A), np.int64)
    witness = dict(match=0, crowd_match=0, ignored_unmatched=0, truncated=0, order_tie=0)
    ranks, matches, ignores = [], [], []
    go = gt['image_gt_offsets']
    for k, s in enumerate(sets):
        n = len(s['score'])
        rank = np.full(n, -1, np.int32)
        match_gt = np.full((n, A, T), -1, np.int64)
        ignore = np.zeros((n, A, T), np.uint8)
        do = s['image_det_offsets']
        if image_mask is not None:
            takes_part = [bool(v) for v in image_mask[k]]
        else:
            takes_part = [bool(s['has_rows'][i]) if dt_images else True for i in range(n_images)]
        for c in range(C):
            per_image = []                              # (rows of D in order, match (A, T, |D|), ign)
            for i in range(n_images):
                if not takes_part[i]:
                    continue
                g_rows = [j for j in range(go[i], go[i + 1]) if gt['cat'][j] == c]
                G = [(gt['x'][j], gt['y'][j], gt['w'][j], gt['h'][j], gt['area'][j], int(gt['crowd'][j])) for j in g_rows]
                d_rows = [j for j in range(do[i], do[i + 1]) if s['cat'][j] == c]
                d_rows = sorted(d_rows, key=lambda j: -s['score'][j])          # stable
                witness['truncated'] += int(len(d_rows) > cap)
                d_rows = d_rows[:cap]
                D = [(s['x'][j], s['y'][j], s['w'][j], s['h'][j]) for j in d_rows]
                m, ig, g_ign = match_problem(D, G, thr, areas, witness)
                for a in range(A):
                    npig[k, c, a] += int((~g_ign[a]).sum())
                for r, j in enumerate(d_rows):
                    rank[j] = r
                    match_gt[j] = np.where(m[:, :, r] >= 0, np.asarray(g_rows + [-1], np.int64)[m[:, :, r]], -1)
                    ignore[j] = ig[:, :, r]
                per_image.append((d_rows, m, ig))
            for a in range(A):
                for mi, md in enumerate(max_dets):
                    score = np.asarray([s['score'][j] for d_rows, _, _ in per_image for j in d_rows[:md]], np.float64)
                    order = np.argsort(-score, kind='mergesort')
                    for t in range(T):
                        if npig[k, c, a] == 0:
                            continue
                        matched = np.asarray([v for _, m, _ in per_image for v in m[a, t, :md] >= 0], bool)[order]
                        ign = np.asarray([v for _, _, ig in per_image for v in ig[a, t, :md]], bool)[order]
                        ctp = np.cumsum(matched & ~ign, dtype=np.float64)
                        cfp = np.cumsum(~matched & ~ign, dtype=np.float64)
                        rc = ctp / npig[k, c, a]
                        pr = ctp / (cfp + ctp + EPS)
                        recall[k, t, c, a, mi] = rc[-1] if len(rc) else 0.0
                        for i in range(len(pr) - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        at = np.searchsorted(rc, rec, side='left')
                        precision[k, t, :, c, a, mi] = [pr[j] if j < len(pr) else 0.0 for j in at]
        ranks.append(rank); matches.append(match_gt); ignores.append(ignore)
    return dict(precision=precision, recall=recall, npig=npig, rank=ranks, match_gt=matches, ignore=ignores, witness=witness)


_CASES = {}


def case_reference(name, build):
    """(gt, [result columns], evaluate(...)) of the case build() -> (annotations, [wire rows], dt_images); computed once per name
    and shared by the test files (nobody writes into it)."""
    if name not in _CASES:
        annotations, sets, dt_images = build()
        gt = ground_truth(annotations)
        packed = [result(gt, rows) for rows in sets]
        _CASES[name] = (annotations, sets, dt_images, gt, packed, evaluate(gt, packed, dt_images))
    return _CASES[name]


def call_from_packed(gt, p, mask=None, per_row=True):
    """evaluate() on columns packed by the product (detnet/evaluate.py: pack_coco_ground_truth, pack_coco_detections), in the shape of
    its HIP call: the hook of evaluate_coco_sets(call=...) and the expected value of the GPU tests."""
    sets = []
    for k in range(len(p['set_row_offsets']) - 1):
        lo, hi = int(p['set_row_offsets'][k]), int(p['set_row_offsets'][k + 1])
        s = {n: p[n][lo:hi] for n in ('score', 'x', 'y', 'w', 'h', 'cat')}
        s['image_det_offsets'] = p['image_det_offsets'][k]
        sets.append(s)
    out = evaluate(gt, sets, image_mask=mask)
    A, T = len(AREAS), len(THR)
    cat = lambda v, shape, dt: np.concatenate(v) if v else np.zeros(shape, dt)
    return dict(precision=out['precision'], recall=out['recall'], npig=out['npig'], rank=cat(out['rank'], 0, np.int32),
                match_gt=cat(out['match_gt'], (0, A, T), np.int64), ignore=cat(out['ignore'], (0, A, T), np.uint8), witness=out['witness'])


def summarize(precision, recall, thr=THR):
    """precision (T, R, C, A, M), recall (T, C, A, M) of one result -> the twelve numbers, in STAT_NAMES order."""
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    t50, t75 = int(np.argmin(np.abs(thr - .5))), int(np.argmin(np.abs(thr - .75)))
    M = precision.shape[-1] - 1
    return np.asarray([mean(precision[:, :, :, 0, M]), mean(precision[t50, :, :, 0, M]), mean(precision[t75, :, :, 0, M]),
                       mean(precision[:, :, :, 1, M]), mean(precision[:, :, :, 2, M]), mean(precision[:, :, :, 3, M]),
                       mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, 1]), mean(recall[:, :, 0, M]),
                       mean(recall[:, :, 1, M]), mean(recall[:, :, 2, M]), mean(recall[:, :, 3, M])])
