"""Plain-Python restatement of the two merge rules behind detnet/ensemble_b.py - weighted boxes fusion (`weighted_fusion`) and
non-maximum weighted (`nmw`) - as this project defines them.  It is the yardstick of csrc/ensemble_wbf.hip:
Python floats are IEEE float64, every line below is one rounded operation or a comparison, and the kernel performs the same
operations in the same order without contraction, so the two are compared with ==.

The definition is the published algorithm (Solovyev, Wang, Gabruseva: "Weighted boxes fusion") on the pixel corner boxes that
ensemble_b.py builds, with the order of equal scores and equal IoUs fixed.  It is NOT pinned against the ensemble_boxes package
(conf_type 'avg', no overflow allowance, no coordinate clipping).

    IoU(A, B):  inter = max(0, min(A.x2, B.x2) - max(A.x1, B.x1)) * max(0, min(A.y2, B.y2) - max(A.y1, B.y1))
                0.0 when inter == 0, else inter / ((area(A) + area(B)) - inter), area = (x2 - x1) * (y2 - y1)
    rows are visited by descending score, equal scores in row order
    weighted_fusion: a row joins the cluster whose FUSED box has the greatest IoU with it, if that IoU > iou_thresh (equal IoUs:
                the earlier cluster), else it starts a cluster whose fused box is the row's box.  A cluster keeps S = sum of scores
                and B[c] = sum of score * corner, member by member; on every join its fused box becomes B[c] / S.
                conf = ((S / n) * min(wsum, n)) / wsum
    nmw:        the same walk against each cluster's FIRST member.  Every member (the first included) weighs
                wt = score * IoU(first member, member); box = (sum of wt * corner) / (sum of wt); conf = the first member's score
    output:     clusters by descending conf, equal conf in creation order, as [conf, x1, y1, x2 - x1, y2 - y1]
"""
import numpy as np

METHODS = {'weighted_fusion': 0, 'nmw': 1}


def iou(a, b):
    iw = max(0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    if inter == 0:
        return 0.0
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[2] - b[0]) * (b[3] - b[1])
    return inter / ((area_a + area_b) - inter)


def fuse_xyxy(rows, wsum, method, iou_thresh):
    """One group.  rows: [[score, x1, y1, x2, y2], ...] (scores already weighted).  Returns (out, members, row_cluster):
    out = [[conf, x1, y1, w, h], ...] in output order, members[k] = rows in output row k, row_cluster[i] = output row of the
    cluster input row i joined."""
    rows = [[float(v) for v in r] for r in rows]
    wsum = float(wsum)
    iou_thresh = float(iou_thresh)
    nmw = {'weighted_fusion': False, 'nmw': True, 0: False, 1: True}[method]
    order = sorted(range(len(rows)), key=lambda i: -rows[i][0])          # stable: equal scores keep row order
    clusters = []                                                        # creation order
    joined = [None] * len(rows)
    for i in order:
        s, box = rows[i][0], rows[i][1:5]
        best, k = iou_thresh, None
        for c, cl in enumerate(clusters):
            v = iou(cl['match'], box)
            if v > best:                                                 # strict: the earlier of equal IoUs stays
                best, k = v, c
        if nmw:
            wt = s * (best if k is not None else iou(box, box))
        else:
            wt = s
        if k is None:
            clusters.append({'match': list(box), 'S': wt, 'B': [wt * box[c] for c in range(4)], 'n': 1, 'first': s})
            joined[i] = len(clusters) - 1
        else:
            cl = clusters[k]
            cl['S'] = cl['S'] + wt
            for c in range(4):
                cl['B'][c] = cl['B'][c] + wt * box[c]
            cl['n'] += 1
            if not nmw:
                cl['match'] = [cl['B'][c] / cl['S'] for c in range(4)]
            joined[i] = k
    confs, boxes = [], []
    for cl in clusters:
        if nmw:
            confs.append(cl['first'])
            boxes.append([cl['B'][c] / cl['S'] for c in range(4)])
        else:
            n = float(cl['n'])
            confs.append(((cl['S'] / n) * min(wsum, n)) / wsum)
            boxes.append(cl['match'])
    out_order = sorted(range(len(clusters)), key=lambda c: -confs[c])    # stable: creation order on equal conf
    position = {c: p for p, c in enumerate(out_order)}
    out = [[confs[c], boxes[c][0], boxes[c][1], boxes[c][2] - boxes[c][0], boxes[c][3] - boxes[c][1]] for c in out_order]
    return out, [clusters[c]['n'] for c in out_order], [position[c] for c in joined]


def fuse_xywh(rows, wsum, method, iou_thresh):
    """The same for rows [score, x, y, w, h]: corners are [x, y, x + w, y + h]."""
    return fuse_xyxy([[r[0], r[1], r[2], r[1] + r[3], r[2] + r[4]] for r in (list(map(float, q)) for q in rows)], wsum, method, iou_thresh)


def fuse_groups(dets5, group_offsets, group_wsum, method, iou_thresh):
    """The packed form wt_fuse_groups_* takes -> (out5, counts, members, row_cluster) in its output layout: group g writes
    counts[g] rows starting at row group_offsets[g]; unused rows stay 0."""
    dets5 = np.asarray(dets5, np.float64).reshape(-1, 5)
    off = [int(v) for v in group_offsets]
    out5 = np.zeros_like(dets5)
    members = np.zeros(len(dets5), np.int32)
    row_cluster = np.zeros(len(dets5), np.int32)
    counts = np.zeros(len(off) - 1, np.int64)
    for g in range(len(off) - 1):
        a, b = off[g], off[g + 1]
        if b == a:
            continue
        out, mem, rc = fuse_xywh(dets5[a:b].tolist(), float(group_wsum[g]), method, iou_thresh)
        counts[g] = len(out)
        out5[a:a + len(out)] = out
        members[a:a + len(out)] = mem
        row_cluster[a:b] = rc
    return out5, counts, members, row_cluster


def merge_fn(packed, method, iou_thresh):
    """Drop-in for ensemble_b.merge_groups (the `merge_fn=` of fuse_columns)."""
    return fuse_groups(packed['dets5'], packed['group_offsets'], packed['group_wsum'], method, iou_thresh)


def random_groups(seed, n_groups=200, max_objects=11, k_inputs=3, p_present=0.8, sigma=3.0):
    """Seeded ensemble-like groups: every object is seen by each of the k inputs with probability p_present, its corners jittered
    by sigma px, scores rounded to 5 decimals.  Rows input by input.  Returns (dets5 [score, x, y, w, h], group_offsets, wsum)."""
    rng = np.random.default_rng(seed)
    rows, offsets, wsum = [], [0], []
    for _ in range(n_groups):
        n_obj = int(rng.integers(0, max_objects + 1))
        x1 = rng.uniform(0, 1700, n_obj); y1 = rng.uniform(0, 1100, n_obj)
        w = rng.uniform(20, 220, n_obj); h = rng.uniform(20, 180, n_obj)
        base = rng.uniform(0.05, 1.0, n_obj)
        for o in range(1, n_obj):                                        # now and then two objects nearly coincide (a crowd): their
            if rng.random() < 0.15:                                      # rows can end up in one cluster of more than k members
                q = int(rng.integers(0, o))
                x1[o], y1[o], w[o], h[o] = x1[q] + rng.normal(0, 2), y1[q] + rng.normal(0, 2), w[q], h[q]
        seen = 0
        for k in range(k_inputs):
            present = rng.random(n_obj) < p_present
            seen += bool(present.any())
            for o in np.nonzero(present)[0]:
                c = np.array([x1[o], y1[o], x1[o] + w[o], y1[o] + h[o]]) + rng.normal(0, sigma, 4)
                score = round(float(np.clip(base[o] + rng.normal(0, 0.05), 0.001, 1.0)), 5)
                rows.append([score, c[0], c[1], max(c[2] - c[0], 1.0), max(c[3] - c[1], 1.0)])
        offsets.append(len(rows))
        wsum.append(float(max(seen, 1)))
    return np.asarray(rows, np.float64).reshape(-1, 5), np.asarray(offsets, np.int64), np.asarray(wsum, np.float64)


def ensemble_rows(submissions, method='weighted_fusion', iou_thresh=0.5, weights=None):
    """detnet/ensemble_b.py on parsed detection files (lists of {image_id, category_id, bbox [x, y, w, h], score}) -> the rows it
    writes.  Rows with w > 0 and h > 0 are kept; a group is one (image, category), its rows input by input in file order; wsum of
    an image = the weights (default 1) of the inputs that have a kept row of ANY category in it, added in input order; per image
    the merged rows of all categories by descending conf (equal conf: ascending category, then group order); images in order of
    first appearance; score = round(conf, 5), bbox = floats."""
    import math
    weights = [1.0] * len(submissions) if weights is None else [float(w) for w in weights]
    images = {}
    for k, sub in enumerate(submissions):
        for d in sub:
            x, y, w, h = (float(v) for v in d['bbox'])
            score = float(d['score'])
            if not all(math.isfinite(v) for v in (x, y, w, h, score)):
                raise ValueError('non-finite value in input %d' % k)
            if not (w > 0 and h > 0):
                continue
            im = images.setdefault(d['image_id'], {'inputs': [], 'groups': {}})
            if k not in im['inputs']:
                im['inputs'].append(k)
            im['groups'].setdefault(int(d['category_id']), []).append([score * weights[k], x, y, w, h])
    out = []
    for image_id, im in images.items():
        wsum = 0.0
        for k in sorted(im['inputs']):
            wsum = wsum + weights[k]
        rows = []
        for cat in sorted(im['groups']):
            merged, _, _ = fuse_xywh(im['groups'][cat], wsum, method, iou_thresh)
            rows += [(cat, r) for r in merged]
        rows.sort(key=lambda cr: -cr[1][0])                              # stable: category, then group order
        out += [{'image_id': image_id, 'category_id': cat, 'bbox': r[1:5], 'score': round(r[0], 5)} for cat, r in rows]
    return out
