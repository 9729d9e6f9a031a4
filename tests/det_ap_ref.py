"""TEST INFRASTRUCTURE ONLY - plain numpy restatement of the detection metric of DESIGN.md section 16, WITH its tie rule.

Written from the definition: nothing is imported from waymo_2d_tracking_amd (detnet/data/metric.py, detnet/evaluate.py) or
csrc/det_eval.hip, which the tests compare against this file.  Rows are flat columns in image order, file order inside.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
BUCKETS = (('', None, None), ('S', None, 32 ** 2), ('M', 32 ** 2, 96 ** 2), ('L', 96 ** 2, None))
THRESHOLDS = {'waymo': lambda name: (0.7,) if name == 'vehicle' else (0.5,), 'voc': lambda name: (0.5, 0.75)}


def columns(image_ids, sizes, gt, detections, labels):
    """{image_id: (n, 5) [x1, y1, x2, y2, label]} and {image_id: [per class (n, 5) [conf, cx, cy, w, h]]} -> (gt, det) columns.
    labels[i] = ground-truth label of class array i (None: not evaluated).  Detections: image order, class by class, array order."""
    g = {k: [] for k in ('image', 'x1', 'y1', 'x2', 'y2', 'label')}
    d = {k: [] for k in ('image', 'label', 'conf', 'cx', 'cy', 'w', 'h')}
    for i, image_id in enumerate(image_ids):
        for row in np.asarray(gt[image_id], np.float64).reshape(-1, 5):
            for k, v in zip(('x1', 'y1', 'x2', 'y2'), row[:4]):
                g[k].append(v)
            g['image'].append(i); g['label'].append(int(row[4]))
        per_class = detections.get(image_id)
        if per_class is None:
            continue
        for ci, label in enumerate(labels):
            if label is None:
                continue
            for row in np.asarray(per_class[ci], np.float64).reshape(-1, 5):
                for k, v in zip(('conf', 'cx', 'cy', 'w', 'h'), row):
                    d[k].append(v)
                d['image'].append(i); d['label'].append(label)
    ints = ('image', 'label')
    g = {k: np.asarray(v, np.int64 if k in ints else np.float64) for k, v in g.items()}
    d = {k: np.asarray(v, np.int64 if k in ints else np.float64) for k, v in d.items()}
    g['image_area'] = np.asarray([float(sizes[k][0] * sizes[k][1]) for k in image_ids], np.float64)
    return g, d


def voc_ap(rec, prec):
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    step = [i for i in range(len(mrec) - 1) if mrec[i + 1] != mrec[i]]
    return float(np.sum([(mrec[i + 1] - mrec[i]) * mpre[i + 1] for i in step]))


def evaluate(g, d, n_classes, thr, min_conf=0.01):
    """thr: (n_classes, n_thr).  Returns dict: tp_flag (n, n_thr) uint8 (2 = took no part), match_gt (n), order {label: rows},
    curves {(label, t, bucket): ap, ar, T, tp, fp, ctp, cfp, rec, prec}."""
    thr = np.asarray(thr, np.float64).reshape(n_classes, -1)
    n, T = len(d['conf']), thr.shape[1]
    tp_flag = np.full((n, T), 2, np.uint8)
    match_gt = np.full(n, -1, np.int64)
    part = (d['label'] >= 1) & (d['label'] <= n_classes) & (d['conf'] > min_conf)
    g_size = (g['x2'] - g['x1']) * (g['y2'] - g['y1'])
    for key in np.unique(d['image'][part] * (n_classes + 1) + d['label'][part]):
        img, c = divmod(int(key), n_classes + 1)
        rows = np.nonzero(part & (d['image'] == img) & (d['label'] == c))[0]
        grows = np.nonzero((g['image'] == img) & (g['label'] == c))[0]
        tp_flag[rows] = 0
        if len(grows) == 0:
            continue
        claimed = [set() for _ in range(T)]
        for r in rows[np.argsort(-d['conf'][rows], kind='stable')]:      # descending, equal confidences in input order
            w, h = d['w'][r], d['h'][r]
            area = w * h
            x1, y1, x2, y2 = d['cx'][r] - w / 2, d['cy'][r] - h / 2, d['cx'][r] + w / 2, d['cy'][r] + h / 2
            iw = np.maximum(np.minimum(g['x2'][grows], x2) - np.maximum(g['x1'][grows], x1), 0.)
            ih = np.maximum(np.minimum(g['y2'][grows], y2) - np.maximum(g['y1'][grows], y1), 0.)
            inter = iw * ih
            with np.errstate(invalid='ignore', divide='ignore'):
                iou = inter / ((area + g_size[grows]) - inter)
            j = int(np.argmax(iou))                                      # the first maximum; a NaN counts as maximal
            match_gt[r] = grows[j]
            for t in range(T):
                if iou[j] > thr[c - 1, t] and j not in claimed[t]:
                    claimed[t].add(j)
                    tp_flag[r, t] = 1
    order, curves = {}, {}
    for c in range(1, n_classes + 1):
        rows = np.nonzero(part & (d['label'] == c))[0]
        rows = rows[np.argsort(-d['conf'][rows], kind='stable')]
        order[c] = rows
        det_size = d['w'][rows] * d['h'][rows] * g['image_area'][d['image'][rows]]
        gl = g['label'] == c
        pos_size = g_size[gl] * g['image_area'][g['image'][gl]]
        for t in range(T):
            for name, low, high in BUCKETS:
                m = np.ones(len(rows), bool)
                p = np.ones(len(pos_size), bool)
                if low is not None:
                    m &= det_size >= low; p &= pos_size >= low
                if high is not None:
                    m &= det_size < high; p &= pos_size < high
                npos = int(p.sum())
                flags = tp_flag[rows, t]
                ctp = np.cumsum((flags == 1) & m)[m] if name else np.cumsum(flags == 1)
                cfp = np.cumsum((flags == 0) & m)[m] if name else np.cumsum(flags == 0)
                rec = ctp / max(npos, EPS)
                prec = ctp / np.maximum(ctp + cfp, EPS)
                curves[(c, t, name)] = dict(ap=voc_ap(rec, prec), ar=float(rec[-1]) if len(rec) else float('nan'), T=npos,
                                            tp=int(ctp[-1]) if len(ctp) else 0, fp=int(cfp[-1]) if len(cfp) else 0,
                                            ctp=ctp.astype(np.int64), cfp=cfp.astype(np.int64), rec=rec, prec=prec)
    return dict(tp_flag=tp_flag, match_gt=match_gt, order=order, curves=curves)


def summary(res, classes, metric):
    """classes: [(name, label)] -> the nesting detnet/data/metric.py's evaluate_detections returns."""
    out = {}
    for name, c in classes:
        cv = res['curves']
        if metric == 'waymo':
            a = cv[(c, 0, '')]
            out[name] = dict(ap=a['ap'], ar=a['ar'], T=a['T'], score=a['ap'], by_size={b: cv[(c, 0, b)]['ap'] for b in 'SML'})
        else:
            s = {}
            for t, tv in enumerate((0.5, 0.75)):
                for b in (('S', 'M', 'L', '') if t == 0 else ('',)):
                    s['ap@%s%s' % (tv, b)] = cv[(c, t, b)]['ap']
                    s['ar@%s%s' % (tv, b)] = cv[(c, t, b)]['ar']
            s['T'] = cv[(c, 0, '')]['T']
            s['score'] = s['ap@0.5']
            out[name] = s
    if metric == 'voc':
        out['mean'] = {k: float(np.mean([out[name][k] for name, _ in classes])) for k in ('ap@0.5', 'ar@0.5', 'T')}
        out['score'] = out['mean']['ap@0.5']
    return out


CATEGORIES = [{'id': 1, 'name': 'vehicle'}, {'id': 2, 'name': 'pedestrian'}, {'id': 3, 'name': 'sign'}, {'id': 4, 'name': 'cyclist'}]


def synthetic(seed, n_images=200, width=1920, height=1280, n_objects=12, dropout=0.15, clutter=5, decimals=None, crowd=None):
    """A data set with clutter and dropouts: (COCO annotations dict, {image_id: [4 arrays (n, 5) float32 [conf, cx, cy, w, h]]}).
    Classes 1, 2, 4 have ground truth, class 3 only clutter; box sizes cover the S / M / L buckets; some confidences lie under 0.01.
    decimals: round the confidences (many ties).  crowd = (image index, boxes): that image gets so many vehicle boxes and detections."""
    rng = np.random.default_rng(seed)
    images, annotations, detections = [], [], {}
    for i in range(n_images):
        image_id = 'segment-%03d/%d/FRONT' % (i // 50, 1550000000000000 + i * 100000)
        images.append({'id': image_id, 'width': width, 'height': height, 'file_name': image_id + '.jpg'})
        n = int(rng.poisson(n_objects))
        cls = np.asarray([1, 2, 4])[rng.choice(3, size=n, p=[0.6, 0.3, 0.1])]
        if crowd is not None and i == crowd[0]:
            n = crowd[1]
            cls = np.ones(n, np.int64)
        w = np.exp(rng.uniform(np.log(8), np.log(400), n)); h = np.exp(rng.uniform(np.log(8), np.log(400), n))
        x = rng.uniform(0, width - w); y = rng.uniform(0, height - h)
        for j in range(n):
            annotations.append({'id': len(annotations), 'image_id': image_id, 'category_id': int(cls[j]),
                                'bbox': [float(x[j]), float(y[j]), float(w[j]), float(h[j])], 'area': float(w[j] * h[j])})
        seen = rng.uniform(size=n) >= dropout
        jit = lambda v, s: v + rng.normal(0, 1, v.shape) * s
        dw, dh = np.maximum(jit(w[seen], 0.06 * w[seen]), 2), np.maximum(jit(h[seen], 0.06 * h[seen]), 2)
        dcx, dcy = jit(x[seen] + w[seen] / 2, 0.05 * w[seen]), jit(y[seen] + h[seen] / 2, 0.05 * h[seen])
        dcls = cls[seen]
        conf = rng.uniform(0.3, 1.0, int(seen.sum()))
        m = int(rng.poisson(clutter))
        cw, ch = np.exp(rng.uniform(np.log(8), np.log(400), m)), np.exp(rng.uniform(np.log(8), np.log(400), m))
        dw, dh = np.concatenate([dw, cw]), np.concatenate([dh, ch])
        dcx = np.concatenate([dcx, rng.uniform(cw / 2, width - cw / 2)]); dcy = np.concatenate([dcy, rng.uniform(ch / 2, height - ch / 2)])
        dcls = np.concatenate([dcls, rng.integers(1, 5, m)])
        conf = np.concatenate([conf, rng.uniform(0.0, 1.0, m)])
        if decimals is not None:
            conf = np.round(conf, decimals)
        perm = rng.permutation(len(conf))
        rows = np.stack([conf, dcx / width, dcy / height, dw / width, dh / height], axis=1)[perm].astype(np.float32)
        detections[image_id] = [rows[dcls[perm] == c] for c in (1, 2, 3, 4)]
    return {'images': images, 'annotations': annotations, 'categories': CATEGORIES}, detections
