"""Inputs of the COCO metric tests: the hand-worked cases (their expected flags are written out in tests/test_coco_ap_ref.py), the
shapes at which the kernels change path, and the random sets.  Data only: a case is (annotations, [wire rows per result], dt_images)."""
import numpy as np

CATS2 = [{'id': 1, 'name': 'vehicle'}, {'id': 2, 'name': 'pedestrian'}]
CATS4 = CATS2 + [{'id': 3, 'name': 'sign'}, {'id': 4, 'name': 'cyclist'}]


def ann(images, boxes, cats=CATS2):
    """boxes: (image_id, category_id, [x, y, w, h]) or (..., extra fields)."""
    out = []
    for j, b in enumerate(boxes):
        a = {'id': j + 1, 'image_id': b[0], 'category_id': b[1], 'bbox': list(b[2])}
        a.update(b[3] if len(b) > 3 else {})
        out.append(a)
    return {'images': [{'id': k, 'width': 1920, 'height': 1280} for k in images], 'categories': cats, 'annotations': out}


def det(image, cat, bbox, score):
    return {'image_id': image, 'category_id': cat, 'bbox': list(bbox), 'score': score}


def hand_cases():
    c = {}
    # (a) two identical ground-truth boxes: the first detection takes the LATER one, the second detection the earlier one
    c['a_equal_iou_takes_the_later'] = (ann(['i'], [('i', 1, [0, 0, 10, 10]), ('i', 1, [0, 0, 10, 10])]),
                                        [[det('i', 1, [0, 0, 10, 10], .9), det('i', 1, [0, 0, 10, 10], .8)]], False)
    # (b) crowd box identical to the detection (IoU 1) listed first, a plain box with IoU 160 / 240 = 2 / 3 second
    c['b_not_ignored_before_ignored'] = (ann(['i'], [('i', 1, [10, 0, 20, 10], {'iscrowd': 1}), ('i', 1, [14, 0, 20, 10])]),
                                         [[det('i', 1, [10, 0, 20, 10], .9)]], False)
    # (c) a crowd box absorbs three detections inside it and, at t = 0.5 only, one that is half inside (200 / 400); box 1 is a plain match
    c['c_crowd_absorbs'] = (ann(['i'], [('i', 1, [0, 0, 100, 100], {'iscrowd': 1}), ('i', 1, [200, 200, 50, 50])]),
                            [[det('i', 1, [10, 10, 20, 20], .9), det('i', 1, [40, 40, 20, 20], .8), det('i', 1, [70, 70, 20, 20], .7),
                              det('i', 1, [90, 0, 20, 20], .6), det('i', 1, [200, 200, 50, 50], .5)]], False)
    # (d) IoU exactly 0.5 (100 / 200), exactly 0.75 (300 / 400), and identical boxes at t = 0.95; one image each
    c['d_iou_equal_to_the_threshold'] = (ann(['p', 'q', 'r'], [('p', 1, [0, 0, 10, 20]), ('q', 1, [0, 0, 40, 10]), ('r', 1, [5, 5, 7, 9])]),
                                         [[det('p', 1, [0, 0, 10, 10], .9), det('q', 1, [0, 0, 30, 10], .8), det('r', 1, [5, 5, 7, 9], .7)]], False)
    # (e) areas of exactly 32^2 and 96^2: each counts in both neighbouring ranges; the third box gives its area as a field
    c['e_area_bounds_are_inclusive'] = (ann(['i'], [('i', 1, [0, 0, 32, 32]), ('i', 1, [100, 100, 96, 96]), ('i', 1, [300, 300, 10, 10], {'area': 9216.0})]), [[]], False)
    # (f) a 30 x 30 detection on a 40 x 40 box: IoU 900 / 1600 = 0.5625
    c['f_unmatched_outside_the_range'] = (ann(['i'], [('i', 1, [0, 0, 40, 40])]), [[det('i', 1, [0, 0, 30, 30], .9)]], False)
    # (g) 101 detections with one score on one box
    c['g_101_equal_scores'] = (ann(['i'], [('i', 1, [0, 0, 50, 50])]), [[det('i', 1, [0, 0, 50, 50 + j], .5) for j in range(101)]], False)
    # (h) category 2 has only a crowd box: -1, out of the means
    c['h_category_without_ground_truth'] = (ann(['i'], [('i', 1, [0, 0, 50, 50]), ('i', 2, [100, 100, 50, 50], {'iscrowd': 1})]),
                                            [[det('i', 1, [0, 0, 50, 50], .9), det('i', 2, [100, 100, 50, 50], .8), det('i', 2, [300, 300, 50, 50], .7)]], False)
    # (i) image 'a' has a false positive, image 'b' a true positive, both with score 0.8; the file lists 'b' first
    c['i_score_tie_across_images'] = (ann(['b', 'a'], [('b', 1, [0, 0, 50, 50])]), [[det('b', 1, [0, 0, 50, 50], .8), det('a', 1, [0, 0, 50, 50], .8)]], False)
    # (j) TP, FP, TP, FP, TP on three boxes
    boxes = [[0, 0, 50, 50], [100, 0, 50, 50], [200, 0, 50, 50]]
    c['j_three_step_curve'] = (ann(['i'], [('i', 1, b) for b in boxes]),
                               [[det('i', 1, boxes[0], .9), det('i', 1, [500, 500, 50, 50], .8), det('i', 1, boxes[1], .7), det('i', 1, [600, 500, 50, 50], .6),
                                 det('i', 1, boxes[2], .5)]], False)
    # (k) two images with one box each, detections on the first only: with and without --dt-images
    two = ann(['a', 'b'], [('a', 1, [0, 0, 50, 50]), ('b', 1, [0, 0, 50, 50])])
    c['k_all_images'] = (two, [[det('a', 1, [0, 0, 50, 50], .9)]], False)
    c['k_dt_images'] = (two, [[det('a', 1, [0, 0, 50, 50], .9)]], True)
    return c


def shapes_case():
    """Problems with 0 / 1 / 63 / 64 / 65 / 130 / 300 ground-truth boxes and 0 / 1 / 99 / 100 / 101 / 165 detections of one category, and one image
    of 280 boxes shared by two categories.  The boxes sit on a grid; detections are shifted copies, several per box, with few different scores."""
    plan = [('s0', 0, 165), ('s1', 1, 101), ('s2', 63, 100), ('s3', 64, 99), ('s4', 65, 1), ('s5', 130, 0), ('s6', 130, 165), ('s7', 300, 40), ('s8', 0, 0)]
    rng = np.random.default_rng(7)
    boxes, rows = [], []
    for name, n_gt, n_det in plan:
        cell = lambda j: j - 1 if j % 13 == 3 else j                          # every 13th box repeats its neighbour: ties decided by order
        grid = [[40.0 * (cell(j) % 20), 40.0 * (cell(j) // 20), 30.0, 30.0] for j in range(max(n_gt, 1))]
        for j in range(n_gt):
            boxes.append((name, 1, grid[j], {'iscrowd': 1} if j % 17 == 5 else {}))
        for j in range(n_det):
            g = grid[int(rng.integers(0, min(len(grid), 12)))]
            dx, dy = (float(v) for v in rng.integers(0, 4, 2))
            rows.append(det(name, 1, [g[0] + dx, g[1] + dy, g[2], g[3]], float(rng.integers(1, 10)) / 10))
    # an image with more rows than the kernel keeps in LDS whose boxes alternate between the two categories: their waves share the image's rows
    for j in range(280):
        boxes.append(('s9', 1 + j % 2, [40.0 * (j % 20), 40.0 * (j // 20), 30.0, 30.0]))
    for j in range(160):
        g = int(rng.integers(0, 12))
        dx, dy = (float(v) for v in rng.integers(0, 4, 2))
        rows.append(det('s9', 1 + g % 2, [40.0 * g + dx, dy, 30.0, 30.0], float(rng.integers(1, 10)) / 10))
    order = rng.permutation(len(rows))
    return ann([p[0] for p in plan] + ['s9'], boxes), [[rows[i] for i in order]], False


def many_categories_case():
    """300 categories, three of them used: more (category, area range) counters than the npig kernel keeps in LDS, and a wide segment key."""
    cats = [{'id': i, 'name': 'c%d' % i} for i in range(1, 301)]
    boxes = [('a', 1, [0, 0, 50, 50]), ('a', 150, [100, 0, 50, 50]), ('b', 300, [0, 0, 120, 120]), ('b', 300, [200, 0, 20, 20], {'iscrowd': 1}), ('b', 150, [300, 300, 40, 40])]
    rows = [det('a', 1, [0, 0, 50, 50], .9), det('a', 150, [104, 0, 50, 50], .8), det('b', 300, [0, 0, 120, 110], .7), det('b', 300, [200, 0, 20, 20], .6),
            det('b', 299, [0, 0, 120, 120], .5), det('a', 150, [300, 300, 40, 40], .4)]
    return ann(['a', 'b'], boxes, cats), [rows, rows[::-1]], False


def random_case(seed, k_sets, n_images=40):
    """At most 40 images x 4 categories: crowd boxes, duplicated boxes, scores of one decimal, a problem with more than 100 detections, rows of a
    category the ground truth does not define, images without rows."""
    rng = np.random.default_rng(seed)
    images = ['img%03d' % i for i in range(n_images)]
    boxes = []
    for k in images:
        for _ in range(int(rng.integers(0, 10))):
            w, h = (float(v) for v in rng.integers(8, 200, 2))
            b = [float(rng.integers(0, 1700)), float(rng.integers(0, 1000)), w, h]
            extra = {}
            if rng.random() < .1:
                extra['iscrowd'] = 1
            if rng.random() < .5:
                extra['area'] = float(int(w * h * .75))
            boxes.append((k, int(rng.integers(1, 5)), b, extra))
            if rng.random() < .2:
                boxes.append((k, boxes[-1][1], list(b)))                    # a duplicated box
    rng.shuffle(boxes)
    sets = []
    for s in range(k_sets):
        rows = []
        for k, c, b, *_ in boxes:
            for _ in range(int(rng.integers(0, 3))):
                jitter = [0, 0, 0, 0] if rng.random() < .4 else [float(v) for v in rng.integers(-6, 7, 4)]
                rows.append(det(k, c if rng.random() < .9 else int(rng.integers(1, 5)), [b[0] + jitter[0], b[1] + jitter[1], max(1.0, b[2] + jitter[2]),
                                                                                      max(1.0, b[3] + jitter[3])], float(rng.integers(1, 10)) / 10))
        for _ in range(n_images):
            rows.append(det(images[int(rng.integers(0, n_images - 2))], int(rng.integers(1, 6)),             # category 5 is not defined
                            [float(rng.integers(0, 1700)), float(rng.integers(0, 1000)), float(rng.integers(8, 300)), float(rng.integers(8, 300))],
                            float(rng.integers(1, 100)) / 100))
        for j in range(120):                                                                                   # a problem that is cut at 100
            rows.append(det(images[s], 1, [10.0 * (j % 12), 10.0 * (j // 12), 50.0, 50.0], float(rng.integers(1, 4)) / 4))
        rows = [rows[i] for i in rng.permutation(len(rows))]
        sets.append(rows)
    return ann(images, boxes, CATS4), sets, False
