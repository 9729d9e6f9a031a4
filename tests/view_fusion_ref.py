"""Host composition of the ensemble_b file route for K views' wire slots (helpers of tests/test_view_fusion_ref.py and
tests/test_gpu_view_fusion.py), the yardstick of wt_fuse_slots_dev.

Every view's slots are read as the columns of one exported detection file (view_ensemble_ref.slots_as_submission: one image per
frame, rows in slot order), the pipeline's input filter drops the rows outside 1..n_categories and those with
score * weight < min_score, then the steps of `python -m waymo_2d_tracking_amd.detnet.ensemble_b` follow: ensemble_b.merge_inputs
(w > 0, h > 0, weighted scores, the image's weight sum) -> ensemble_b.pack_groups -> the plain-Python merge of tests/wbf_ref.py ->
conf > min_score, float boxes, numpy's round(conf, 5).  The result is laid out like the kernel's output: per frame K * S slots,
groups in ascending category order, inside a group wbf_ref's output order, then empty slots."""
import numpy as np

import wbf_ref
from view_ensemble_ref import slots_as_submission
from waymo_2d_tracking_amd.detnet import ensemble_b as EB

REF_METHOD = {'weighted_fusion_b': 'weighted_fusion', 'weighted_fusion': 'weighted_fusion', 'nmw': 'nmw'}


def host_fuse_slots(xywhs, category, n_frames, slots, weights, n_categories, method, iou_thresh, min_score):
    """xywhs (K, 5, F * S), category (K, F * S) -> (out_xywhs (5, F * K * S), out_category (F * K * S), counts (F))."""
    K = len(weights)
    subs = []
    for k in range(K):
        s = slots_as_submission(xywhs[k], category[k], n_frames, slots)
        keep = (s['category'] >= 1) & (s['category'] <= n_categories) & (s['score'] * float(weights[k]) >= min_score)
        subs.append({c: (v if c == 'image_ids' else v[keep]) for c, v in s.items()})
    out_x = np.zeros((5, n_frames * K * slots))
    out_c = np.zeros(n_frames * K * slots, np.int32)
    counts = np.zeros(n_frames, np.int64)
    image_ids, category_ids, rows, wsum = EB.merge_inputs(subs, weights)
    if not image_ids:
        return out_x, out_c, counts
    packed = EB.pack_groups(len(image_ids), category_ids, rows, K, wsum)
    out5, cnt = wbf_ref.fuse_groups(packed['dets5'], packed['group_offsets'], packed['group_wsum'], REF_METHOD[method], iou_thresh)[:2]
    ncat = packed['ncat']
    for g in range(packed['n_groups']):
        frame = int(image_ids[g // ncat])
        o = int(packed['group_offsets'][g])
        r = out5[o:o + int(cnt[g])]
        r = r[r[:, 0] > min_score]
        a = frame * K * slots + int(counts[frame])
        out_x[0:4, a:a + len(r)] = r[:, 1:5].T
        out_x[4, a:a + len(r)] = np.round(r[:, 0], 5)
        out_c[a:a + len(r)] = category_ids[g % ncat]
        counts[frame] += len(r)
    return out_x, out_c, counts


def case_as_slots(rows, wsum):
    """One hand-worked case of tests/wbf_cases.py (rows [score, x1, y1, x2, y2], integer wsum) as one frame of K = wsum views of
    weight 1, S = len(rows) + 1 slots, 2 categories: the rows are category 1 and go to the views in row order (row i to view
    min(i, K - 1), so the group's rows keep their order); a view left without a row gets one category-2 row, which makes it count
    for wsum.  Returns (xywhs (K, 5, S), category (K, S), weights)."""
    K, S = int(wsum), len(rows) + 1
    xywhs, cat = np.zeros((K, 5, S)), np.zeros((K, S), np.int32)
    used = [0] * K
    for i, (s, x1, y1, x2, y2) in enumerate(rows):
        k = min(i, K - 1)
        xywhs[k, :, used[k]] = [x1, y1, x2 - x1, y2 - y1, s]
        cat[k, used[k]] = 1
        used[k] += 1
    for k in range(K):
        if not used[k]:
            xywhs[k, :, 0] = [1000.0, 1000.0, 8.0, 8.0, 0.5]
            cat[k, 0] = 2
    return xywhs, cat, [1.0] * K


# The wsum case, worked by hand.  Three views, weights 1, 0.5, 0.25, min_score 0.01, 2 categories, 2 frames of 4 slots.
# Frame 0: every view has one far-apart category-1 row: wsum = (1 + 0.5) + 0.25 = 1.75, three single-member clusters,
#          conf = ((s * w / 1) * min(1.75, 1)) / 1.75 under weighted_fusion and s * w under nmw.
# Frame 1: view 0 has A (0.75) and B twice (0.75, 0.375), all category 1; view 1's only row is category 2 (0.5 * 0.5 = 0.25);
#          view 2's only row (category 1, 0.03 * 0.25 = 0.0075 < 0.01) is not kept.  wsum = 1 + 0.5 = 1.5: not K = 3, not the 1.75 of
#          all weights, not the 1 of the category-1 group's own view.  weighted_fusion: B has S = 1.125, n = 2:
#          ((1.125 / 2) * min(1.5, 2)) / 1.5 = 0.5625; A: ((0.75 / 1) * 1) / 1.5 = 0.5; category 2: (0.25 * 1) / 1.5 -> 0.16667.
#          nmw: conf = the first member's score: A 0.75 (created first), B 0.75, category 2 0.25.
WSUM_WEIGHTS = [1.0, 0.5, 0.25]
WSUM_MIN_SCORE = 0.01


def wsum_case():
    """-> (xywhs (3, 5, 8), category (3, 8), n_frames 2, slots 4, n_categories 2, expected {method: (out_x, out_c, counts)})."""
    F, S, K = 2, 4, 3
    xywhs, cat = np.zeros((K, 5, F * S)), np.zeros((K, F * S), np.int32)

    def put(k, slot, box, score, c):
        xywhs[k, :, slot] = list(box) + [score]
        cat[k, slot] = c
    put(0, 1, (0, 0, 10, 10), 0.5, 1)
    put(1, 0, (100, 0, 10, 10), 0.5, 1)
    put(2, 3, (200, 0, 10, 10), 0.5, 1)
    A, B = (0, 0, 16, 16), (300, 40, 8, 24)
    put(0, 4, A, 0.75, 1)
    put(0, 5, B, 0.75, 1)
    put(0, 7, B, 0.375, 1)
    put(1, 6, (500, 500, 20, 20), 0.5, 2)
    put(2, 4, B, 0.03, 1)
    expected = {}
    for method in ('weighted_fusion_b', 'nmw'):
        out_x, out_c, counts = np.zeros((5, F * K * S)), np.zeros(F * K * S, np.int32), np.asarray([3, 3], np.int64)
        if method == 'nmw':
            f0 = [((0, 0, 10, 10), 0.5), ((100, 0, 10, 10), 0.25), ((200, 0, 10, 10), 0.125)]
            f1 = [(A, 0.75, 1), (B, 0.75, 1), ((500, 500, 20, 20), 0.25, 2)]
        else:
            f0 = [((0, 0, 10, 10), round(np.float64(0.5 / 1.75), 5)), ((100, 0, 10, 10), round(np.float64(0.25 / 1.75), 5)),
                  ((200, 0, 10, 10), round(np.float64(0.125 / 1.75), 5))]
            f1 = [(B, 0.5625, 1), (A, 0.5, 1), ((500, 500, 20, 20), 0.16667, 2)]
        for j, (box, score) in enumerate(f0):
            out_x[:, j] = list(box) + [score]
            out_c[j] = 1
        for j, (box, score, c) in enumerate(f1):
            out_x[:, K * S + j] = list(box) + [score]
            out_c[K * S + j] = c
        expected[method] = (out_x, out_c, counts)
    return xywhs, cat, F, S, 2, expected
