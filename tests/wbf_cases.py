"""Hand-worked cases of weighted boxes fusion / NMW in exact (dyadic) arithmetic, shared by tests/test_wbf_ref.py (the restatement)
and tests/test_gpu_wbf.py (the kernel).  Quotients that are not dyadic are written as the one correctly rounded division they are."""

# name -> (rows [score, x1, y1, x2, y2], wsum, method, iou_thresh, expected out [conf, x, y, w, h], members, row_cluster)
CASES = {
    # 0.25-box joins the 0.75-box (IoU 80 / 120): S = 1, B = (0.5, 0, 10.5, 10); conf = ((1 / 2) * min(2, 2)) / 2
    'fusion': ([[0.75, 0, 0, 10, 10], [0.25, 2, 0, 12, 10], [0.5, 40, 40, 50, 50]], 2, 'weighted_fusion', 0.5,
               [[0.5, 0.5, 0, 10, 10], [0.25, 40, 40, 10, 10]], [2, 1], [0, 0, 1]),
    # third box: IoU 1/3 with the first box, 7/13 with the fused box (2, 0, 12, 10): joins under weighted_fusion ...
    'drift_fusion': ([[0.5, 0, 0, 10, 10], [0.5, 4, 0, 14, 10], [0.25, 5, 0, 15, 10]], 1, 'weighted_fusion', 0.4,
                     [[1.25 / 3, 3.25 / 1.25, 0.0, 15.75 / 1.25 - 3.25 / 1.25, 12.5 / 1.25]], [3], [0, 0, 0]),
    # ... and not under nmw.  Cluster 1: wt = 0.5 * 1 and 0.5 * (3 / 7)
    'drift_nmw': ([[0.5, 0, 0, 10, 10], [0.5, 4, 0, 14, 10], [0.25, 5, 0, 15, 10]], 1, 'nmw', 0.4,
                  [[0.5, (0.5 * (3 / 7) * 4) / (0.5 + 0.5 * (3 / 7)), 0.0,
                    (5.0 + 0.5 * (3 / 7) * 14) / (0.5 + 0.5 * (3 / 7)) - (0.5 * (3 / 7) * 4) / (0.5 + 0.5 * (3 / 7)),
                    (5.0 + 0.5 * (3 / 7) * 10) / (0.5 + 0.5 * (3 / 7))],
                   [0.25, 5, 0, 10, 10]], [2, 1], [0, 0, 1]),
    # IoU = 2 / 4 is not > 0.5
    'iou_at_threshold': ([[0.5, 0, 0, 3, 1], [0.25, 1, 0, 4, 1]], 1, 'weighted_fusion', 0.5,
                         [[0.5, 0, 0, 3, 1], [0.25, 1, 0, 3, 1]], [1, 1], [0, 1]),
    'iou_at_threshold_nmw': ([[0.5, 0, 0, 3, 1], [0.25, 1, 0, 4, 1]], 1, 'nmw', 0.5,
                             [[0.5, 0, 0, 3, 1], [0.25, 1, 0, 3, 1]], [1, 1], [0, 1]),
    # the middle box has IoU 8 / 40 with both clusters: it joins the one created first, whichever row that is
    'equal_iou_first_cluster': ([[1.0, 0, 0, 4, 4], [0.5, 8, 0, 12, 4], [0.5, 2, 0, 10, 4]], 1, 'weighted_fusion', 0.125,
                                [[0.75, 1.0 / 1.5, 0, 9.0 / 1.5 - 1.0 / 1.5, 4], [0.5, 8, 0, 4, 4]], [2, 1], [0, 1, 0]),
    'equal_iou_first_cluster_swapped': ([[0.5, 0, 0, 4, 4], [1.0, 8, 0, 12, 4], [0.5, 2, 0, 10, 4]], 1, 'weighted_fusion', 0.125,
                                        [[0.75, 9.0 / 1.5, 0, 17.0 / 1.5 - 9.0 / 1.5, 4], [0.5, 0, 0, 4, 4]], [2, 1], [1, 0, 0]),
    # equal scores: visited in row order (the first row founds the cluster the second joins); equal conf: creation order
    'equal_scores_row_order': ([[0.5, 100, 0, 110, 10], [0.5, 0, 0, 8, 8], [0.5, 0, 0, 8, 8], [0.5, 50, 0, 60, 10]], 2, 'nmw', 0.5,
                               [[0.5, 100, 0, 10, 10], [0.5, 0, 0, 8, 8], [0.5, 50, 0, 10, 10]], [1, 2, 1], [0, 1, 1, 2]),
    # touching boxes: inter == 0 gives IoU 0.0, which is not > 0
    'touching': ([[0.5, 0, 0, 10, 10], [0.25, 10, 0, 20, 10], [0.125, 0, 10, 10, 20]], 1, 'weighted_fusion', 0.0,
                 [[0.5, 0, 0, 10, 10], [0.25, 10, 0, 10, 10], [0.125, 0, 10, 10, 10]], [1, 1, 1], [0, 1, 2]),
    # conf is capped by the members: one member of three inputs -> ((0.75 / 1) * min(4, 1)) / 4; two -> ((1 / 2) * 2) / 4
    'wsum_scales_conf': ([[0.75, 0, 0, 8, 8], [0.5, 20, 0, 28, 8], [0.5, 20, 0, 28, 8]], 4, 'weighted_fusion', 0.5,
                         [[0.25, 20, 0, 8, 8], [0.1875, 0, 0, 8, 8]], [2, 1], [1, 0, 0]),
}
