"""tests/coco_ap_ref.py, the plain restatement of the COCO metric, pinned by cases small enough to check on paper.  pycocotools is not
installed where these run: the expected flags below are worked out by hand from the definition of DESIGN.md section 28."""
import numpy as np
import pytest

import coco_ap_ref as R
import coco_cases as CC

E = 2.0 ** -52
ALL, SMALL, MEDIUM, LARGE = range(4)


def ref(name):
    return R.case_reference(name, lambda: CC.hand_cases()[name])[5]


def test_constants():
    assert R.THR[0] == 0.5 and R.THR[5] == 0.75 and R.THR[9] == 0.95 and len(R.THR) == 10
    assert R.THR[3] < 2 / 3 < R.THR[4] and R.THR[1] < 0.5625 < R.THR[2]
    assert R.REC[0] == 0 and R.REC[100] == 1 and len(R.REC) == 101 and R.REC[33] <= 1 / 3 < R.REC[34] and R.REC[66] <= 2 / 3 < R.REC[67]
    assert R.AREAS.tolist() == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]] and R.MAX_DETS.tolist() == [1, 10, 100]


def test_a_two_boxes_with_equal_iou_the_later_one_is_taken():
    out = ref('a_equal_iou_takes_the_later')
    m, ig = out['match_gt'][0], out['ignore'][0]
    assert (m[0] == 1).all() and (m[1] == 0).all()
    assert (ig[:, [ALL, SMALL]] == 0).all() and (ig[:, [MEDIUM, LARGE]] == 1).all()            # area 100: ignored as medium / large, matched all the same
    assert out['npig'][0, 0].tolist() == [2, 2, 0, 0]
    assert (out['precision'][0, :, :, 0, ALL, 2] == 1.0).all() and (out['precision'][0, :, :, 0, MEDIUM] == -1).all()
    assert out['witness']['order_tie'] > 0


def test_b_a_not_ignored_box_with_lower_iou_wins_over_an_ignored_one():
    out = ref('b_not_ignored_before_ignored')
    m, ig = out['match_gt'][0][0], out['ignore'][0][0]
    for a in (ALL, SMALL):
        assert m[a].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0] and ig[a].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1]
    for a in (MEDIUM, LARGE):                           # both ignored: annotation order, the higher IoU stays
        assert m[a].tolist() == [0] * 10 and ig[a].tolist() == [1] * 10


def test_c_a_crowd_box_absorbs_detections_with_iou_over_the_detection_area():
    out = ref('c_crowd_absorbs')
    m, ig = out['match_gt'][0], out['ignore'][0]
    assert (m[:3] == 0).all() and (ig[:3] == 1).all()                                         # three inside: all matched to the crowd box, all ignored
    assert R.iou((90, 0, 20, 20), (0, 0, 100, 100), 1) == 0.5 and R.iou((90, 0, 20, 20), (0, 0, 100, 100), 0) == 200 / 10200
    assert (m[3, :, 0] == 0).all() and (ig[3, :, 0] == 1).all() and (m[3, :, 1:] == -1).all()
    assert (ig[3, [ALL, SMALL], 1:] == 0).all() and (ig[3, [MEDIUM, LARGE], 1:] == 1).all()   # unmatched, 400 px^2
    assert (m[4] == 1).all() and ig[4, :, 0].tolist() == [0, 1, 0, 1]                         # 2500 px^2 is medium
    assert out['npig'][0, 0].tolist() == [1, 0, 1, 0]
    tp = (m[:, ALL, 0] >= 0) & (ig[:, ALL, 0] == 0)
    fp = (m[:, ALL, 0] < 0) & (ig[:, ALL, 0] == 0)
    assert tp.tolist() == [False, False, False, False, True] and not fp.any()
    assert out['recall'][0, 0, 0, ALL, 2] == 1.0 and (out['precision'][0, 0, :, 0, ALL, 2] == 1 / (1 + E)).all()


def test_d_iou_exactly_equal_to_the_threshold_matches():
    out = ref('d_iou_equal_to_the_threshold')
    m = out['match_gt'][0]
    assert R.iou((0, 0, 10, 10), (0, 0, 10, 20), 0) == 0.5 and R.iou((0, 0, 30, 10), (0, 0, 40, 10), 0) == 0.75
    for a in (ALL, SMALL):
        assert m[0, a].tolist() == [0] + [-1] * 9
        assert m[1, a].tolist() == [1] * 6 + [-1] * 4
        assert m[2, a].tolist() == [2] * 10                                                     # identical boxes: matched at 0.95 too
    assert (out['ignore'][0][:, ALL] == 0).all()


def test_e_areas_of_exactly_1024_and_9216_count_in_both_ranges():
    out = ref('e_area_bounds_are_inclusive')
    assert out['npig'][0, 0].tolist() == [3, 1, 3, 2]                                           # the third box: its area field, not w * h
    assert (out['precision'][0, :, :, 0] == 0).all() and (out['recall'][0, :, 0] == 0).all()   # no detection: zeros, not -1
    assert (out['precision'][0, :, :, 1] == -1).all()
    assert R.summarize(out['precision'][0], out['recall'][0]).tolist() == [0.0] * 12


def test_f_unmatched_outside_the_range_is_ignored_matched_inside_counts():
    out = ref('f_unmatched_outside_the_range')
    m, ig = out['match_gt'][0][0], out['ignore'][0][0]
    assert R.iou((0, 0, 30, 30), (0, 0, 40, 40), 0) == 0.5625
    for a in range(4):
        assert m[a].tolist() == [0, 0] + [-1] * 8
    assert ig[ALL].tolist() == [0] * 10
    assert ig[SMALL].tolist() == [1, 1] + [0] * 8           # the 1600 px^2 box is ignored as small; unmatched, 900 px^2 is a small false positive
    assert ig[MEDIUM].tolist() == [0, 0] + [1] * 8          # matched to an in-range box: counts, though 900 px^2 is not medium; unmatched: ignored
    assert ig[LARGE].tolist() == [1] * 10
    assert out['recall'][0, :, 0, MEDIUM, 2].tolist() == [1, 1] + [0] * 8


def test_g_the_101st_of_equal_scores_in_input_order_is_out():
    out = ref('g_101_equal_scores')
    assert out['rank'][0].tolist() == list(range(100)) + [-1]
    assert (out['match_gt'][0][100] == -1).all() and out['witness']['truncated'] == 1
    assert (out['match_gt'][0][0] == 0).all() and (out['match_gt'][0][1:] == -1).all()


def test_h_a_category_without_not_ignored_ground_truth_is_minus_one_and_out_of_the_means():
    out = ref('h_category_without_ground_truth')
    assert (out['precision'][0, :, :, 1] == -1).all() and (out['recall'][0, :, 1] == -1).all() and out['npig'][0, 1].tolist() == [0] * 4
    assert (out['match_gt'][0][1] == 1).all() and (out['ignore'][0][1] == 1).all()
    stats = R.summarize(out['precision'][0], out['recall'][0])
    assert (out['precision'][0, :, :, 0, ALL, 2] == 1 / (1 + E)).all()                         # one TP: 1 / (0 + 1 + 2^-52)
    assert stats[0] == pytest.approx(1.0, abs=1e-15) and stats[8] == 1.0 and stats[3] == -1 and stats[5] == -1           # 2500 px^2: medium only
    assert R.summarize(out['precision'][0][:, :, 1:], out['recall'][0][:, 1:]).tolist() == [-1.0] * 12


def test_i_a_score_tie_across_images_resolves_by_image_order():
    name = 'i_score_tie_across_images'
    out = ref(name)
    packed = R.case_reference(name, None)[4][0]
    assert packed['source_row'].tolist() == [1, 0]                                              # image 'a' (the false positive) goes first
    assert (out['precision'][0, :, :, 0, ALL, 2] == 0.5).all() and (out['recall'][0, :, 0, ALL, 2] == 1).all()


def test_j_the_101_point_read_out_of_a_three_step_curve():
    out = ref('j_three_step_curve')
    expected = [1 / (1 + E)] * 34 + [2 / (3 + E)] * 33 + [3 / (5 + E)] * 34
    for t in range(10):
        assert out['precision'][0, t, :, 0, ALL, 2].tolist() == expected
        assert out['precision'][0, t, :, 0, ALL, 0].tolist() == [1 / (1 + E)] * 34 + [0.0] * 67   # one detection per image
    assert out['recall'][0, 0, 0, ALL].tolist() == [1 / 3, 1.0, 1.0]
    stats = R.summarize(out['precision'][0], out['recall'][0])
    assert stats[0] == pytest.approx((34 + 33 * 2 / 3 + 34 * .6) / 101, abs=1e-12) and stats[6] == pytest.approx(1 / 3, abs=1e-15)


def test_k_dt_images_changes_npig():
    a, b = ref('k_all_images'), ref('k_dt_images')
    assert a['npig'][0, 0, ALL] == 2 and b['npig'][0, 0, ALL] == 1
    assert a['recall'][0, 0, 0, ALL, 2] == 0.5 and b['recall'][0, 0, 0, ALL, 2] == 1.0


@pytest.mark.parametrize('k_sets', [1, 2, 3])
def test_the_random_cases_show_every_event(k_sets):
    w = R.case_reference('random%d' % k_sets, lambda: CC.random_case(k_sets, k_sets))[5]['witness']
    print(w)
    assert w['match'] > 0 and w['crowd_match'] > 0 and w['ignored_unmatched'] > 0 and w['truncated'] > 0 and w['order_tie'] > 0


def test_the_shapes_case_has_the_stated_problem_sizes():
    _, _, _, gt, packed, out = R.case_reference('shapes', CC.shapes_case)
    assert np.diff(gt['image_gt_offsets']).tolist() == [0, 1, 63, 64, 65, 130, 130, 300, 0, 280]
    assert np.diff(packed[0]['image_det_offsets']).tolist() == [165, 101, 100, 99, 1, 0, 165, 40, 0, 160]
    s9 = packed[0]['cat'][packed[0]['image'] == 9]
    assert 40 < (s9 == 0).sum() <= 100 and 40 < (s9 == 1).sum() <= 100 and (gt['cat'][-280:] == np.arange(280) % 2).all()
    assert out['witness']['truncated'] == 3 and out['witness']['crowd_match'] > 0 and out['witness']['order_tie'] > 0


def test_packing_errors_name_the_row():
    gt = R.ground_truth(CC.hand_cases()['k_all_images'][0])
    with pytest.raises(ValueError, match='row 0 is on image zz'):
        R.result(gt, [CC.det('zz', 1, [0, 0, 1, 1], .5)])
    with pytest.raises(ValueError, match='row 1'):
        R.result(gt, [CC.det('a', 1, [0, 0, 1, 1], .5), CC.det('a', 1, [0, 0, float('nan'), 1], .5)])
    assert len(R.result(gt, [CC.det('a', 9, [0, 0, 1, 1], .5)])['score']) == 0                  # an undefined category takes no part
