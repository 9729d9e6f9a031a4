// The layout checks of wt_det_eval_host and wt_det_coco_host (csrc/det_metric_host.h) as a program of their own, for a host
// sanitizer:
//
//     hipcc -Xarch_host -fsanitize=address,undefined -g -O1 tools/det_metric_layout_check.cpp -o det_metric_layout_check && ./det_metric_layout_check
//
// It feeds check_det_layout and the row walks of both metrics one valid layout and the malformed ones the entry points must
// refuse, prints what each gave and returns 0 when every answer is the expected one.  No device is touched.
#include "../waymo_2d_tracking_amd/csrc/det_metric_host.h"
#include <limits>
#include <vector>

#include "layout_check_common.h"

namespace {

struct Case {                                   // three images (2 + 0 + 2 boxes), two results (3 + 2 rows), two classes
    std::vector<int64_t> igo = {0, 2, 2, 4}, sro = {0, 3, 5}, ido = {0, 1, 3, 3, /* result 1 */ 0, 0, 1, 2};
    std::vector<int32_t> label = {1, 2, 1, 2}, category = {1, 2, 2, 1, 1};             // section 16: 1..2; section 28 takes them less 1
    std::vector<std::vector<double>> g = std::vector<std::vector<double>>(5, {1, 2, 3, 4}), d = std::vector<std::vector<double>>(5, {1, 2, 3, 4, 5});
    wt::DetLayout layout() const { return {4, 3, 2, igo.data(), sro.data(), ido.data()}; }
};

int check_eval(const Case& c) {
    const int rc = wt::check_det_layout(c.layout(), "wt_det_eval_host");
    return rc != WT_OK ? rc : wt::check_det_eval_rows(c.layout(), c.label.data(), c.category.data(), 2);
}

int check_coco(const Case& c) {
    std::vector<int32_t> g_cat = c.label, cat = c.category;
    for (int32_t& v : g_cat) --v;
    for (int32_t& v : cat) --v;
    const double* g[5] = {c.g[0].data(), c.g[1].data(), c.g[2].data(), c.g[3].data(), c.g[4].data()};
    const double* d[5] = {c.d[0].data(), c.d[1].data(), c.d[2].data(), c.d[3].data(), c.d[4].data()};
    const int rc = wt::check_det_layout(c.layout(), "wt_det_coco_host");
    return rc != WT_OK ? rc : wt::check_det_coco_rows(c.layout(), g, g_cat.data(), d, cat.data(), 2);
}

void expect(const char* name, int (*check)(const Case&), const Case& c, int want, const char* text) {
    wt::g_error[0] = 0;
    const int rc = check(c);
    report(name, rc, rc == want && (want == WT_OK ? wt::g_error[0] == 0 : std::string(wt::g_error).find(text) != std::string::npos));
}

void expect_both(const char* name, const Case& c, const char* text) {
    expect(name, check_eval, c, WT_ERR_INVALID, text);
    expect(name, check_coco, c, WT_ERR_INVALID, text);
}

}  // namespace

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    expect("valid (section 16)", check_eval, Case(), WT_OK, "");
    expect("valid (section 28)", check_coco, Case(), WT_OK, "");
    { Case c; c.igo[0] = 1; expect_both("box offsets do not start at 0", c, "_host: CSR offsets do not cover the rows"); }
    { Case c; c.igo[3] = 5; expect_both("box offsets do not cover", c, "_host: CSR offsets do not cover the rows"); }
    { Case c; c.sro[0] = 1; expect_both("set offsets do not start at 0", c, "_host: CSR offsets do not cover the rows"); }
    { Case c; c.igo[1] = 3; expect_both("box offsets decrease", c, "image_gt_offsets must be non-decreasing (image 1)"); }
    { Case c; c.ido[0] = 1; expect_both("row offsets do not start at 0", c, "result set 0: image_det_offsets do not cover its rows"); }
    { Case c; c.ido[7] = 3; expect_both("row offsets do not cover", c, "result set 1: image_det_offsets do not cover its rows"); }
    { Case c; c.ido[5] = 2; c.ido[6] = 1; expect_both("row offsets decrease", c, "result set 1: image_det_offsets must be non-decreasing (image 1)"); }
    { Case c; c.sro[2] = 2; expect_both("row count below 0", c, "result set 1: image_det_offsets do not cover its rows"); }
    { Case c; c.label[1] = 0; expect("label 0", check_eval, c, WT_ERR_INVALID, "ground-truth row 1: label 0 outside 1..2"); }
    { Case c; c.label[3] = 3; expect("label n_classes + 1", check_eval, c, WT_ERR_INVALID, "ground-truth row 3: label 3 outside 1..2"); }
    { Case c; c.category[3] = 0; expect("result label 0", check_eval, c, WT_ERR_INVALID, "result set 1, row 0: category 0 outside 1..2"); }
    { Case c; c.category[2] = 3; expect("result label n_classes + 1", check_eval, c, WT_ERR_INVALID, "result set 0, row 2: category 3 outside 1..2"); }
    { Case c; c.label[0] = 0; expect("category -1", check_coco, c, WT_ERR_INVALID, "ground-truth row 0: category index -1 outside 0..1"); }
    { Case c; c.label[2] = 3; expect("category n_cats", check_coco, c, WT_ERR_INVALID, "ground-truth row 2: category index 2 outside 0..1"); }
    { Case c; c.category[4] = 0; expect("result category -1", check_coco, c, WT_ERR_INVALID, "result set 1, row 1: category index -1 outside 0..1"); }
    { Case c; c.category[0] = 3; expect("result category n_cats", check_coco, c, WT_ERR_INVALID, "result set 0, row 0: category index 2 outside 0..1"); }
    { Case c; c.g[2][1] = nan; expect("NaN box width", check_coco, c, WT_ERR_INVALID, "ground-truth row 1: a coordinate or the area is not finite"); }
    { Case c; c.g[4][3] = inf; expect("infinite box area", check_coco, c, WT_ERR_INVALID, "ground-truth row 3: a coordinate or the area is not finite"); }
    { Case c; c.d[0][4] = nan; expect("NaN score", check_coco, c, WT_ERR_INVALID, "result set 1, row 1: the score or a coordinate is not finite"); }
    { Case c; c.d[1][2] = -inf; expect("infinite result x", check_coco, c, WT_ERR_INVALID, "result set 0, row 2: the score or a coordinate is not finite"); }
    return summary();
}
