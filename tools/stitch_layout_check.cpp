// The layout checks of wt_stitch_tracks_host (csrc/stitch_host.h) as a program of their own, for a host sanitizer:
//
//     hipcc -Xarch_host -fsanitize=address,undefined -g -O1 tools/stitch_layout_check.cpp -o stitch_layout_check && ./stitch_layout_check
//
// It feeds check_stitch_layout one valid layout and the malformed ones the entry point must refuse, prints what each gave and
// returns 0 when every answer is the expected one.  No device is touched.
#include "../waymo_2d_tracking_amd/csrc/stitch_host.h"

#include "layout_check_common.h"

namespace {

struct Case {                                   // two results over two streams (3 + 2 slots), two jobs, four classes
    std::vector<int64_t> sfo = {0, 3, 5}, sro = {0, 5, 7};
    std::vector<int64_t> fro = {0, 2, 2, 3, 5, 5, /* result 1 */ 0, 0, 1, 1, 1, 2};
    std::vector<double> v = {1, 2, 3, 4, 5, 6, 7};
    std::vector<int32_t> cat = {1, 2, 1, 4, 1, 3, 3}, local = {0, 1, 0, 0, 1, 0, 0}, n_traj = {2, 2, 1, 1};
    std::vector<int32_t> job_result = {0, 1}, link = {0, 1, 2, 3, 0, 0, 0, 0}, motion = {0, 1};
    std::vector<double> iou = {0.3, 0.0, -1.0, 2.0, 0.5, 0.5, 0.5, 0.5};
    wt::StitchInput in() const {
        return {{5, 2, sfo.data(), 2, sro.data(), fro.data(), v.data(), v.data(), v.data(), v.data(), nullptr, cat.data(), local.data(),
                 n_traj.data(), 4}, 2, job_result.data(), link.data(), iou.data(), motion.data()};
    }
};

void expect(const char* name, const Case& c, int want, const char* text) { expect_input(name, c.in(), wt::check_stitch_layout, want, text); }

}  // namespace

int main() {
    Case c;
    expect("valid", c, WT_OK, "");
    { Case d; d.fro[2] = 1; expect("frames not sorted", d, WT_ERR_INVALID, "non-decreasing"); }
    { Case d; d.fro[11] = 3; expect("offsets beyond the rows", d, WT_ERR_INVALID, "do not fit its rows"); }
    { Case d; d.sfo[2] = 4; expect("streams do not cover", d, WT_ERR_INVALID, "do not cover"); }
    { Case d; d.cat[3] = 5; expect("class above n_classes", d, WT_ERR_INVALID, "category 5 outside"); }
    { Case d; d.local[1] = 0; expect("duplicate in a slot", d, WT_ERR_INVALID, "trajectory 0 occurs twice in frame 0"); }
    { Case d; d.local[4] = 2; expect("local index = count", d, WT_ERR_INVALID, "trajectory index 2 outside"); }
    { Case d; d.local[5] = -1; expect("negative local index", d, WT_ERR_INVALID, "trajectory index -1 outside"); }
    { Case d; d.n_traj[3] = -1; expect("negative trajectory count", d, WT_ERR_INVALID, "negative trajectory count"); }
    { Case d; d.local[0] = 1; d.local[1] = 0; expect("not by first appearance", d, WT_ERR_INVALID, "by first appearance"); }
    { Case d; d.local[3] = 1; d.local[4] = 0; expect("second stream against appearance", d, WT_ERR_INVALID, "trajectory index 1 before 0 appeared"); }
    { Case d; d.n_traj[2] = 2; expect("a declared trajectory is missing", d, WT_ERR_INVALID, "2 trajectories declared, 1 occur"); }
    { Case d; d.n_traj = {0, 0, 0, 0}; expect("no trajectories declared", d, WT_ERR_INVALID, "trajectory index 0 outside"); }
    { Case d; d.job_result[1] = 2; expect("job names no result", d, WT_ERR_INVALID, "result 2 outside"); }
    { Case d; d.job_result[0] = -1; expect("job names result -1", d, WT_ERR_INVALID, "result -1 outside"); }
    { Case d; d.link[5] = -1; expect("negative max_link", d, WT_ERR_INVALID, "max_link of class 2"); }
    { Case d; d.iou[6] = std::nan(""); expect("NaN link_iou", d, WT_ERR_INVALID, "link_iou of class 3 is NaN"); }
    { Case d; d.iou[0] = INFINITY; d.iou[1] = -INFINITY; expect("infinite link_iou is a number", d, WT_OK, ""); }
    { Case d; d.motion[0] = 2; expect("unknown motion", d, WT_ERR_INVALID, "motion must be"); }
    {
        Case d;
        wt::StitchInput in = d.in();
        in.job_link_iou = nullptr;
        expect_input("jobs without link_iou", in, wt::check_stitch_layout, WT_ERR_INVALID, "wt_stitch_tracks_host: bad argument");
    }
    return summary();
}
