// The layout checks of wt_split_tracks_host (csrc/split_host.h) as a program of their own, for a host sanitizer:
//
//     hipcc -Xarch_host -fsanitize=address,undefined -g -O1 tools/split_layout_check.cpp -o split_layout_check && ./split_layout_check
//
// It feeds check_split_layout one valid layout and the malformed ones the entry point must refuse, prints what each gave and
// returns 0 when every answer is the expected one.  No device is touched.
#include "../waymo_2d_tracking_amd/csrc/split_host.h"

#include "layout_check_common.h"

namespace {

struct Case {                                   // two results over two streams (3 + 2 slots), two jobs, four classes
    std::vector<int64_t> sfo = {0, 3, 5}, sro = {0, 5, 7};
    std::vector<int64_t> fro = {0, 2, 2, 3, 5, 5, /* result 1 */ 0, 0, 1, 1, 1, 2};
    std::vector<double> v = {1, 2, 3, 4, 5, 6, 7};
    std::vector<int32_t> cat = {1, 2, 1, 4, 1, 3, 3}, local = {0, 1, 0, 0, 1, 0, 0}, n_traj = {2, 2, 1, 1};
    std::vector<int32_t> job_result = {0, 1}, gap = {0, 1, 2, 3, 0, 0, 0, 0}, motion = {0, 1};
    std::vector<double> iou = {0.3, 0.0, -1.0, 2.0, 0.5, 0.5, 0.5, 0.5};
    wt::SplitInput in() const {
        return {{5, 2, sfo.data(), 2, sro.data(), fro.data(), v.data(), v.data(), v.data(), v.data(), nullptr, cat.data(), local.data(),
                 n_traj.data(), 4}, 2, job_result.data(), iou.data(), gap.data(), motion.data()};
    }
};

void expect(const char* name, const Case& c, int want, const char* text) { expect_input(name, c.in(), wt::check_split_layout, want, text); }

}  // namespace

int main() {
    Case c;
    expect("valid", c, WT_OK, "");
    { Case d; d.local[0] = 1; d.local[1] = 0; d.local[2] = 1; expect("indices in another order", d, WT_OK, ""); }
    { Case d; d.fro[2] = 1; expect("frames not sorted", d, WT_ERR_INVALID, "non-decreasing"); }
    { Case d; d.fro[11] = 3; expect("offsets beyond the rows", d, WT_ERR_INVALID, "do not fit its rows"); }
    { Case d; d.fro[6] = 1; expect("offsets do not start at 0", d, WT_ERR_INVALID, "do not fit its rows"); }
    { Case d; d.sfo[2] = 4; expect("streams do not cover", d, WT_ERR_INVALID, "do not cover"); }
    { Case d; d.sfo[1] = 6; expect("stream offsets descend", d, WT_ERR_INVALID, "stream_frame_offsets must be non-decreasing"); }
    { Case d; d.cat[3] = 5; expect("class above n_classes", d, WT_ERR_INVALID, "category 5 outside"); }
    { Case d; d.cat[6] = 0; expect("class 0", d, WT_ERR_INVALID, "category 0 outside"); }
    { Case d; d.local[1] = 0; expect("duplicate in a slot", d, WT_ERR_INVALID, "trajectory 0 occurs twice in frame 0"); }
    { Case d; d.local[4] = 2; expect("local index = count", d, WT_ERR_INVALID, "trajectory index 2 outside"); }
    { Case d; d.local[5] = -1; expect("negative local index", d, WT_ERR_INVALID, "trajectory index -1 outside"); }
    { Case d; d.n_traj[3] = -1; expect("negative trajectory count", d, WT_ERR_INVALID, "negative trajectory count"); }
    { Case d; d.n_traj = {0, 0, 0, 0}; expect("no trajectories declared", d, WT_ERR_INVALID, "trajectory index 0 outside"); }
    { Case d; d.job_result[1] = 2; expect("job names no result", d, WT_ERR_INVALID, "result 2 outside"); }
    { Case d; d.job_result[0] = -1; expect("job names result -1", d, WT_ERR_INVALID, "result -1 outside"); }
    { Case d; d.gap[5] = -1; expect("negative split_gap", d, WT_ERR_INVALID, "job 1: split_gap of class 2 is negative"); }
    { Case d; d.iou[6] = std::nan(""); expect("NaN split_iou", d, WT_ERR_INVALID, "job 1: split_iou of class 3 is NaN"); }
    { Case d; d.iou[0] = INFINITY; d.iou[1] = -INFINITY; expect("infinite split_iou is a number", d, WT_OK, ""); }
    { Case d; d.motion[0] = 2; expect("unknown motion", d, WT_ERR_INVALID, "job 0: motion must be"); }
    {
        Case d;
        wt::SplitInput in = d.in();
        in.job_split_iou = nullptr;
        expect_input("jobs without split_iou", in, wt::check_split_layout, WT_ERR_INVALID, "wt_split_tracks_host: bad argument");
    }
    {
        Case d;
        wt::SplitInput in = d.in();
        in.local = nullptr;
        expect_input("rows without local indices", in, wt::check_split_layout, WT_ERR_INVALID, "wt_split_tracks_host: bad argument");
    }
    {
        Case d;
        wt::SplitInput in = d.in();
        in.n_jobs = -1;
        expect_input("negative job count", in, wt::check_split_layout, WT_ERR_INVALID, "wt_split_tracks_host: bad argument");
    }
    return summary();
}
