// The layout checks of wt_smooth_tracks_host (csrc/smooth_host.h) as a program of their own, for a host sanitizer:
//
//     hipcc -Xarch_host -fsanitize=address,undefined -g -O1 tools/smooth_layout_check.cpp -o smooth_layout_check && ./smooth_layout_check
//
// It feeds check_smooth_layout one valid layout and the malformed ones the entry point must refuse, prints what each gave and
// returns 0 when every answer is the expected one.  No device is touched.
#include "../waymo_2d_tracking_amd/csrc/smooth_host.h"

#include "layout_check_common.h"

namespace {

struct Case {                                   // two results over two streams (3 + 2 slots), two jobs, four classes, three weights
    std::vector<int64_t> sfo = {0, 3, 5}, sro = {0, 5, 7};
    std::vector<int64_t> fro = {0, 2, 2, 3, 5, 5, /* result 1 */ 0, 0, 1, 1, 1, 2};
    std::vector<double> v = {1, 2, 3, 4, 5, 6, 7};
    std::vector<int32_t> cat = {1, 2, 1, 4, 1, 3, 3}, local = {1, 0, 1, 0, 1, 0, 0}, n_traj = {2, 2, 1, 1};
    std::vector<int32_t> job_result = {0, 1}, window = {0, 1, 2, 2, 0, 0, 0, 0};
    std::vector<double> k = std::vector<double>(2 * 4 * 3, 1.0);
    int32_t n_weights = 3;
    wt::SmoothInput in() const {
        return {{5, 2, sfo.data(), 2, sro.data(), fro.data(), v.data(), v.data(), v.data(), v.data(), nullptr, cat.data(), local.data(),
                 n_traj.data(), 4}, 2, job_result.data(), window.data(), k.data(), n_weights};
    }
};

void expect(const char* name, const Case& c, int want, const char* text) { expect_input(name, c.in(), wt::check_smooth_layout, want, text); }

}  // namespace

int main() {
    Case c;
    expect("valid (indices in any order)", c, WT_OK, "");
    { Case d; d.fro[2] = 1; expect("frames not sorted", d, WT_ERR_INVALID, "non-decreasing"); }
    { Case d; d.fro[11] = 3; expect("offsets beyond the rows", d, WT_ERR_INVALID, "do not fit its rows"); }
    { Case d; d.sfo[2] = 4; expect("streams do not cover", d, WT_ERR_INVALID, "do not cover"); }
    { Case d; d.sfo[1] = 6; expect("streams not sorted", d, WT_ERR_INVALID, "stream_frame_offsets must be non-decreasing"); }
    { Case d; d.cat[3] = 5; expect("class above n_classes", d, WT_ERR_INVALID, "category 5 outside"); }
    { Case d; d.cat[6] = 0; expect("class 0", d, WT_ERR_INVALID, "result 1, row 1: category 0 outside"); }
    { Case d; d.local[1] = 1; expect("duplicate in a slot", d, WT_ERR_INVALID, "trajectory 1 occurs twice in frame 0"); }
    { Case d; d.local[4] = 2; expect("local index = count", d, WT_ERR_INVALID, "trajectory index 2 outside"); }
    { Case d; d.local[5] = -1; expect("negative local index", d, WT_ERR_INVALID, "trajectory index -1 outside"); }
    { Case d; d.n_traj[3] = -1; expect("negative trajectory count", d, WT_ERR_INVALID, "negative trajectory count"); }
    { Case d; d.n_traj = {0, 0, 0, 0}; expect("no trajectories declared", d, WT_ERR_INVALID, "trajectory index 1 outside"); }
    { Case d; d.job_result[1] = 2; expect("job names no result", d, WT_ERR_INVALID, "job 1: result 2 outside"); }
    { Case d; d.job_result[0] = -1; expect("job names result -1", d, WT_ERR_INVALID, "result -1 outside"); }
    { Case d; d.window[5] = -1; expect("negative window", d, WT_ERR_INVALID, "job 1: window -1 of class 2 outside 0..32"); }
    { Case d; d.window[2] = 33; expect("window above the maximum", d, WT_ERR_INVALID, "job 0: window 33 of class 3 outside 0..32"); }
    { Case d; d.window[3] = 3; expect("window = n_weights", d, WT_ERR_INVALID, "window 3 of class 4 needs 4 weights, 3 given"); }
    {
        Case d;
        d.n_weights = 33;
        d.k.assign(2 * 4 * 33, 0.5);
        d.window[6] = 32;
        expect("window 32 with 33 weights", d, WT_OK, "");
    }
    { Case d; d.k[4] = std::nan(""); expect("NaN weight", d, WT_ERR_INVALID, "job 0: weight 1 of class 2 is not finite"); }
    { Case d; d.k[23] = INFINITY; expect("infinite weight", d, WT_ERR_INVALID, "job 1: weight 2 of class 4 is not finite"); }
    { Case d; d.k[8] = -1e-300; expect("negative weight", d, WT_ERR_INVALID, "job 0: weight 2 of class 3 is negative"); }
    { Case d; d.k[12] = 0.0; expect("centre weight 0", d, WT_ERR_INVALID, "job 1: weight 0 of class 1 must be above 0"); }
    { Case d; d.k[0] = -0.0; expect("centre weight -0", d, WT_ERR_INVALID, "job 0: weight 0 of class 1 must be above 0"); }
    { Case d; d.k[1] = 0.0; d.k[2] = 5e-324; expect("outer weights 0 and denormal", d, WT_OK, ""); }
    { Case d; d.n_weights = 0; expect("no weights", d, WT_ERR_INVALID, "wt_smooth_tracks_host: bad argument"); }
    {
        Case d;
        wt::SmoothInput in = d.in();
        in.job_weights = nullptr;
        expect_input("jobs without weights", in, wt::check_smooth_layout, WT_ERR_INVALID, "wt_smooth_tracks_host: bad argument");
    }
    {
        Case d;
        wt::SmoothInput in = d.in();
        in.n_jobs = 0;
        in.job_result = nullptr; in.job_window = nullptr; in.job_weights = nullptr;
        expect_input("no jobs", in, wt::check_smooth_layout, WT_OK, "");
    }
    return summary();
}
