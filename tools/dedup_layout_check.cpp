// The layout and job checks of wt_dedup_tracks_host (csrc/dedup_host.h) as a program of their own, for a host sanitizer:
//
//     hipcc -Xarch_host -fsanitize=address,undefined -g -O1 tools/dedup_layout_check.cpp -o dedup_layout_check && ./dedup_layout_check
//
// It feeds check_dedup_layout one valid layout and the malformed ones the entry point must refuse, prints what each gave and
// returns 0 when every answer is the expected one.  No device is touched.
#include "../waymo_2d_tracking_amd/csrc/dedup_host.h"

#include "layout_check_common.h"

namespace {

struct Case {                                   // two results over two streams (3 + 2 slots), two jobs, four classes
    std::vector<int64_t> sfo = {0, 3, 5}, sro = {0, 5, 7};
    std::vector<int64_t> fro = {0, 2, 2, 3, 5, 5, /* result 1 */ 0, 0, 1, 1, 1, 2};
    std::vector<double> v = {1, 2, 3, 4, 5, 6, 7}, score = {0.5, 0.25, 0.0, -1.5, 1e300, 5e-324, 0.75};
    std::vector<int32_t> cat = {1, 2, 1, 4, 1, 3, 3}, local = {0, 1, 1, 0, 1, 0, 0}, n_traj = {2, 2, 1, 1};
    std::vector<int32_t> job_result = {0, 1}, min_frames = {0, 1, 2, 3, 0, 0, 0, 0};
    std::vector<double> iou = {0.7, 0.0, -1.0, 2.0, 0.5, 0.5, 0.5, INFINITY}, frac = {0.0, 1.0, 0.5, 5e-324, 0.5, 0.5, 0.5, -0.0};
    wt::DedupInput in() const {
        return {{5, 2, sfo.data(), 2, sro.data(), fro.data(), v.data(), v.data(), v.data(), v.data(), score.data(), cat.data(), local.data(),
                 n_traj.data(), 4}, 2, job_result.data(), min_frames.data(), iou.data(), frac.data()};
    }
};

void expect(const char* name, const Case& c, int want, const char* text) { expect_input(name, c.in(), wt::check_dedup_layout, want, text); }

}  // namespace

int main() {
    Case c;
    expect("valid (thresholds at their edges)", c, WT_OK, "");
    { Case d; d.fro[2] = 1; expect("frames not sorted", d, WT_ERR_INVALID, "non-decreasing"); }
    { Case d; d.fro[11] = 3; expect("offsets beyond the rows", d, WT_ERR_INVALID, "do not fit its rows"); }
    { Case d; d.sfo[2] = 4; expect("streams do not cover", d, WT_ERR_INVALID, "wt_dedup_tracks_host: CSR offsets do not cover"); }
    { Case d; d.sfo[1] = 6; expect("streams not sorted", d, WT_ERR_INVALID, "stream_frame_offsets must be non-decreasing"); }
    { Case d; d.cat[3] = 5; expect("class above n_classes", d, WT_ERR_INVALID, "category 5 outside"); }
    { Case d; d.cat[6] = 0; expect("class 0", d, WT_ERR_INVALID, "result 1, row 1: category 0 outside"); }
    { Case d; d.local[1] = 0; expect("duplicate in a slot", d, WT_ERR_INVALID, "trajectory 0 occurs twice in frame 0"); }
    { Case d; d.local[4] = 2; expect("local index = count", d, WT_ERR_INVALID, "trajectory index 2 outside"); }
    { Case d; d.local[5] = -1; expect("negative local index", d, WT_ERR_INVALID, "trajectory index -1 outside"); }
    { Case d; d.local[0] = 1; d.local[1] = 0; expect("not by first appearance", d, WT_ERR_INVALID, "result 0, row 0: trajectory index 1 before 0 appeared"); }
    { Case d; d.local[4] = 0; d.local[3] = 1; expect("not by first appearance, stream 1", d, WT_ERR_INVALID, "result 0, row 3: trajectory index 1 before 0 appeared"); }
    { Case d; d.n_traj[3] = -1; expect("negative trajectory count", d, WT_ERR_INVALID, "negative trajectory count"); }
    { Case d; d.n_traj[2] = 2; expect("a declared trajectory is missing", d, WT_ERR_INVALID, "result 1, stream 0: 2 trajectories declared, 1 occur"); }
    { Case d; d.n_traj = {0, 0, 0, 0}; expect("no trajectories declared", d, WT_ERR_INVALID, "trajectory index 0 outside"); }
    { Case d; d.score[2] = std::nan(""); expect("NaN score", d, WT_ERR_INVALID, "result 0, row 2: score is not finite"); }
    { Case d; d.score[6] = INFINITY; expect("infinite score", d, WT_ERR_INVALID, "result 1, row 1: score is not finite"); }
    { Case d; d.score[3] = -INFINITY; expect("score -infinity", d, WT_ERR_INVALID, "result 0, row 3: score is not finite"); }
    { Case d; d.job_result[1] = 2; expect("job names no result", d, WT_ERR_INVALID, "job 1: result 2 outside"); }
    { Case d; d.job_result[0] = -1; expect("job names result -1", d, WT_ERR_INVALID, "result -1 outside"); }
    { Case d; d.min_frames[5] = -1; expect("negative min_frames", d, WT_ERR_INVALID, "job 1: min_frames of class 2 is negative"); }
    { Case d; d.min_frames[3] = 0x7fffffff; expect("min_frames INT_MAX", d, WT_OK, ""); }
    { Case d; d.iou[2] = std::nan(""); expect("NaN dup_iou", d, WT_ERR_INVALID, "job 0: dup_iou of class 3 is NaN"); }
    { Case d; d.frac[0] = std::nan(""); expect("NaN dup_frac", d, WT_ERR_INVALID, "job 0: dup_frac of class 1 is outside 0..1"); }
    { Case d; d.frac[7] = std::nextafter(1.0, 2.0); expect("dup_frac one ulp above 1", d, WT_ERR_INVALID, "job 1: dup_frac of class 4 is outside 0..1"); }
    { Case d; d.frac[4] = -5e-324; expect("dup_frac below 0", d, WT_ERR_INVALID, "job 1: dup_frac of class 1 is outside 0..1"); }
    {
        Case d;
        wt::DedupInput in = d.in();
        in.job_dup_frac = nullptr;
        expect_input("jobs without dup_frac", in, wt::check_dedup_layout, WT_ERR_INVALID, "wt_dedup_tracks_host: bad argument");
    }
    {
        Case d;
        wt::DedupInput in = d.in();
        in.score = nullptr;
        expect_input("rows without scores", in, wt::check_dedup_layout, WT_ERR_INVALID, "wt_dedup_tracks_host: bad argument");
    }
    {
        Case d;
        wt::DedupInput in = d.in();
        in.n_jobs = 0;
        in.job_result = nullptr; in.job_min_frames = nullptr; in.job_dup_iou = nullptr; in.job_dup_frac = nullptr;
        expect_input("no jobs", in, wt::check_dedup_layout, WT_OK, "");
    }
    return summary();
}
