// The layout checks of wt_mot_coverage_host (csrc/coverage_host.h) as a program of their own, for a host sanitizer:
//
//     hipcc -Xarch_host -fsanitize=address,undefined -g -O1 tools/coverage_layout_check.cpp -o coverage_layout_check && ./coverage_layout_check
//
// It feeds check_coverage_layout one valid layout and the malformed ones the entry point must refuse, prints what each gave and
// returns 0 when every answer is the expected one.  No device is touched.  (hyp_match never comes from the caller of the host
// form: wt_mot_eval_dev writes it in the same call, and the mark pass checks its range on the device.)
#include "../waymo_2d_tracking_amd/csrc/coverage_host.h"

#include "layout_check_common.h"

namespace {

struct Case {                                   // two streams (3 + 2 frames), two classes, seven rows; two results (4 + 2 rows)
    std::vector<int64_t> sfo = {0, 3, 5}, fgo = {0, 2, 2, 4, 6, 7};
    std::vector<double> v = {1, 2, 3, 4, 5, 6, 7};
    std::vector<int32_t> cat = {1, 2, 1, 1, 1, 2, 2}, level = {1, 2, 1, 2, 1, 1, 2}, gid = {0, 1, 0, 2, 0, 1, 1};
    std::vector<int32_t> traj = {0, 0, 0, 1, 0, 0, 0}, ntraj = {2, 1, 1, 2};          // stream 1, class 2 declares one it never shows
    std::vector<int64_t> sro = {0, 4, 6}, fho = {0, 1, 1, 2, 3, 3, /* result 1 */ 0, 0, 0, 0, 1, 1};
    std::vector<int32_t> hcat = {1, 1, 2, 9, 2, 1}, hid = {0, 0, 3, -4, 5, 5};        // the last row of either set takes no part
    int32_t k_sets = 2, n_classes = 2;
    wt::CoverageInput in() const {
        return {{7, v.data(), v.data(), v.data(), v.data(), cat.data(), level.data(), gid.data(), 5, fgo.data(), 2, sfo.data(), k_sets, sro.data(),
                 fho.data(), v.data(), v.data(), v.data(), v.data(), hcat.data(), hid.data(), n_classes}, traj.data(), ntraj.data()};
    }
};

void expect(const char* name, const Case& c, int want, const char* text) { expect_input(name, c.in(), wt::check_coverage_layout, want, text); }

}  // namespace

int main() {
    Case c;
    expect("valid", c, WT_OK, "");
    { Case d; d.fgo[2] = 1; expect("frame offsets not ascending", d, WT_ERR_INVALID, "frame_gt_offsets must be non-decreasing"); }
    { Case d; d.fgo[5] = 6; expect("frame offsets do not cover", d, WT_ERR_INVALID, "wt_mot_coverage_host: CSR offsets do not cover"); }
    { Case d; d.sfo[1] = 6; expect("stream offsets not ascending", d, WT_ERR_INVALID, "stream_frame_offsets must be non-decreasing"); }
    { Case d; d.fho[8] = 1; d.fho[9] = 0; expect("result offsets not ascending", d, WT_ERR_INVALID, "result set 1: frame_hyp_offsets must be non-decreasing"); }
    { Case d; d.fho[11] = 3; expect("result offsets beyond its rows", d, WT_ERR_INVALID, "result set 1: frame_hyp_offsets do not fit its rows"); }
    { Case d; d.traj[3] = 2; expect("g_traj = count", d, WT_ERR_INVALID, "trajectory index is out of range or occurs twice in frame 2"); }
    { Case d; d.traj[6] = -1; expect("g_traj negative", d, WT_ERR_INVALID, "trajectory index is out of range or occurs twice in frame 4"); }
    { Case d; d.traj[3] = 0; expect("g_traj twice in a frame", d, WT_ERR_INVALID, "occurs twice in frame 2"); }
    { Case d; d.traj[1] = 1; expect("g_traj beyond its class's count", d, WT_ERR_INVALID, "out of range or occurs twice in frame 0"); }
    { Case d; d.ntraj[2] = -1; expect("negative trajectory count", d, WT_ERR_INVALID, "g_ntraj[2] is negative"); }
    { Case d; d.ntraj[3] = 4097; expect("4097 trajectories", d, WT_ERR_CAPACITY, "4097 trajectories of one class in one stream"); }
    { Case d; d.gid[5] = -1; expect("negative ground-truth id", d, WT_ERR_INVALID, "ground-truth row 5: negative object id"); }
    { Case d; d.gid[3] = 0; expect("ground-truth id twice", d, WT_ERR_INVALID, "an object id occurs twice in frame 2"); }
    { Case d; d.hid[4] = -1; expect("negative result id", d, WT_ERR_INVALID, "result set 1: an object id is negative or occurs twice in frame 3"); }
    { Case d; d.k_sets = -1; expect("negative K", d, WT_ERR_INVALID, "wt_mot_coverage_host: bad argument"); }
    { Case d; d.k_sets = 0; expect("K = 0", d, WT_ERR_INVALID, "wt_mot_coverage_host: bad argument"); }
    { Case d; d.n_classes = 17; expect("17 classes", d, WT_ERR_INVALID, "wt_mot_coverage: n_classes must be 1..16"); }
    {
        Case d;
        wt::CoverageInput in = d.in();
        in.g_traj = nullptr;
        expect_input("rows without trajectory indices", in, wt::check_coverage_layout, WT_ERR_INVALID, "wt_mot_coverage_host: bad argument");
    }
    {
        Case d;
        wt::CoverageInput in = d.in();
        in.g_ntraj = nullptr;
        expect_input("no trajectory counts", in, wt::check_coverage_layout, WT_ERR_INVALID, "wt_mot_coverage_host: bad argument");
    }
    {
        Case d;                                     // the frame limit: one stream of 65536 empty frames
        d.sfo = {0, 65536, 65536};
        d.fgo.assign(65537, 0);
        d.fho.assign(2 * 65537, 0);
        d.sro = {0, 0, 0};
        wt::CoverageInput in = d.in();
        in.in.n_gt = 0; in.in.n_frames = 65536;
        d.ntraj = {0, 0, 0, 0};
        in.g_ntraj = d.ntraj.data();
        expect_input("65536 frames in a stream", in, wt::check_coverage_layout, WT_ERR_CAPACITY, "stream 0 has 65536 frames");
    }
    return summary();
}
