// The layout and job checks of wt_xclass_tracks_host (csrc/xclass_host.h) as a program of their own, for a host sanitizer:
//
//     hipcc -Xarch_host -fsanitize=address,undefined -g -O1 tools/xclass_layout_check.cpp -o xclass_layout_check && ./xclass_layout_check
//
// It feeds check_xclass_layout one valid layout and the malformed ones the entry point must refuse, prints what each gave and
// returns 0 when every answer is the expected one.  No device is touched.
#include "../waymo_2d_tracking_amd/csrc/xclass_host.h"

#include "layout_check_common.h"

namespace {

struct Case {                                   // two results over two streams (3 + 2 slots), two jobs, four classes
    std::vector<int64_t> sfo = {0, 3, 5}, sro = {0, 5, 7};
    std::vector<int64_t> fro = {0, 2, 2, 3, 5, 5, /* result 1 */ 0, 0, 1, 1, 1, 2};
    std::vector<double> v = {1, 2, 3, 4, 5, 6, 7}, score = {0.5, 0.25, 0.0, -1.5, 1e300, 5e-324, 0.75};
    std::vector<int32_t> cat = {1, 2, 1, 4, 1, 3, 3}, local = {0, 1, 1, 0, 1, 0, 0}, n_traj = {2, 2, 1, 1};
    std::vector<int32_t> job_result = {0, 1}, frames, prio = {0, 0, 0, 1, -5, 0x7fffffff, 0, 0}, measure = {1, 0};
    std::vector<double> overlap, frac;
    Case() : frames(32, 0), overlap(32, 0.7), frac(32, 0.5) {
        set(0, 2, 4, 3, 0.9, 0.5);              // job 0: the rider pair
        set(0, 1, 1, 0x7fffffff, -1.0, 0.0);    //        and a diagonal entry at the edges of its ranges
        set(1, 1, 2, 1, INFINITY, 1.0);         // job 1
        set(1, 3, 4, 0, 2.0, 5e-324);           //        a pair that is off keeps its other entries
    }
    void set(int j, int a, int b, int32_t f, double o, double q) {
        for (int k : {j * 16 + (a - 1) * 4 + (b - 1), j * 16 + (b - 1) * 4 + (a - 1)}) { frames[k] = f; overlap[k] = o; frac[k] = q; }
    }
    wt::XClassInput in() const {
        return {{5, 2, sfo.data(), 2, sro.data(), fro.data(), v.data(), v.data(), v.data(), v.data(), score.data(), cat.data(), local.data(),
                 n_traj.data(), 4}, 2, job_result.data(), frames.data(), overlap.data(), frac.data(), prio.data(), measure.data()};
    }
};

constexpr int at(int j, int a, int b) { return j * 16 + (a - 1) * 4 + (b - 1); }

void expect(const char* name, const Case& c, int want, const char* text) { expect_input(name, c.in(), wt::check_xclass_layout, want, text); }

}  // namespace

int main() {
    Case c;
    expect("valid (parameters at their edges)", c, WT_OK, "");
    { Case d; d.fro[2] = 1; expect("frames not sorted", d, WT_ERR_INVALID, "non-decreasing"); }
    { Case d; d.fro[11] = 3; expect("offsets beyond the rows", d, WT_ERR_INVALID, "do not fit its rows"); }
    { Case d; d.sfo[2] = 4; expect("streams do not cover", d, WT_ERR_INVALID, "wt_xclass_tracks_host: CSR offsets do not cover"); }
    { Case d; d.cat[3] = 5; expect("class above n_classes", d, WT_ERR_INVALID, "category 5 outside"); }
    { Case d; d.cat[6] = 0; expect("class 0", d, WT_ERR_INVALID, "result 1, row 1: category 0 outside"); }
    { Case d; d.local[1] = 0; expect("duplicate in a slot", d, WT_ERR_INVALID, "trajectory 0 occurs twice in frame 0"); }
    { Case d; d.local[4] = 2; expect("local index = count", d, WT_ERR_INVALID, "trajectory index 2 outside"); }
    { Case d; d.local[0] = 1; d.local[1] = 0; expect("not by first appearance", d, WT_ERR_INVALID, "result 0, row 0: trajectory index 1 before 0 appeared"); }
    { Case d; d.n_traj[2] = 2; expect("a declared trajectory is missing", d, WT_ERR_INVALID, "result 1, stream 0: 2 trajectories declared, 1 occur"); }
    { Case d; d.score[2] = std::nan(""); expect("NaN score", d, WT_ERR_INVALID, "result 0, row 2: score is not finite"); }
    { Case d; d.score[6] = INFINITY; expect("infinite score", d, WT_ERR_INVALID, "result 1, row 1: score is not finite"); }
    { Case d; d.job_result[1] = 2; expect("job names no result", d, WT_ERR_INVALID, "job 1: result 2 outside"); }
    { Case d; d.job_result[0] = -1; expect("job names result -1", d, WT_ERR_INVALID, "result -1 outside"); }
    { Case d; d.frames[at(0, 2, 4)] = 4; expect("asymmetric frames", d, WT_ERR_INVALID, "job 0: pair (2, 4) and pair (4, 2) differ"); }
    { Case d; d.overlap[at(1, 2, 1)] = std::nextafter(INFINITY, 0.0); expect("asymmetric overlap", d, WT_ERR_INVALID, "job 1: pair (1, 2) and pair (2, 1) differ"); }
    { Case d; d.frac[at(0, 3, 1)] = std::nextafter(0.5, 1.0); expect("asymmetric frac by one ulp", d, WT_ERR_INVALID, "job 0: pair (1, 3) and pair (3, 1) differ"); }
    { Case d; d.overlap[at(1, 1, 4)] = 0.0; d.overlap[at(1, 4, 1)] = -0.0; expect("0.0 against -0.0", d, WT_ERR_INVALID, "job 1: pair (1, 4) and pair (4, 1) differ"); }
    { Case d; d.set(1, 3, 3, -1, 0.7, 0.5); expect("negative frames", d, WT_ERR_INVALID, "job 1: frames of pair (3, 3) is negative"); }
    { Case d; d.set(0, 2, 4, 3, std::nan(""), 0.5); expect("NaN overlap", d, WT_ERR_INVALID, "job 0: overlap of pair (2, 4) is NaN"); }
    { Case d; d.set(0, 2, 4, 3, 0.9, std::nan("")); expect("NaN frac", d, WT_ERR_INVALID, "job 0: frac of pair (2, 4) is outside 0..1"); }
    { Case d; d.set(1, 4, 4, 3, 0.9, std::nextafter(1.0, 2.0)); expect("frac one ulp above 1", d, WT_ERR_INVALID, "job 1: frac of pair (4, 4) is outside 0..1"); }
    { Case d; d.set(1, 1, 3, 3, 0.9, -5e-324); expect("frac below 0", d, WT_ERR_INVALID, "job 1: frac of pair (1, 3) is outside 0..1"); }
    { Case d; d.measure[1] = 2; expect("measure 2", d, WT_ERR_INVALID, "job 1: measure 2 is neither"); }
    { Case d; d.measure[0] = -1; expect("measure -1", d, WT_ERR_INVALID, "job 0: measure -1 is neither"); }
    {
        Case d;
        wt::XClassInput in = d.in();
        in.job_class_prio = nullptr;
        expect_input("jobs without priorities", in, wt::check_xclass_layout, WT_ERR_INVALID, "wt_xclass_tracks_host: bad argument");
    }
    {
        Case d;
        wt::XClassInput in = d.in();
        in.score = nullptr;
        expect_input("rows without scores", in, wt::check_xclass_layout, WT_ERR_INVALID, "wt_xclass_tracks_host: bad argument");
    }
    {
        Case d;
        wt::XClassInput in = d.in();
        in.n_jobs = 0;
        in.job_result = nullptr; in.job_pair_frames = nullptr; in.job_pair_overlap = nullptr; in.job_pair_frac = nullptr;
        in.job_class_prio = nullptr; in.job_measure = nullptr;
        expect_input("no jobs", in, wt::check_xclass_layout, WT_OK, "");
    }
    return summary();
}
