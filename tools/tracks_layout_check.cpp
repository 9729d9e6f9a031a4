// The layout checks of wt_tracks_layout_host and wt_tracks_to_eval_host (csrc/tracks_layout_host.h) as a program of their own, for
// a host sanitizer:
//
//     hipcc -Xarch_host -fsanitize=address,undefined -g -O1 tools/tracks_layout_check.cpp -o tracks_layout_check && ./tracks_layout_check
//
// It feeds check_layout_input and check_to_eval_input one valid input each and the malformed ones the entry points must refuse,
// prints what each gave and returns 0 when every answer is the expected one.  No device is touched.
#include "../waymo_2d_tracking_amd/csrc/tracks_layout_host.h"

#include "layout_check_common.h"

namespace {

struct Rows {                                   // three results of two rows over two streams (3 + 2 slots), four classes
    std::vector<int64_t> sfo = {0, 3, 5}, iro = {0, 2, 4, 6};
    std::vector<int64_t> frame = {0, 4, /* result 1 */ 1, 1, /* result 2 */ 2, 3}, oid = {7, -7, 7, 8, 1ll << 40, 7};
    std::vector<int32_t> cat = {1, 4, 2, 2, 1, 3};
    std::vector<double> bbox = std::vector<double>(24, 1.5), score = {1, 2, 3, 4, 5, 6};
    wt::LayoutInput in() const {
        return {5, 2, sfo.data(), 3, iro.data(), frame.data(), cat.data(), bbox.data(), score.data(), oid.data(), 4};
    }
};

struct Sets {                                   // two results of three rows over five slots, four ground-truth slots, four classes
    std::vector<int64_t> sro = {0, 3, 6};
    std::vector<int64_t> fro = {0, 2, 2, 3, 3, 3, /* result 1 */ 0, 0, 1, 1, 2, 2}, map = {2, -1, 0, 3, -1};
    std::vector<double> v = {1, 2, 3, 4, 5, 6};
    std::vector<int32_t> cat = {1, 0, 5, 2, 2, 2}, local = {0, 1, 0, 0, 1, 0};
    wt::ToEvalInput in() const {
        return {5, 2, sro.data(), fro.data(), v.data(), v.data(), v.data(), v.data(), 1, cat.data(), local.data(), map.data(), 4, 4};
    }
};

void expect(const char* name, const Rows& c, int want, const char* text) { expect_input(name, c.in(), wt::check_layout_input, want, text); }
void expect(const char* name, const Sets& c, int want, const char* text) { expect_input(name, c.in(), wt::check_to_eval_input, want, text); }

}  // namespace

int main() {
    expect("layout: valid", Rows(), WT_OK, "");
    { Rows d; d.frame[1] = 0; d.frame[0] = 1; expect("layout: slots descend once", d, WT_ERR_INVALID, "frame slot 0 after 1"); }
    { Rows d; d.frame[5] = 5; expect("layout: slot = n_frames", d, WT_ERR_INVALID, "frame slot 5 outside 0..4"); }
    { Rows d; d.frame[2] = -1; expect("layout: negative slot", d, WT_ERR_INVALID, "frame slot -1 outside"); }
    { Rows d; d.iro[2] = 1; expect("layout: negative row count", d, WT_ERR_INVALID, "result 1: negative row count"); }
    { Rows d; d.iro[0] = 1; expect("layout: first offset not 0", d, WT_ERR_INVALID, "do not cover"); }
    { Rows d; d.cat[3] = 5; expect("layout: class above n_classes", d, WT_ERR_INVALID, "category 5 outside"); }
    { Rows d; d.cat[4] = 0; expect("layout: class 0", d, WT_ERR_INVALID, "category 0 outside"); }
    { Rows d; d.sfo[2] = 4; expect("layout: streams do not cover", d, WT_ERR_INVALID, "do not cover"); }
    { Rows d; d.sfo[1] = 6; expect("layout: stream offsets descend", d, WT_ERR_INVALID, "non-decreasing"); }
    { Rows d; wt::LayoutInput in = d.in(); in.r_sets = 0; expect_input("layout: no result", in, wt::check_layout_input, WT_ERR_INVALID, "bad argument"); }
    { Rows d; wt::LayoutInput in = d.in(); in.object_id = nullptr; expect_input("layout: a column is missing", in, wt::check_layout_input, WT_ERR_INVALID, "bad argument"); }
    expect("to_eval: valid", Sets(), WT_OK, "");
    { Sets d; d.map[4] = 2; expect("to_eval: a slot is named twice", d, WT_ERR_INVALID, "named by the frame slots 0 and 4"); }
    { Sets d; d.map[1] = 4; expect("to_eval: map beyond the ground truth", d, WT_ERR_INVALID, "ground-truth slot 4 outside"); }
    { Sets d; d.map[1] = -2; expect("to_eval: map below -1", d, WT_ERR_INVALID, "ground-truth slot -2 outside"); }
    { Sets d; d.fro[2] = 1; expect("to_eval: offsets descend", d, WT_ERR_INVALID, "non-decreasing"); }
    { Sets d; d.fro[11] = 4; expect("to_eval: offsets beyond the rows", d, WT_ERR_INVALID, "do not fit its rows"); }
    { Sets d; d.fro[6] = 1; expect("to_eval: first offset not 0", d, WT_ERR_INVALID, "do not fit its rows"); }
    { Sets d; d.sro[1] = 7; expect("to_eval: set offsets descend", d, WT_ERR_INVALID, "result 1: negative row count"); }
    { Sets d; d.sro[0] = 1; expect("to_eval: rows do not begin at 0", d, WT_ERR_INVALID, "do not cover"); }
    { Sets d; d.local[4] = -1; expect("to_eval: negative local index", d, WT_ERR_INVALID, "trajectory index -1 is negative"); }
    { Sets d; wt::ToEvalInput in = d.in(); in.box_stride = 0; expect_input("to_eval: stride 0", in, wt::check_to_eval_input, WT_ERR_INVALID, "bad argument"); }
    return summary();
}
