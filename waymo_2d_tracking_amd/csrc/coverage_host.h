// Host side of wt_mot_coverage_host (mot_coverage.hip): the layout checks it makes before it touches a device, on top of those
// every tracking metric shares (eval_host.h).  Kept in a header of its own so that tools/coverage_layout_check.cpp can run them
// under a host sanitizer.
#pragma once
#include "eval_host.h"

namespace wt {

constexpr int kCoverageMaxTraj = 4096;          // trajectories of one (stream, class): the evaluators' limit
constexpr int64_t kCoverageMaxFrames = 65535;   // frames of one stream, likewise

// What the coverage call takes: the CLEAR-MOT input (g_id / h_id are object ids), and beside it the ground truth's trajectory
// indices with their counts per (stream, class).
struct CoverageInput {
    TrackInput in;
    const int32_t* g_traj;
    const int32_t* g_ntraj;
};

// The checks of wt_mot_eval_host (ids not negative, at most once per frame and class) and of the trajectory columns (an index
// inside its (stream, class)'s count, at most once per frame).  max_traj: the largest count; total_traj: their sum.
inline int check_coverage_layout(const CoverageInput& ci, int64_t* max_traj, int64_t* total_traj) {
    const TrackInput& in = ci.in;
    WT_TRY(check_track_layout(in, "wt_mot_coverage_host", ci.g_ntraj && (in.n_gt == 0 || (ci.g_traj && in.g_id && in.g_category && in.g_level)), 16));
    int64_t mx = 0, total = 0;
    for (size_t i = 0; i < (size_t)in.n_streams * (size_t)in.n_classes; ++i) {
        if (ci.g_ntraj[i] < 0) { set_error("g_ntraj[%zu] is negative", i); return WT_ERR_INVALID; }
        mx = std::max<int64_t>(mx, ci.g_ntraj[i]);
        total += ci.g_ntraj[i];
    }
    const int32_t C = in.n_classes;
    WT_TRY(walk_track_frames(in,
        [&](int32_t s, int64_t f, int64_t r0, int64_t r1) {
            if (r0 < 0 || r1 > in.n_gt) { set_error("frame_gt_offsets of frame %lld lie outside the rows", (long long)f); return WT_ERR_INVALID; }
            for (int64_t r = r0; r < r1; ++r)
                if (in.g_id[r] < 0) { set_error("ground-truth row %lld: negative object id", (long long)r); return WT_ERR_INVALID; }
            if (!frame_ids_unique(in.g_category, in.g_id, r0, r1, C, [](int64_t) { return true; })) {
                set_error("ground truth: an object id occurs twice in frame %lld", (long long)f);
                return WT_ERR_INVALID;
            }
            const int32_t* counts = ci.g_ntraj + (size_t)s * C;
            if (!frame_ids_unique(in.g_category, ci.g_traj, r0, r1, C,
                                  [&](int64_t r) { return ci.g_traj[r] >= 0 && ci.g_traj[r] < counts[in.g_category[r] - 1]; })) {
                set_error("ground truth: a trajectory index is out of range or occurs twice in frame %lld", (long long)f);
                return WT_ERR_INVALID;
            }
            return WT_OK;
        },
        [&](int32_t k, int32_t, int64_t f, int64_t r0, int64_t r1) {
            if (frame_ids_unique(in.h_category, in.h_id, r0, r1, C, [&](int64_t r) { return in.h_id[r] >= 0; })) return WT_OK;
            set_error("result set %d: an object id is negative or occurs twice in frame %lld", (int)k, (long long)f);
            return WT_ERR_INVALID;
        }));
    for (int32_t s = 0; s < in.n_streams; ++s)
        if (in.stream_frame_offsets[s + 1] - in.stream_frame_offsets[s] > kCoverageMaxFrames) {
            set_error("stream %d has %lld frames: at most %lld", (int)s, (long long)(in.stream_frame_offsets[s + 1] - in.stream_frame_offsets[s]),
                      (long long)kCoverageMaxFrames);
            return WT_ERR_CAPACITY;
        }
    if (mx > kCoverageMaxTraj) {
        set_error("%lld trajectories of one class in one stream: at most %d", (long long)mx, kCoverageMaxTraj);
        return WT_ERR_CAPACITY;
    }
    *max_traj = mx;
    *total_traj = total;
    return WT_OK;
}

// After check_coverage_layout(): what sizes wt_mot_eval_dev's scratch, the most boxes of one class in one frame on either side
// and the number of ground-truth ids.
inline void coverage_eval_bounds(const TrackInput& in, int64_t* max_boxes, int32_t* max_gt_ids) {
    std::vector<int64_t> per_class((size_t)in.n_classes);
    int64_t most = 0;
    auto frame = [&](const int32_t* cat, int64_t r0, int64_t r1) {
        std::fill(per_class.begin(), per_class.end(), 0);
        for (int64_t r = r0; r < r1; ++r)
            if (cat[r] >= 1 && cat[r] <= in.n_classes) most = std::max(most, ++per_class[(size_t)cat[r] - 1]);
    };
    int32_t max_id = -1;
    for (int64_t r = 0; r < in.n_gt; ++r) max_id = std::max(max_id, in.g_id[r]);
    (void)walk_track_frames(in, [&](int32_t, int64_t, int64_t r0, int64_t r1) { frame(in.g_category, r0, r1); return WT_OK; },
                            [&](int32_t, int32_t, int64_t, int64_t r0, int64_t r1) { frame(in.h_category, r0, r1); return WT_OK; });
    *max_boxes = most;
    *max_gt_ids = max_id + 1;
}

}  // namespace wt
