// Host side of wt_split_tracks_host (track_split.hip): the input it takes and the checks it makes before it touches a device.
// Host code only, so that the checks can also be compiled into a program of their own (tools/split_layout_check.cpp).
#pragma once
#include "tracks_host.h"

namespace wt {

// R tracking results (no score column) and J jobs as wt_split_tracks_host takes them (include/waymotrack.h).
struct SplitInput : TrackSet {
    int32_t n_jobs;
    const int32_t* job_result;
    const double* job_split_iou;
    const int32_t *job_split_gap, *job_motion;
};

// The layout (check_trackset_layout; the local indices may number a stream's trajectories in any order), then the job parameters.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_split_layout(const SplitInput& in, int64_t* max_traj, int64_t* n_traj_total) {
    WT_TRY(check_trackset_layout(in, "wt_split_tracks_host", 0,
                                 in.n_jobs >= 0 && (!in.n_jobs || (in.job_result && in.job_split_iou && in.job_split_gap && in.job_motion)),
                                 max_traj, n_traj_total));
    return check_job_results(in.job_result, in.n_jobs, in.r_sets, [&](int32_t j) {
        if (in.job_motion[j] != 0 && in.job_motion[j] != 1) { set_error("job %d: motion must be 0 (hold) or 1 (linear)", (int)j); return WT_ERR_INVALID; }
        for (int32_t c = 0; c < in.n_classes; ++c) {
            const double v = in.job_split_iou[(size_t)j * in.n_classes + c];
            if (v != v) { set_error("job %d: split_iou of class %d is NaN", (int)j, (int)c + 1); return WT_ERR_INVALID; }
            if (in.job_split_gap[(size_t)j * in.n_classes + c] < 0) { set_error("job %d: split_gap of class %d is negative", (int)j, (int)c + 1); return WT_ERR_INVALID; }
        }
        return WT_OK;
    });
}

}  // namespace wt
