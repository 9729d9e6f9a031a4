// Host side of wt_refine_tracks_host (track_refine.hip): the input it takes and the checks it makes before it touches a device.
// Host code only, so that the checks can also be compiled into a program of their own (tools/refine_layout_check.cpp).
#pragma once
#include "tracks_host.h"

namespace wt {

// R tracking results and J jobs as wt_refine_tracks_host takes them (include/waymotrack.h).
struct RefineInput : TrackSet {
    int32_t n_jobs;
    const int32_t *job_result, *job_max_gap, *job_min_len, *job_score_mode;
};

// The layout (check_trackset_layout), then the job parameters.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_refine_layout(const RefineInput& in, int64_t* max_traj, int64_t* n_traj_total) {
    WT_TRY(check_trackset_layout(in, "wt_refine_tracks_host", kNeedsScore | kStreamOrderFirst,
                                 in.n_jobs >= 0 && (!in.n_jobs || (in.job_result && in.job_max_gap && in.job_min_len && in.job_score_mode)),
                                 max_traj, n_traj_total));
    return check_job_results(in.job_result, in.n_jobs, in.r_sets, [&](int32_t j) {
        if (in.job_score_mode[j] != 0 && in.job_score_mode[j] != 1) { set_error("job %d: score_mode must be 0 (keep) or 1 (mean)", (int)j); return WT_ERR_INVALID; }
        for (int32_t c = 0; c < in.n_classes; ++c) {
            if (in.job_max_gap[(size_t)j * in.n_classes + c] < 0) { set_error("job %d: max_gap of class %d is negative", (int)j, (int)c + 1); return WT_ERR_INVALID; }
            if (in.job_min_len[(size_t)j * in.n_classes + c] < 1) { set_error("job %d: min_len of class %d is below 1", (int)j, (int)c + 1); return WT_ERR_INVALID; }
        }
        return WT_OK;
    });
}

}  // namespace wt
