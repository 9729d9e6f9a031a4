// Host side of wt_stitch_tracks_host (track_stitch.hip): the input it takes and the checks it makes before it touches a device.
// Host code only, so that the checks can also be compiled into a program of their own (tools/stitch_layout_check.cpp).
#pragma once
#include "tracks_host.h"

namespace wt {

// R tracking results (no score column) and J jobs as wt_stitch_tracks_host takes them (include/waymotrack.h).
struct StitchInput : TrackSet {
    int32_t n_jobs;
    const int32_t *job_result, *job_max_link;
    const double* job_link_iou;
    const int32_t* job_motion;
};

// The layout (check_trackset_layout) with what the match relies on - local indices by first appearance, so that first slots
// ascend with the index - then the job parameters.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_stitch_layout(const StitchInput& in, int64_t* max_traj, int64_t* n_traj_total) {
    WT_TRY(check_trackset_layout(in, "wt_stitch_tracks_host", kFirstAppearance,
                                 in.n_jobs >= 0 && (!in.n_jobs || (in.job_result && in.job_max_link && in.job_link_iou && in.job_motion)),
                                 max_traj, n_traj_total));
    return check_job_results(in.job_result, in.n_jobs, in.r_sets, [&](int32_t j) {
        WT_TRY(check_link_motion(in.job_motion, j));
        for (int32_t c = 0; c < in.n_classes; ++c) {
            if (in.job_max_link[(size_t)j * in.n_classes + c] < 0) { set_error("job %d: max_link of class %d is negative", (int)j, (int)c + 1); return WT_ERR_INVALID; }
            const double v = in.job_link_iou[(size_t)j * in.n_classes + c];
            if (v != v) { set_error("job %d: link_iou of class %d is NaN", (int)j, (int)c + 1); return WT_ERR_INVALID; }
        }
        return WT_OK;
    });
}

}  // namespace wt
