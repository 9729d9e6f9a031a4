// Host side of wt_dedup_tracks_host (track_dedup.hip): the input it takes and the checks it makes before it touches a device.
// Host code only, so that the checks can also be compiled into a program of their own (tools/dedup_layout_check.cpp).
#pragma once
#include "tracks_host.h"

namespace wt {

// R tracking results and J jobs as wt_dedup_tracks_host takes them (include/waymotrack.h).
struct DedupInput : TrackSet {
    int32_t n_jobs;
    const int32_t *job_result, *job_min_frames;
    const double *job_dup_iou, *job_dup_frac;
};

// The layout (check_trackset_layout) with what the match relies on - local indices by first appearance - and what the strength
// order relies on - finite scores, so that the order is strict and total - then the job parameters.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_dedup_layout(const DedupInput& in, int64_t* max_traj, int64_t* n_traj_total) {
    WT_TRY(check_trackset_layout(in, "wt_dedup_tracks_host", kNeedsScore | kFirstAppearance | kFiniteScores,
                                 in.n_jobs >= 0 && (!in.n_jobs || (in.job_result && in.job_min_frames && in.job_dup_iou && in.job_dup_frac)),
                                 max_traj, n_traj_total));
    return check_job_results(in.job_result, in.n_jobs, in.r_sets, [&](int32_t j) {
        for (int32_t c = 0; c < in.n_classes; ++c) {
            const size_t k = (size_t)j * in.n_classes + c;
            if (in.job_min_frames[k] < 0) { set_error("job %d: min_frames of class %d is negative", (int)j, (int)c + 1); return WT_ERR_INVALID; }
            const double v = in.job_dup_iou[k], q = in.job_dup_frac[k];
            if (v != v) { set_error("job %d: dup_iou of class %d is NaN", (int)j, (int)c + 1); return WT_ERR_INVALID; }
            if (!(q >= 0.0 && q <= 1.0)) { set_error("job %d: dup_frac of class %d is outside 0..1", (int)j, (int)c + 1); return WT_ERR_INVALID; }
        }
        return WT_OK;
    });
}

}  // namespace wt
