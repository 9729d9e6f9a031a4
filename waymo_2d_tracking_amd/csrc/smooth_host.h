// Host side of wt_smooth_tracks_host (track_smooth.hip): the input it takes and the checks it makes before it touches a device.
// Host code only, so that the checks can also be compiled into a program of their own (tools/smooth_layout_check.cpp).
#pragma once
#include "tracks_host.h"

namespace wt {

// R tracking results (no score column) and J jobs as wt_smooth_tracks_host takes them (include/waymotrack.h).
struct SmoothInput : TrackSet {
    int32_t n_jobs;
    const int32_t *job_result, *job_window;
    const double* job_weights;
    int32_t n_weights;
};

// The layout (check_trackset_layout), then the job parameters: windows in 0..WT_SMOOTH_MAX_WINDOW and below n_weights, weights
// that are finite and not negative, the centre weight above 0.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_smooth_layout(const SmoothInput& in, int64_t* max_traj, int64_t* n_traj_total) {
    WT_TRY(check_trackset_layout(in, "wt_smooth_tracks_host", 0,
                                 in.n_jobs >= 0 && in.n_weights >= 1 && (!in.n_jobs || (in.job_result && in.job_window && in.job_weights)),
                                 max_traj, n_traj_total));
    return check_job_results(in.job_result, in.n_jobs, in.r_sets, [&](int32_t j) {
        for (int32_t c = 0; c < in.n_classes; ++c) {
            const int32_t W = in.job_window[(size_t)j * in.n_classes + c];
            if (W < 0 || W > WT_SMOOTH_MAX_WINDOW) {
                set_error("job %d: window %d of class %d outside 0..%d", (int)j, (int)W, (int)c + 1, WT_SMOOTH_MAX_WINDOW);
                return WT_ERR_INVALID;
            }
            if (W >= in.n_weights) {
                set_error("job %d: window %d of class %d needs %d weights, %d given", (int)j, (int)W, (int)c + 1, (int)W + 1, (int)in.n_weights);
                return WT_ERR_INVALID;
            }
            const double* k = in.job_weights + ((size_t)j * in.n_classes + c) * (size_t)in.n_weights;
            for (int32_t d = 0; d < in.n_weights; ++d) {
                if (!(k[d] - k[d] == 0.0)) { set_error("job %d: weight %d of class %d is not finite", (int)j, (int)d, (int)c + 1); return WT_ERR_INVALID; }
                if (k[d] < 0.0) { set_error("job %d: weight %d of class %d is negative", (int)j, (int)d, (int)c + 1); return WT_ERR_INVALID; }
            }
            if (!(k[0] > 0.0)) { set_error("job %d: weight 0 of class %d must be above 0", (int)j, (int)c + 1); return WT_ERR_INVALID; }
        }
        return WT_OK;
    });
}

}  // namespace wt
