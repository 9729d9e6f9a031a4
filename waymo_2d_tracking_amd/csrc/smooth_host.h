// Host side of wt_smooth_tracks_host (track_smooth.hip): the input it takes and the layout checks it makes before it touches a
// device.  Host code only, so that the checks can also be compiled into a program of their own (tools/smooth_layout_check.cpp).
#pragma once
#include "refine_host.h"

namespace wt {

// R tracking results and J jobs as wt_smooth_tracks_host takes them (include/waymotrack.h), in the order of its arguments.
struct SmoothInput {
    int64_t n_frames;
    int32_t n_streams;
    const int64_t* stream_frame_offsets;
    int32_t r_sets;
    const int64_t *set_row_offsets, *frame_row_offsets;
    const double *x, *y, *w, *h;
    const int32_t *category, *local, *n_traj;
    int32_t n_jobs;
    const int32_t *job_result, *job_window;
    const double* job_weights;
    int32_t n_weights, n_classes;
};

// The layout as refinement checks it (check_refine_layout: arguments, CSR cover, frame order, classes, local indices, one row per
// trajectory and slot); then the job parameters: the result, windows in 0..WT_SMOOTH_MAX_WINDOW and below n_weights, weights that
// are finite and not negative, the centre weight above 0.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_smooth_layout(const SmoothInput& in, int64_t* max_traj, int64_t* n_traj_total) {
    const char* entry = "wt_smooth_tracks_host";
    if (in.r_sets < 1 || in.n_jobs < 0 || in.n_streams < 0 || in.n_frames < 0 || in.n_classes < 1 || in.n_weights < 1 || !in.stream_frame_offsets ||
        !in.set_row_offsets || !in.frame_row_offsets || !in.n_traj || (in.n_jobs && (!in.job_result || !in.job_window || !in.job_weights))) {
        set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if (in.stream_frame_offsets[0] != 0 || in.stream_frame_offsets[in.n_streams] != in.n_frames || in.set_row_offsets[0] != 0) {
        set_error("%s: CSR offsets do not cover the rows", entry);
        return WT_ERR_INVALID;
    }
    if (in.set_row_offsets[in.r_sets] > 0 && (!in.x || !in.y || !in.w || !in.h || !in.category || !in.local)) {
        set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    const RefineInput layout = {in.n_frames, in.n_streams, in.stream_frame_offsets, in.r_sets, in.set_row_offsets, in.frame_row_offsets,
                                in.x, in.y, in.w, in.h, in.x /* no score column: not read */, in.category, in.local, in.n_traj,
                                0, nullptr, nullptr, nullptr, nullptr, in.n_classes};
    WT_TRY(check_refine_layout(layout, max_traj, n_traj_total));
    for (int32_t j = 0; j < in.n_jobs; ++j) {
        if (in.job_result[j] < 0 || in.job_result[j] >= in.r_sets) { set_error("job %d: result %d outside 0..%d", (int)j, (int)in.job_result[j], (int)in.r_sets - 1); return WT_ERR_INVALID; }
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
    }
    return WT_OK;
}

}  // namespace wt
