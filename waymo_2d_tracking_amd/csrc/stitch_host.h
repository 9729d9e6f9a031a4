// Host side of wt_stitch_tracks_host (track_stitch.hip): the input it takes and the layout checks it makes before it touches a
// device.  Host code only, so that the checks can also be compiled into a program of their own (tools/stitch_layout_check.cpp).
#pragma once
#include "refine_host.h"

namespace wt {

// R tracking results and J jobs as wt_stitch_tracks_host takes them (include/waymotrack.h), in the order of its arguments.
struct StitchInput {
    int64_t n_frames;
    int32_t n_streams;
    const int64_t* stream_frame_offsets;
    int32_t r_sets;
    const int64_t *set_row_offsets, *frame_row_offsets;
    const double *x, *y, *w, *h;
    const int32_t *category, *local, *n_traj;
    int32_t n_jobs;
    const int32_t *job_result, *job_max_link;
    const double* job_link_iou;
    const int32_t* job_motion;
    int32_t n_classes;
};

// The layout as refinement checks it (check_refine_layout: arguments, CSR cover, frame order, classes, local indices, one row per
// trajectory and slot); then what the match relies on - the local indices of every (result, stream) number its trajectories by
// first appearance, none missing, so that first slots ascend with the index - and the job parameters.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_stitch_layout(const StitchInput& in, int64_t* max_traj, int64_t* n_traj_total) {
    const char* entry = "wt_stitch_tracks_host";
    if (in.r_sets < 1 || in.n_jobs < 0 || in.n_streams < 0 || in.n_frames < 0 || in.n_classes < 1 || !in.stream_frame_offsets ||
        !in.set_row_offsets || !in.frame_row_offsets || !in.n_traj ||
        (in.n_jobs && (!in.job_result || !in.job_max_link || !in.job_link_iou || !in.job_motion))) {
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
    for (int32_t r = 0; r < in.r_sets; ++r) {
        const int64_t* fro = in.frame_row_offsets + (size_t)r * (size_t)(in.n_frames + 1);
        const int64_t base = in.set_row_offsets[r];
        for (int32_t s = 0; s < in.n_streams; ++s) {
            const int64_t T = in.n_traj[(size_t)r * in.n_streams + s];
            int64_t seen = 0;                         // trajectories met so far: the next new one must carry this index
            for (int64_t i = base + fro[in.stream_frame_offsets[s]]; i < base + fro[in.stream_frame_offsets[s + 1]]; ++i) {
                if (in.local[i] > seen) {
                    set_error("result %d, row %lld: trajectory index %d before %lld appeared (indices number the trajectories by first appearance)",
                              (int)r, (long long)(i - base), (int)in.local[i], (long long)seen);
                    return WT_ERR_INVALID;
                }
                if (in.local[i] == seen) ++seen;
            }
            if (seen != T) {
                set_error("result %d, stream %d: %lld trajectories declared, %lld occur", (int)r, (int)s, (long long)T, (long long)seen);
                return WT_ERR_INVALID;
            }
        }
    }
    for (int32_t j = 0; j < in.n_jobs; ++j) {
        if (in.job_result[j] < 0 || in.job_result[j] >= in.r_sets) { set_error("job %d: result %d outside 0..%d", (int)j, (int)in.job_result[j], (int)in.r_sets - 1); return WT_ERR_INVALID; }
        if (in.job_motion[j] != 0 && in.job_motion[j] != 1) { set_error("job %d: motion must be 0 (hold) or 1 (linear)", (int)j); return WT_ERR_INVALID; }
        for (int32_t c = 0; c < in.n_classes; ++c) {
            if (in.job_max_link[(size_t)j * in.n_classes + c] < 0) { set_error("job %d: max_link of class %d is negative", (int)j, (int)c + 1); return WT_ERR_INVALID; }
            const double v = in.job_link_iou[(size_t)j * in.n_classes + c];
            if (v != v) { set_error("job %d: link_iou of class %d is NaN", (int)j, (int)c + 1); return WT_ERR_INVALID; }
        }
    }
    return WT_OK;
}

}  // namespace wt
