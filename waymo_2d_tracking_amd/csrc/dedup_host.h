// Host side of wt_dedup_tracks_host (track_dedup.hip): the input it takes and the layout checks it makes before it touches a
// device.  Host code only, so that the checks can also be compiled into a program of their own (tools/dedup_layout_check.cpp).
#pragma once
#include "stitch_host.h"

namespace wt {

// R tracking results and J jobs as wt_dedup_tracks_host takes them (include/waymotrack.h), in the order of its arguments.
struct DedupInput {
    int64_t n_frames;
    int32_t n_streams;
    const int64_t* stream_frame_offsets;
    int32_t r_sets;
    const int64_t *set_row_offsets, *frame_row_offsets;
    const double *x, *y, *w, *h, *score;
    const int32_t *category, *local, *n_traj;
    int32_t n_jobs;
    const int32_t *job_result, *job_min_frames;
    const double *job_dup_iou, *job_dup_frac;
    int32_t n_classes;
};

// The layout as stitching checks it (check_stitch_layout without jobs: arguments, CSR cover, frame order, classes, local indices
// numbered by first appearance, one row per trajectory and slot); then what the strength order relies on - every score of a row
// that a slot holds is finite, so that the order is strict and total - and the job parameters.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_dedup_layout(const DedupInput& in, int64_t* max_traj, int64_t* n_traj_total) {
    const char* entry = "wt_dedup_tracks_host";
    if (in.r_sets < 1 || in.n_jobs < 0 || in.n_streams < 0 || in.n_frames < 0 || in.n_classes < 1 || !in.stream_frame_offsets ||
        !in.set_row_offsets || !in.frame_row_offsets || !in.n_traj ||
        (in.n_jobs && (!in.job_result || !in.job_min_frames || !in.job_dup_iou || !in.job_dup_frac))) {
        set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if (in.stream_frame_offsets[0] != 0 || in.stream_frame_offsets[in.n_streams] != in.n_frames || in.set_row_offsets[0] != 0) {
        set_error("%s: CSR offsets do not cover the rows", entry);
        return WT_ERR_INVALID;
    }
    if (in.set_row_offsets[in.r_sets] > 0 && (!in.x || !in.y || !in.w || !in.h || !in.score || !in.category || !in.local)) {
        set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    const StitchInput layout = {in.n_frames, in.n_streams, in.stream_frame_offsets, in.r_sets, in.set_row_offsets, in.frame_row_offsets,
                                in.x, in.y, in.w, in.h, in.category, in.local, in.n_traj, 0, nullptr, nullptr, nullptr, nullptr, in.n_classes};
    WT_TRY(check_stitch_layout(layout, max_traj, n_traj_total));
    for (int32_t r = 0; r < in.r_sets; ++r) {
        const int64_t* fro = in.frame_row_offsets + (size_t)r * (size_t)(in.n_frames + 1);
        const int64_t base = in.set_row_offsets[r];
        for (int64_t i = base + fro[0]; i < base + fro[in.n_frames]; ++i) {
            const double v = in.score[i];
            if (!(v - v == 0.0)) {
                set_error("result %d, row %lld: score is not finite (the strength order of the tracks needs finite scores)", (int)r, (long long)(i - base));
                return WT_ERR_INVALID;
            }
        }
    }
    for (int32_t j = 0; j < in.n_jobs; ++j) {
        if (in.job_result[j] < 0 || in.job_result[j] >= in.r_sets) { set_error("job %d: result %d outside 0..%d", (int)j, (int)in.job_result[j], (int)in.r_sets - 1); return WT_ERR_INVALID; }
        for (int32_t c = 0; c < in.n_classes; ++c) {
            const size_t k = (size_t)j * in.n_classes + c;
            if (in.job_min_frames[k] < 0) { set_error("job %d: min_frames of class %d is negative", (int)j, (int)c + 1); return WT_ERR_INVALID; }
            const double v = in.job_dup_iou[k], q = in.job_dup_frac[k];
            if (v != v) { set_error("job %d: dup_iou of class %d is NaN", (int)j, (int)c + 1); return WT_ERR_INVALID; }
            if (!(q >= 0.0 && q <= 1.0)) { set_error("job %d: dup_frac of class %d is outside 0..1", (int)j, (int)c + 1); return WT_ERR_INVALID; }
        }
    }
    return WT_OK;
}

}  // namespace wt
