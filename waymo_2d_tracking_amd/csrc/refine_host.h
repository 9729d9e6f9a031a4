// Host side of wt_refine_tracks_host (track_refine.hip): the input it takes and the layout checks it makes before it touches a
// device.  Host code only, so that the checks can also be compiled into a program of their own (tools/refine_layout_check.cpp).
#pragma once
#include "common.h"
#include <vector>

namespace wt {

// R tracking results and J jobs as wt_refine_tracks_host takes them (include/waymotrack.h), in the order of its arguments.
struct RefineInput {
    int64_t n_frames;
    int32_t n_streams;
    const int64_t* stream_frame_offsets;
    int32_t r_sets;
    const int64_t *set_row_offsets, *frame_row_offsets;
    const double *x, *y, *w, *h, *score;
    const int32_t *category, *local, *n_traj;
    int32_t n_jobs;
    const int32_t *job_result, *job_max_gap, *job_min_len, *job_score_mode;
    int32_t n_classes;
};

// Arguments, CSR cover, frame order, classes, local indices, one row per trajectory and slot, job parameters.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_refine_layout(const RefineInput& in, int64_t* max_traj, int64_t* n_traj_total) {
    const char* entry = "wt_refine_tracks_host";
    if (in.r_sets < 1 || in.n_jobs < 0 || in.n_streams < 0 || in.n_frames < 0 || in.n_classes < 1 || !in.stream_frame_offsets ||
        !in.set_row_offsets || !in.frame_row_offsets || !in.n_traj || (in.n_jobs && (!in.job_result || !in.job_max_gap || !in.job_min_len || !in.job_score_mode))) {
        set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if (in.stream_frame_offsets[0] != 0 || in.stream_frame_offsets[in.n_streams] != in.n_frames || in.set_row_offsets[0] != 0) {
        set_error("%s: CSR offsets do not cover the rows", entry);
        return WT_ERR_INVALID;
    }
    for (int32_t s = 0; s < in.n_streams; ++s)
        if (in.stream_frame_offsets[s + 1] < in.stream_frame_offsets[s]) { set_error("stream_frame_offsets must be non-decreasing"); return WT_ERR_INVALID; }
    const int64_t n_rows = in.set_row_offsets[in.r_sets];
    if (n_rows > 0 && (!in.x || !in.y || !in.w || !in.h || !in.score || !in.category || !in.local)) {
        set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    *max_traj = 0;
    *n_traj_total = 0;
    std::vector<int64_t> seen;                        // per trajectory of the stream: the last slot that had it, + 1
    for (int32_t r = 0; r < in.r_sets; ++r) {
        const int64_t* fro = in.frame_row_offsets + (size_t)r * (size_t)(in.n_frames + 1);
        const int64_t base = in.set_row_offsets[r], rows = in.set_row_offsets[r + 1] - base;
        if (rows < 0 || fro[0] != 0 || fro[in.n_frames] > rows) { set_error("result %d: frame_row_offsets do not fit its rows", (int)r); return WT_ERR_INVALID; }
        for (int32_t s = 0; s < in.n_streams; ++s) {
            const int64_t T = in.n_traj[(size_t)r * in.n_streams + s];
            if (T < 0) { set_error("result %d, stream %d: negative trajectory count", (int)r, (int)s); return WT_ERR_INVALID; }
            if (T > *max_traj) *max_traj = T;
            *n_traj_total += T;
            seen.assign((size_t)T, 0);
            for (int64_t f = in.stream_frame_offsets[s]; f < in.stream_frame_offsets[s + 1]; ++f) {
                if (fro[f + 1] < fro[f]) { set_error("result %d: frame_row_offsets must be non-decreasing", (int)r); return WT_ERR_INVALID; }
                for (int64_t i = base + fro[f]; i < base + fro[f + 1]; ++i) {
                    if (in.category[i] < 1 || in.category[i] > in.n_classes) {
                        set_error("result %d, row %lld: category %d outside 1..%d", (int)r, (long long)(i - base), (int)in.category[i], (int)in.n_classes);
                        return WT_ERR_INVALID;
                    }
                    const int64_t t = in.local[i];
                    if (t < 0 || t >= T) {
                        set_error("result %d, row %lld: trajectory index %lld outside 0..%lld", (int)r, (long long)(i - base), (long long)t, (long long)T - 1);
                        return WT_ERR_INVALID;
                    }
                    if (seen[(size_t)t] == f + 1) {
                        set_error("result %d: trajectory %lld occurs twice in frame %lld", (int)r, (long long)t, (long long)f);
                        return WT_ERR_INVALID;
                    }
                    seen[(size_t)t] = f + 1;
                }
            }
        }
    }
    for (int32_t j = 0; j < in.n_jobs; ++j) {
        if (in.job_result[j] < 0 || in.job_result[j] >= in.r_sets) { set_error("job %d: result %d outside 0..%d", (int)j, (int)in.job_result[j], (int)in.r_sets - 1); return WT_ERR_INVALID; }
        if (in.job_score_mode[j] != 0 && in.job_score_mode[j] != 1) { set_error("job %d: score_mode must be 0 (keep) or 1 (mean)", (int)j); return WT_ERR_INVALID; }
        for (int32_t c = 0; c < in.n_classes; ++c) {
            if (in.job_max_gap[(size_t)j * in.n_classes + c] < 0) { set_error("job %d: max_gap of class %d is negative", (int)j, (int)c + 1); return WT_ERR_INVALID; }
            if (in.job_min_len[(size_t)j * in.n_classes + c] < 1) { set_error("job %d: min_len of class %d is below 1", (int)j, (int)c + 1); return WT_ERR_INVALID; }
        }
    }
    return WT_OK;
}

}  // namespace wt
