// Host side shared by the track post-passes (track_refine.hip, track_stitch.hip, track_smooth.hip, track_dedup.hip,
// track_split.hip, track_xclass.hip; DESIGN.md section 20, "The shared layer"): the tracking results all six take, the checks every entry point makes on them before it
// touches a device, and the staging of a host-side input in device memory.  Host code only, so that the checks can also be
// compiled into programs of their own (tools/*_layout_check.cpp).
#pragma once
#include "common.h"
#include <vector>

namespace wt {

// R tracking results as the wt_*_tracks_* entry points take them (include/waymotrack.h).  Host or device pointers; score is NULL
// for a stage without a score column, n_traj is NULL in a device form (it takes traj_offsets).
struct TrackSet {
    int64_t n_frames;
    int32_t n_streams;
    const int64_t* stream_frame_offsets;
    int32_t r_sets;
    const int64_t *set_row_offsets, *frame_row_offsets;
    const double *x, *y, *w, *h, *score;
    const int32_t *category, *local, *n_traj;
    int32_t n_classes;
};

enum : unsigned {
    kNeedsScore = 1,            // the stage reads a score column
    kFirstAppearance = 2,       // the local indices of every (result, stream) number its trajectories by first appearance, none missing
    kFiniteScores = 4,          // every score of a row that a slot holds is finite
    kStreamOrderFirst = 8,      // refinement names descending stream offsets before missing columns, the later stages after
};

// Arguments, CSR cover, frame order, classes, local indices, one row per trajectory and slot; then what `flags` ask for.  `entry`
// is the name of the entry point ("...._host"); others_ok: the stage's own counts and pointers are there.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_trackset_layout(const TrackSet& in, const char* entry, unsigned flags, bool others_ok, int64_t* max_traj, int64_t* n_traj_total) {
    if (in.r_sets < 1 || in.n_streams < 0 || in.n_frames < 0 || in.n_classes < 1 || !in.stream_frame_offsets || !in.set_row_offsets ||
        !in.frame_row_offsets || !in.n_traj || !others_ok) {
        set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if (in.stream_frame_offsets[0] != 0 || in.stream_frame_offsets[in.n_streams] != in.n_frames || in.set_row_offsets[0] != 0) {
        set_error("%s: CSR offsets do not cover the rows", entry);
        return WT_ERR_INVALID;
    }
    const bool columns_ok = in.set_row_offsets[in.r_sets] <= 0 ||
                            (in.x && in.y && in.w && in.h && in.category && in.local && (in.score || !(flags & kNeedsScore)));
    if (!columns_ok && !(flags & kStreamOrderFirst)) { set_error("%s: bad argument", entry); return WT_ERR_INVALID; }
    for (int32_t s = 0; s < in.n_streams; ++s)
        if (in.stream_frame_offsets[s + 1] < in.stream_frame_offsets[s]) { set_error("stream_frame_offsets must be non-decreasing"); return WT_ERR_INVALID; }
    if (!columns_ok) { set_error("%s: bad argument", entry); return WT_ERR_INVALID; }
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
    for (int32_t r = 0; r < in.r_sets && (flags & kFirstAppearance); ++r) {   // what a match relies on: first slots ascend with the index
        const int64_t* fro = in.frame_row_offsets + (size_t)r * (size_t)(in.n_frames + 1);
        const int64_t base = in.set_row_offsets[r];
        for (int32_t s = 0; s < in.n_streams; ++s) {
            const int64_t T = in.n_traj[(size_t)r * in.n_streams + s];
            int64_t met = 0;                          // trajectories met so far: the next new one must carry this index
            for (int64_t i = base + fro[in.stream_frame_offsets[s]]; i < base + fro[in.stream_frame_offsets[s + 1]]; ++i) {
                if (in.local[i] > met) {
                    set_error("result %d, row %lld: trajectory index %d before %lld appeared (indices number the trajectories by first appearance)",
                              (int)r, (long long)(i - base), (int)in.local[i], (long long)met);
                    return WT_ERR_INVALID;
                }
                if (in.local[i] == met) ++met;
            }
            if (met != T) {
                set_error("result %d, stream %d: %lld trajectories declared, %lld occur", (int)r, (int)s, (long long)T, (long long)met);
                return WT_ERR_INVALID;
            }
        }
    }
    for (int32_t r = 0; r < in.r_sets && (flags & kFiniteScores); ++r) {      // what a strength order relies on: it is strict and total
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
    return WT_OK;
}

// Every job names a result; params(j) then checks the stage's own parameters of job j, so that the first job at fault is the one named.
template <class Params>
int check_job_results(const int32_t* job_result, int32_t n_jobs, int32_t r_sets, Params params) {
    for (int32_t j = 0; j < n_jobs; ++j) {
        if (job_result[j] < 0 || job_result[j] >= r_sets) { set_error("job %d: result %d outside 0..%d", (int)j, (int)job_result[j], (int)r_sets - 1); return WT_ERR_INVALID; }
        WT_TRY(params(j));
    }
    return WT_OK;
}

// the motion of job j of a linking pass (stitch_host.h, xlink_host.h)
inline int check_link_motion(const int32_t* job_motion, int32_t j) {
    if (job_motion[j] != 0 && job_motion[j] != 1) { set_error("job %d: motion must be 0 (hold) or 1 (linear)", (int)j); return WT_ERR_INVALID; }
    return WT_OK;
}

// a * b blocks fit one grid dimension
inline bool grid_fits(uint64_t a, uint64_t b) { return a * b <= 0x7fffffffull; }

// The counts every entry point takes; others_ok: its own counts and pointers are there.  grid_ok: the stage's launches fit
// their grids; when they do not, grid_text (a format, the entry's name first) with `numbers` says what was too much.
template <class... Numbers>
int check_track_args(const char* entry, int64_t n_frames, int32_t n_streams, int32_t r_sets, int64_t n_rows, int64_t n_traj_total, int64_t max_traj,
                     int32_t n_jobs, int32_t n_classes, bool others_ok, bool grid_ok, const char* grid_text, Numbers... numbers) {
    if (n_frames < 0 || n_streams < 0 || r_sets < 1 || n_rows < 0 || n_traj_total < 0 || max_traj < 0 || n_jobs < 0 || n_classes < 1 || !others_ok) {
        set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if (!grid_ok) { set_error(grid_text, entry, numbers...); return WT_ERR_CAPACITY; }
    return WT_OK;
}

// the caller's workspace holds what the stage carved (`need` bytes behind the first 256-byte boundary); `rc` is what the stage
// answers when it does not
inline int check_workspace_fits(const char* entry, const void* workspace, size_t workspace_bytes, size_t need, int rc) {
    if (!workspace || workspace_bytes < need + 256) {
        set_error("%s: workspace too small: need %zu bytes, have %zu", entry, need + 256, workspace_bytes);
        return rc;
    }
    return WT_OK;
}

// The common fields of a stage's device Layout (tracks_device.h: TrackLayout) from a TrackSet of device pointers.  lds_limit: the
// stage's kLdsTraj when it sizes its tables at launch - max_traj then counts as at least 1 - and 0 when it does not.
template <class Layout>
void fill_track_layout(Layout* L, const TrackSet& dev, int64_t n_rows, const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                       int32_t n_jobs, const int32_t* job_result, int lds_limit) {
    L->n_frames = dev.n_frames; L->n_rows = n_rows; L->n_traj_total = n_traj_total;
    L->max_traj = lds_limit && max_traj < 1 ? 1 : max_traj;
    L->n_streams = dev.n_streams; L->r_sets = dev.r_sets; L->n_jobs = n_jobs; L->n_classes = dev.n_classes;
    L->lds_traj = (int)(L->max_traj < lds_limit ? L->max_traj : lds_limit);
    L->stream_frame_offsets = dev.stream_frame_offsets; L->set_row_offsets = dev.set_row_offsets; L->frame_row_offsets = dev.frame_row_offsets;
    L->traj_offsets = traj_offsets; L->category = dev.category; L->local = dev.local; L->job_result = job_result;
}

// A checked host-side TrackSet in device memory, with the job results, the trajectory offsets the device forms take and the
// status word the kernels report through.  After check_trackset_layout() and ensure_device().
struct StagedTrackSet {
    DevBuf so, sr, fr, dx, dy, dw, dh, ds, dc, dl, dt, jr, status;
    TrackSet dev;            // the same results with device pointers
    int64_t n_rows = 0;

    int upload(const TrackSet& in, int32_t n_jobs, const int32_t* job_result) {
        n_rows = in.set_row_offsets[in.r_sets];
        const size_t nr = (size_t)n_rows, nf = (size_t)(in.n_frames + 1), rs = (size_t)in.r_sets * (size_t)in.n_streams;
        std::vector<int64_t> traj_offsets(rs + 1, 0);
        for (size_t i = 0; i < rs; ++i) traj_offsets[i + 1] = traj_offsets[i] + in.n_traj[i];
        WT_TRY(so.upload(in.stream_frame_offsets, 8 * (size_t)(in.n_streams + 1))); WT_TRY(sr.upload(in.set_row_offsets, 8 * (size_t)(in.r_sets + 1)));
        WT_TRY(fr.upload(in.frame_row_offsets, 8 * (size_t)in.r_sets * nf));
        WT_TRY(dx.upload(in.x, 8 * nr)); WT_TRY(dy.upload(in.y, 8 * nr)); WT_TRY(dw.upload(in.w, 8 * nr)); WT_TRY(dh.upload(in.h, 8 * nr));
        if (in.score) WT_TRY(ds.upload(in.score, 8 * nr));
        WT_TRY(dc.upload(in.category, 4 * nr)); WT_TRY(dl.upload(in.local, 4 * nr)); WT_TRY(dt.upload(traj_offsets.data(), 8 * (rs + 1)));
        WT_TRY(jr.upload(job_result, 4 * (size_t)n_jobs)); WT_TRY(status.alloc(16));
        dev = {in.n_frames, in.n_streams, so.as<int64_t>(), in.r_sets, sr.as<int64_t>(), fr.as<int64_t>(), dx.as<double>(), dy.as<double>(),
               dw.as<double>(), dh.as<double>(), ds.as<double>(), dc.as<int32_t>(), dl.as<int32_t>(), nullptr, in.n_classes};
        return WT_OK;
    }

    // the common fields of the stage's Layout; the totals are those check_trackset_layout() gave
    template <class Layout>
    void fill(Layout* L, int64_t n_traj_total, int64_t max_traj, int32_t n_jobs, int lds_limit) const {
        fill_track_layout(L, dev, n_rows, dt.as<int64_t>(), n_traj_total, max_traj, n_jobs, jr.as<int32_t>(), lds_limit);
    }

    // wait for the launches and read the kernels' status; `what` names the stage in the message, `hint` what status 4 means for it
    int finish(const char* what, const char* hint) {
        WT_HIP(hipDeviceSynchronize());
        int32_t st = 0;
        WT_HIP(hipMemcpy(&st, status.p, sizeof(st), hipMemcpyDeviceToHost));
        if (st) set_error("%s kernel reported status %d (4 = %s that do not fit the rows)", what, (int)st, hint);
        return (int)st;
    }
};

}  // namespace wt
