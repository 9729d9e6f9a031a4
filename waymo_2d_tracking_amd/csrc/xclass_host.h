// Host side of wt_xclass_tracks_host (track_xclass.hip): the input it takes and the checks it makes before it touches a device.
// Host code only, so that the checks can also be compiled into a program of their own.
#pragma once
#include "tracks_host.h"
#include <cstring>

namespace wt {

constexpr int32_t kXClassMaxClasses = 16;     // the classes that can be in a pair travel as one mask per job

// R tracking results and J jobs as wt_xclass_tracks_host takes them (include/waymotrack.h).
struct XClassInput : TrackSet {
    int32_t n_jobs;
    const int32_t *job_result, *job_pair_frames;        // [J], [J][C][C]
    const double *job_pair_overlap, *job_pair_frac;     // [J][C][C]
    const int32_t *job_class_prio, *job_measure;        // [J][C], [J]
};

inline bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// The layout (check_trackset_layout) with what the match relies on - local indices by first appearance - and what the strength
// order relies on - finite scores, so that the order is strict and total - then the job parameters: every entry in its range
// and the three tables symmetric, the doubles bit for bit.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_xclass_layout(const XClassInput& in, int64_t* max_traj, int64_t* n_traj_total) {
    WT_TRY(check_trackset_layout(in, "wt_xclass_tracks_host", kNeedsScore | kFirstAppearance | kFiniteScores,
                                 in.n_jobs >= 0 && (!in.n_jobs || (in.job_result && in.job_pair_frames && in.job_pair_overlap && in.job_pair_frac &&
                                                                   in.job_class_prio && in.job_measure)),
                                 max_traj, n_traj_total));
    if (in.n_classes > kXClassMaxClasses) { set_error("wt_xclass_tracks_host: %d classes, at most %d", (int)in.n_classes, (int)kXClassMaxClasses); return WT_ERR_INVALID; }
    return check_job_results(in.job_result, in.n_jobs, in.r_sets, [&](int32_t j) {
        const size_t C = (size_t)in.n_classes, o = (size_t)j * C * C;
        if (in.job_measure[j] != 0 && in.job_measure[j] != 1) { set_error("job %d: measure %d is neither 0 (IoU) nor 1 (IoMin)", (int)j, (int)in.job_measure[j]); return WT_ERR_INVALID; }
        for (size_t a = 0; a < C; ++a)
            for (size_t b = 0; b < C; ++b) {
                const size_t k = o + a * C + b, t = o + b * C + a;
                const int ca = (int)a + 1, cb = (int)b + 1;
                if (in.job_pair_frames[k] < 0) { set_error("job %d: frames of pair (%d, %d) is negative", (int)j, ca, cb); return WT_ERR_INVALID; }
                const double v = in.job_pair_overlap[k], q = in.job_pair_frac[k];
                if (v != v) { set_error("job %d: overlap of pair (%d, %d) is NaN", (int)j, ca, cb); return WT_ERR_INVALID; }
                if (!(q >= 0.0 && q <= 1.0)) { set_error("job %d: frac of pair (%d, %d) is outside 0..1", (int)j, ca, cb); return WT_ERR_INVALID; }
                if (in.job_pair_frames[k] != in.job_pair_frames[t] || !same_bits(v, in.job_pair_overlap[t]) || !same_bits(q, in.job_pair_frac[t])) {
                    set_error("job %d: pair (%d, %d) and pair (%d, %d) differ (the tables must be symmetric)", (int)j, ca, cb, cb, ca);
                    return WT_ERR_INVALID;
                }
            }
        return WT_OK;
    });
}

}  // namespace wt
