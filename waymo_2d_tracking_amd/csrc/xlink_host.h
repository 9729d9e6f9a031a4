// Host side of wt_xlink_tracks_host (track_xlink.hip): the input it takes and the checks it makes before it touches a device.
// Host code only, so that the checks can also be compiled into a program of their own (tools/xlink_layout_check.cpp).
#pragma once
#include "tracks_host.h"
#include <cstring>

namespace wt {

constexpr int32_t kXLinkMaxClasses = 16;      // the classes of a chain travel as one mask per root

// R tracking results (no score column) and J jobs as wt_xlink_tracks_host takes them (include/waymotrack.h).
struct XLinkInput : TrackSet {
    int32_t n_jobs;
    const int32_t *job_result, *job_pair_max_link;      // [J], [J][C][C]
    const double* job_pair_link_iou;                    // [J][C][C]
    const int32_t *job_class_prio, *job_motion;         // [J][C], [J]
};

// The two pair tables of job j: every entry in its range and both symmetric, the doubles bit for bit.
inline int check_xlink_pair_tables(const int32_t* max_link, const double* link_iou, int32_t j, int32_t n_classes) {
    const size_t C = (size_t)n_classes, o = (size_t)j * C * C;
    for (size_t a = 0; a < C; ++a)
        for (size_t b = 0; b < C; ++b) {
            const size_t k = o + a * C + b, t = o + b * C + a;
            const int ca = (int)a + 1, cb = (int)b + 1;
            if (max_link[k] < 0) { set_error("job %d: max_link of pair (%d, %d) is negative", (int)j, ca, cb); return WT_ERR_INVALID; }
            const double v = link_iou[k];
            if (v != v) { set_error("job %d: link_iou of pair (%d, %d) is NaN", (int)j, ca, cb); return WT_ERR_INVALID; }
            if (max_link[k] != max_link[t] || std::memcmp(&v, &link_iou[t], sizeof(double)) != 0) {
                set_error("job %d: pair (%d, %d) and pair (%d, %d) differ (the tables must be symmetric)", (int)j, ca, cb, cb, ca);
                return WT_ERR_INVALID;
            }
        }
    return WT_OK;
}

// The layout (check_trackset_layout) with what the match relies on - local indices by first appearance, so that first slots
// ascend with the index - then the job parameters.
// On WT_OK: *max_traj is the largest n_traj and *n_traj_total their sum.
inline int check_xlink_layout(const XLinkInput& in, int64_t* max_traj, int64_t* n_traj_total) {
    WT_TRY(check_trackset_layout(in, "wt_xlink_tracks_host", kFirstAppearance,
                                 in.n_jobs >= 0 && (!in.n_jobs || (in.job_result && in.job_pair_max_link && in.job_pair_link_iou &&
                                                                   in.job_class_prio && in.job_motion)),
                                 max_traj, n_traj_total));
    if (in.n_classes > kXLinkMaxClasses) { set_error("wt_xlink_tracks_host: %d classes, at most %d", (int)in.n_classes, (int)kXLinkMaxClasses); return WT_ERR_INVALID; }
    return check_job_results(in.job_result, in.n_jobs, in.r_sets, [&](int32_t j) {
        WT_TRY(check_link_motion(in.job_motion, j));
        return check_xlink_pair_tables(in.job_pair_max_link, in.job_pair_link_iou, j, in.n_classes);
    });
}

}  // namespace wt
