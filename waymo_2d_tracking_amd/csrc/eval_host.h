// Host side shared by the *_host forms of the tracking metrics (mot_eval.hip, mot_identity.hip): the input both take, the
// layout checks both make before they touch a device, and the staging of that input in device memory.
#pragma once
#include "common.h"
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace wt {

// Ground truth and K results as wt_mot_eval_* / wt_mot_identity_* take them (include/waymotrack.h), in the order of their arguments.
// g_id / h_id are object ids for CLEAR-MOT and class-local trajectory indices for the identity metric.  Host or device pointers.
struct TrackInput {
    int64_t n_gt;
    const double *gx, *gy, *gw, *gh;
    const int32_t *g_category, *g_level, *g_id;
    int64_t n_frames;
    const int64_t* frame_gt_offsets;
    int32_t n_streams;
    const int64_t* stream_frame_offsets;
    int32_t k_sets;
    const int64_t *set_row_offsets, *frame_hyp_offsets;
    const double *hx, *hy, *hw, *hh;
    const int32_t *h_category, *h_id;
    int32_t n_classes;
};

// Arguments, class count, CSR cover and stream order of a host-side input; `entry` is the name of the entry point ("...._host").
// others_ok: the entry point's own pointers are there.  The class-count text names the metric, as the device form's does.
inline int check_track_layout(const TrackInput& in, const char* entry, bool others_ok, int max_classes) {
    if (in.k_sets < 1 || in.n_streams < 0 || in.n_frames < 0 || in.n_gt < 0 || !in.set_row_offsets || !in.frame_hyp_offsets ||
        !in.frame_gt_offsets || !in.stream_frame_offsets || !others_ok) {
        set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if (in.n_classes < 1 || in.n_classes > max_classes) {
        set_error("%.*s: n_classes must be 1..%d", (int)strlen(entry) - 5, entry, max_classes);
        return WT_ERR_INVALID;
    }
    // ---- the layout must be what the kernel walks: checked here, the device form trusts its caller ----
    if (in.frame_gt_offsets[0] != 0 || in.frame_gt_offsets[in.n_frames] != in.n_gt || in.stream_frame_offsets[0] != 0 ||
        in.stream_frame_offsets[in.n_streams] != in.n_frames || in.set_row_offsets[0] != 0) {
        set_error("%s: CSR offsets do not cover the rows", entry);
        return WT_ERR_INVALID;
    }
    for (int32_t s = 0; s < in.n_streams; ++s)
        if (in.stream_frame_offsets[s + 1] < in.stream_frame_offsets[s]) { set_error("stream_frame_offsets must be non-decreasing"); return WT_ERR_INVALID; }
    return WT_OK;
}

// Rows [r0, r1) of one frame: every row of a class 1..n_classes is valid(r), and no (class, id) occurs twice.
template <class Valid>
bool frame_ids_unique(const int32_t* cat, const int32_t* id, int64_t r0, int64_t r1, int32_t n_classes, Valid valid) {
    static thread_local std::vector<std::pair<int32_t, int32_t>> seen;
    seen.clear();
    for (int64_t r = r0; r < r1; ++r) {
        if (cat[r] < 1 || cat[r] > n_classes) continue;
        if (!valid(r)) return false;
        seen.emplace_back(cat[r], id[r]);
    }
    std::sort(seen.begin(), seen.end());
    return std::adjacent_find(seen.begin(), seen.end()) == seen.end();
}

// Walk the frames in the kernel's order and check the per-frame offsets on the way: gt_frame(s, f, r0, r1) for every
// ground-truth frame, then hyp_frame(k, s, f, r0, r1) for every frame of every result set; the first status that is not
// WT_OK ends the walk.  After check_track_layout().
template <class GtFrame, class HypFrame>
int walk_track_frames(const TrackInput& in, GtFrame gt_frame, HypFrame hyp_frame) {
    for (int32_t s = 0; s < in.n_streams; ++s)
        for (int64_t f = in.stream_frame_offsets[s]; f < in.stream_frame_offsets[s + 1]; ++f) {
            const int64_t r0 = in.frame_gt_offsets[f], r1 = in.frame_gt_offsets[f + 1];
            if (r1 < r0) { set_error("frame_gt_offsets must be non-decreasing"); return WT_ERR_INVALID; }
            WT_TRY(gt_frame(s, f, r0, r1));
        }
    for (int32_t k = 0; k < in.k_sets; ++k) {
        const int64_t* fho = in.frame_hyp_offsets + (size_t)k * (size_t)(in.n_frames + 1);
        const int64_t base = in.set_row_offsets[k], rows = in.set_row_offsets[k + 1] - base;
        if (rows < 0 || fho[0] != 0 || fho[in.n_frames] > rows) { set_error("result set %d: frame_hyp_offsets do not fit its rows", (int)k); return WT_ERR_INVALID; }
        for (int32_t s = 0; s < in.n_streams; ++s)
            for (int64_t f = in.stream_frame_offsets[s]; f < in.stream_frame_offsets[s + 1]; ++f) {
                if (fho[f + 1] < fho[f]) { set_error("result set %d: frame_hyp_offsets must be non-decreasing", (int)k); return WT_ERR_INVALID; }
                WT_TRY(hyp_frame(k, s, f, base + fho[f], base + fho[f + 1]));
            }
    }
    return WT_OK;
}

// The input in device memory, with the status word the kernels report through.  After ensure_device().
struct StagedTrackInput {
    DevBuf gx, gy, gw, gh, gc, gl, gi, fo, so, sr, fh, hx, hy, hw, hh, hc, hi, status;
    TrackInput dev;          // the same input with device pointers
    int64_t n_hyp = 0;

    int upload(const TrackInput& in) {
        n_hyp = in.set_row_offsets[in.k_sets];
        const size_t ng = (size_t)in.n_gt, nh = (size_t)n_hyp, nf = (size_t)(in.n_frames + 1);
        WT_TRY(gx.upload(in.gx, 8 * ng)); WT_TRY(gy.upload(in.gy, 8 * ng)); WT_TRY(gw.upload(in.gw, 8 * ng)); WT_TRY(gh.upload(in.gh, 8 * ng));
        WT_TRY(gc.upload(in.g_category, 4 * ng)); WT_TRY(gl.upload(in.g_level, 4 * ng)); WT_TRY(gi.upload(in.g_id, 4 * ng));
        WT_TRY(fo.upload(in.frame_gt_offsets, 8 * nf)); WT_TRY(so.upload(in.stream_frame_offsets, 8 * (size_t)(in.n_streams + 1)));
        WT_TRY(sr.upload(in.set_row_offsets, 8 * (size_t)(in.k_sets + 1))); WT_TRY(fh.upload(in.frame_hyp_offsets, 8 * (size_t)in.k_sets * nf));
        WT_TRY(hx.upload(in.hx, 8 * nh)); WT_TRY(hy.upload(in.hy, 8 * nh)); WT_TRY(hw.upload(in.hw, 8 * nh)); WT_TRY(hh.upload(in.hh, 8 * nh));
        WT_TRY(hc.upload(in.h_category, 4 * nh)); WT_TRY(hi.upload(in.h_id, 4 * nh));
        WT_TRY(status.alloc(16));
        dev = {in.n_gt, gx.as<double>(), gy.as<double>(), gw.as<double>(), gh.as<double>(), gc.as<int32_t>(), gl.as<int32_t>(), gi.as<int32_t>(),
               in.n_frames, fo.as<int64_t>(), in.n_streams, so.as<int64_t>(), in.k_sets, sr.as<int64_t>(), fh.as<int64_t>(),
               hx.as<double>(), hy.as<double>(), hw.as<double>(), hh.as<double>(), hc.as<int32_t>(), hi.as<int32_t>(), in.n_classes};
        return WT_OK;
    }

    // wait for the launch and read the kernel's status; `what` names the kernel in the message
    int finish(const char* what) {
        WT_HIP(hipDeviceSynchronize());
        int32_t st = 0;
        WT_HIP(hipMemcpy(&st, status.p, sizeof(st), hipMemcpyDeviceToHost));
        if (st) set_error("%s kernel reported status %d (4 = capacity, 5 = assignment did not converge)", what, (int)st);
        return (int)st;
    }
};

}  // namespace wt
