// Track stitching on gfx950 (include/waymotrack.h, "Track stitching"; DESIGN.md section 21 has the definition): the second
// association pass.  A trajectory that ends (tail) is linked to one of the same stream and class that begins up to max_link slots
// later (head) when the tail's extrapolated box overlaps the head's first box; the linked pieces take the id of the earliest one.
// R tracking results come in once; J jobs each name a result and their parameters.  No row is added, removed or moved.
//
// The summary, the match in rounds, the roots and the launches are those of link_match_device.h, shared with track_xlink.hip; this
// unit gives them the rules of section 21 as a compile-time policy - its match kernel reads no flag on account of the sharing - and
// labels the rows with their roots.
// Compile with -ffp-contract=off: the extrapolation is x + ((x - xp) / (e - p)) * n with every operation rounded on its own, and
// iou_dd is the IoU the metrics use.
#include "eval_device.h"
#include "tracks_device.h"
#include "link_match_device.h"
#include "stitch_host.h"

using namespace wtdev;
using link::kLdsTraj;

namespace {

struct Layout : link::Layout {                // device pointers
    const int32_t* job_max_link;
    const double* job_link_iou;
};

// Section 21: pairs inside a class, with the class's gap and threshold.
struct StitchPolicy {
    static constexpr bool kRowCounts = false, kRounds = false;
    const int32_t* max_link;
    const double* link_iou;
    struct Row {
        int cls, gap;
        double thr;
        __device__ __forceinline__ int reach() const { return gap; }
        __device__ __forceinline__ bool meets(int cj) const { return cj == cls; }
        __device__ __forceinline__ int max_link(int) const { return gap; }
        __device__ __forceinline__ double threshold(int) const { return thr; }
    };
    __device__ __forceinline__ static StitchPolicy make(const Layout& L, int job) {
        const size_t o = (size_t)job * L.n_classes;
        return {L.job_max_link + o, L.job_link_iou + o};
    }
    __device__ __forceinline__ Row row(int c) const { return {c, max_link[c - 1], link_iou[c - 1]}; }
};

__global__ __launch_bounds__(kWave) void stitch_match_kernel(Layout L, Boxes B, link::Workspace ws, link::Outputs O, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const link::Matched M = link::match_problem<StitchPolicy>(L, B, ws, O, status, smem);
    if (!M.ok) return;
    int err = M.err;
    for (long long d = M.q.rs0 + lane; d < M.end; d += kWave) {
        const int t = L.local[d];
        if (t < 0 || t >= M.q.T) { err = kErrCapacity; continue; }
        O.row_root[M.lbase + d] = M.root[t];
    }
    if (__ballot(err != 0) != 0ull && lane == 0) atomicMax(status, kErrCapacity);
    if (lane == 0) O.links[blockIdx.x] = M.n_links;
}

}  // namespace

extern "C" {

void wt_stitch_tracks_limits(int32_t* lds_trajectories) {
    if (lds_trajectories) *lds_trajectories = kLdsTraj;
}

size_t wt_stitch_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj) {
    return link::workspace_bytes<StitchPolicy>(n_jobs, n_streams, n_rows, n_traj_total, max_traj);
}

int wt_stitch_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                         const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                         int32_t n_jobs, const int32_t* job_result, const int32_t* job_max_link, const double* job_link_iou,
                         const int32_t* job_motion, int32_t n_classes,
                         int32_t* out_pred, int32_t* out_root, double* out_affinity, int32_t* out_row_root, int64_t* out_links,
                         int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    WT_TRY(wt::check_track_args("wt_stitch_tracks_dev", n_frames, n_streams, r_sets, n_rows, n_traj_total, max_traj, n_jobs, n_classes,
                                stream_frame_offsets && set_row_offsets && frame_row_offsets && x && y && w && h && category && local && traj_offsets &&
                                    job_result && job_max_link && job_link_iou && job_motion && out_pred && out_root && out_affinity && out_row_root &&
                                    out_links && status_dev,
                                wt::grid_fits(n_jobs, n_streams) && wt::grid_fits(r_sets, n_streams), link::kGridText, (int)n_jobs, (int)r_sets, (int)n_streams));
    const wt::TrackSet dev = {n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, nullptr,
                              category, local, nullptr, n_classes};
    Layout L;
    wt::fill_track_layout(&L, dev, n_rows, traj_offsets, n_traj_total, max_traj, n_jobs, job_result, kLdsTraj);
    L.job_max_link = job_max_link; L.job_motion = job_motion; L.job_link_iou = job_link_iou;
    const Boxes B = {x, y, w, h};
    const link::Outputs O = {out_pred, out_root, out_affinity, out_row_root, out_links};
    return link::launch<StitchPolicy>("wt_stitch_tracks_dev", stitch_match_kernel, L, B, O, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_stitch_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                          int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                          const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                          const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const int32_t* job_max_link,
                          const double* job_link_iou, const int32_t* job_motion, int32_t n_classes,
                          int32_t* out_pred, int32_t* out_root, double* out_affinity, int32_t* out_row_root, int64_t* out_links) {
    const wt::StitchInput in = {{n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, nullptr,
                                 category, local, n_traj, n_classes}, n_jobs, job_result, job_max_link, job_link_iou, job_motion};
    int64_t max_traj = 0, n_traj_total = 0;
    WT_TRY(wt::check_stitch_layout(in, &max_traj, &n_traj_total));
    const size_t jc = (size_t)n_jobs * (size_t)n_classes;
    wt::DevBuf jl, ji, jm;
    return link::run_host<StitchPolicy, Layout, link::Outputs>("wt_stitch_tracks_host", "stitch", stitch_match_kernel, in, n_jobs, job_result, n_traj_total,
                                                               max_traj, [&](Layout* L, link::Outputs*) {
        WT_TRY(jl.upload(job_max_link, 4 * jc)); WT_TRY(ji.upload(job_link_iou, 8 * jc)); WT_TRY(jm.upload(job_motion, 4 * (size_t)n_jobs));
        L->job_max_link = jl.as<int32_t>(); L->job_link_iou = ji.as<double>(); L->job_motion = jm.as<int32_t>();
        return (int)WT_OK;
    }, {out_pred, out_root, out_affinity, out_row_root, out_links});
}

}  // extern "C"
