// Track deduplication on gfx950 (include/waymotrack.h, "Track deduplication"; DESIGN.md section 23 has the definition): track-level
// non-maximum suppression.  Two trajectories of one stream and class whose boxes overlap by dup_iou in at least min_frames slots and
// in at least dup_frac of the shorter one's rows are duplicates; the trajectories are walked from strongest (most rows, then
// highest score sum, then lowest index) to weakest and one is suppressed when a stronger KEPT one is its duplicate.  R tracking
// results come in once; J jobs each name a result and their parameters.  Rows are only selected: no float is produced.
//
// The summary, the match in rounds and the launches are those of dup_match_device.h, shared with track_xclass.hip; this unit gives
// them the rules of section 23 as a compile-time policy - its match kernel reads no flag on account of the sharing.
// Compile with -ffp-contract=off: iou_dd is the IoU the metrics use, and dup_frac * min(n) is one multiplication.
#include "eval_device.h"
#include "tracks_device.h"
#include "dup_match_device.h"
#include "dedup_host.h"

using namespace wtdev;
using dup::kLdsTraj;

namespace {

struct Layout : dup::Layout {                 // device pointers
    const int32_t* job_min_frames;
    const double *job_dup_iou, *job_dup_frac;
};

// Section 23: pairs inside a class, the IoU, more rows before the higher score sum before the lower index, a share of the
// shorter one's rows.
struct DedupPolicy {
    const int32_t* min_frames;
    const double *dup_iou, *dup_frac;
    const int32_t* n;
    const double* ssum;
    int C;
    __device__ __forceinline__ static DedupPolicy make(const Layout& L, int job, const int32_t* n, const double* ssum, const int32_t*) {
        const size_t o = (size_t)job * L.n_classes;
        return {L.job_min_frames + o, L.job_dup_iou + o, L.job_dup_frac + o, n, ssum, L.n_classes};
    }
    // the class when the job deduplicates it, 0 otherwise
    __device__ __forceinline__ int live_class(int c) const { return c >= 1 && c <= C && min_frames[c - 1] > 0 ? c : 0; }
    __device__ __forceinline__ bool pair_live(int ca, int cb) const { return ca == cb; }
    __device__ __forceinline__ double threshold(int ca, int) const { return dup_iou[ca - 1]; }
    __device__ __forceinline__ int frames(int ca, int) const { return min_frames[ca - 1]; }
    __device__ __forceinline__ double measure(const double a[4], const double b[4]) const { return iou_dd(a, b); }
    // t is stronger than u: more rows, then the higher score sum, then the lower index
    __device__ __forceinline__ bool stronger(int t, int u) const {
        const int nt = n[t], nu = n[u];
        if (nt != nu) return nt > nu;
        const double st = ssum[t], su = ssum[u];
        if (st > su) return true;
        if (st < su) return false;
        return t < u;
    }
    __device__ __forceinline__ double need(int ca, int, int t, int u) const {
        const int nt = n[t], nu = n[u];
        return dup_frac[ca - 1] * (double)(nt < nu ? nt : nu);
    }
};

__global__ __launch_bounds__(kWave) void dedup_match_kernel(Layout L, Boxes B, dup::Workspace ws, dup::Outputs O, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    dup::match_problem<DedupPolicy>(L, B, ws, O, status, smem);
}

constexpr const char* kGridText = "%s: %d jobs, %d results x %d streams in one call";

}  // namespace

extern "C" {

void wt_dedup_tracks_limits(int32_t* lds_trajectories) {
    if (lds_trajectories) *lds_trajectories = kLdsTraj;
}

size_t wt_dedup_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj) {
    return dup::workspace_bytes(n_jobs, n_streams, n_rows, n_traj_total, max_traj);
}

int wt_dedup_tracks_rounds(const void* workspace, int32_t n_jobs, int32_t n_streams, int32_t* out_rounds) {
    return dup::read_rounds("wt_dedup_tracks_rounds", workspace, n_jobs, n_streams, out_rounds);
}

int wt_dedup_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                        int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                        const double* x, const double* y, const double* w, const double* h, const double* score,
                        const int32_t* category, const int32_t* local,
                        const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                        int32_t n_jobs, const int32_t* job_result, const int32_t* job_min_frames,
                        const double* job_dup_iou, const double* job_dup_frac, int32_t n_classes,
                        int32_t* out_keep, int32_t* out_by, int32_t* out_match, int32_t* out_row_keep, int64_t* out_dropped,
                        int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    WT_TRY(wt::check_track_args("wt_dedup_tracks_dev", n_frames, n_streams, r_sets, n_rows, n_traj_total, max_traj, n_jobs, n_classes,
                                stream_frame_offsets && set_row_offsets && frame_row_offsets && x && y && w && h && score && category && local &&
                                    traj_offsets && job_result && job_min_frames && job_dup_iou && job_dup_frac && out_keep && out_by && out_match &&
                                    out_row_keep && out_dropped && status_dev,
                                wt::grid_fits(n_jobs, n_streams) && wt::grid_fits(r_sets, n_streams), kGridText, (int)n_jobs, (int)r_sets, (int)n_streams));
    const wt::TrackSet dev = {n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, score,
                              category, local, nullptr, n_classes};
    Layout L;
    wt::fill_track_layout(&L, dev, n_rows, traj_offsets, n_traj_total, max_traj, n_jobs, job_result, kLdsTraj);
    L.score = score; L.job_min_frames = job_min_frames; L.job_dup_iou = job_dup_iou; L.job_dup_frac = job_dup_frac;
    const Boxes B = {x, y, w, h};
    const dup::Outputs O = {out_keep, out_by, out_match, out_row_keep, out_dropped};
    return dup::launch("wt_dedup_tracks_dev", dedup_match_kernel, L, B, O, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_dedup_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const double* score,
                         const int32_t* category, const int32_t* local,
                         const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const int32_t* job_min_frames,
                         const double* job_dup_iou, const double* job_dup_frac, int32_t n_classes,
                         int32_t* out_keep, int32_t* out_by, int32_t* out_match, int32_t* out_row_keep, int64_t* out_dropped) {
    const wt::DedupInput in = {{n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, score,
                                category, local, n_traj, n_classes}, n_jobs, job_result, job_min_frames, job_dup_iou, job_dup_frac};
    int64_t max_traj = 0, n_traj_total = 0;
    WT_TRY(wt::check_dedup_layout(in, &max_traj, &n_traj_total));
    const size_t nr = (size_t)set_row_offsets[r_sets], J = (size_t)n_jobs, nt = (size_t)n_traj_total, jc = J * (size_t)n_classes;
    if ((J * nt && !(out_keep && out_by && out_match)) || (J * nr && !out_row_keep) || (J * (size_t)n_streams && !out_dropped)) {
        wt::set_error("wt_dedup_tracks_host: bad argument");
        return WT_ERR_INVALID;
    }
    wt::DevBuf jm, ji, jf;
    WT_TRY(wt::check_track_args("wt_dedup_tracks_host", n_frames, n_streams, r_sets, (int64_t)nr, n_traj_total, max_traj, n_jobs, n_classes, true,
                                wt::grid_fits(n_jobs, n_streams) && wt::grid_fits(r_sets, n_streams), kGridText, (int)n_jobs, (int)r_sets, (int)n_streams));
    return dup::run_host<Layout>("wt_dedup_tracks_host", "dedup", dedup_match_kernel, in, n_jobs, job_result, n_traj_total, max_traj, [&](Layout* L) {
        WT_TRY(jm.upload(job_min_frames, 4 * jc)); WT_TRY(ji.upload(job_dup_iou, 8 * jc)); WT_TRY(jf.upload(job_dup_frac, 8 * jc));
        L->job_min_frames = jm.as<int32_t>(); L->job_dup_iou = ji.as<double>(); L->job_dup_frac = jf.as<double>();
        return (int)WT_OK;
    }, out_keep, out_by, out_match, out_row_keep, out_dropped);
}

}  // extern "C"
