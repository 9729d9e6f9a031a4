// Suppression of duplicate tracks across classes on gfx950 (include/waymotrack.h, "Cross-class track suppression"; DESIGN.md
// section 26 has the definition): the detector puts a pedestrian box on the rider of a bicycle beside the cyclist box, nothing
// before this pass compares boxes of two classes, and both become tracks.  Two trajectories of one stream whose class pair a job
// switches on are the same object when their boxes reach the pair's overlap - IoU or intersection over the smaller area - in at
// least frames slots and in at least frac of the WEAKER one's rows; the trajectories are walked from strongest (highest class
// priority, then most rows, then highest score sum, then lowest index) to weakest and one is suppressed when a stronger KEPT one
// is the same object.  Rows are only selected: no float is produced.
// The summary, the match in rounds and the launches are those of dup_match_device.h, shared with track_dedup.hip; this unit gives
// them the relation and the order above as the policy.
// Compile with -ffp-contract=off: the measures are built from the terms of iou_dd, and frac * n_weak is one multiplication.
#include "eval_device.h"
#include "tracks_device.h"
#include "dup_match_device.h"
#include "xclass_host.h"

using namespace wtdev;
using dup::kLdsTraj;

namespace {

struct Layout : dup::Layout {                 // device pointers
    const int32_t *job_pair_frames, *job_class_prio, *job_measure;
    const double *job_pair_overlap, *job_pair_frac;
};

constexpr double kLargestDouble = 1.7976931348623157e308;

// Intersection over the smaller area, from the terms of iou_dd in its operation order.  It counts only between two boxes of
// positive, finite area - comparisons that a NaN fails; otherwise NaN, which reaches no threshold.
__device__ __forceinline__ double iomin_dd(const double a[4], const double b[4]) {
    const double xx1 = (a[0] > b[0]) ? a[0] : b[0];
    const double yy1 = (a[1] > b[1]) ? a[1] : b[1];
    const double xx2 = (a[2] < b[2]) ? a[2] : b[2];
    const double yy2 = (a[3] < b[3]) ? a[3] : b[3];
    double w = xx2 - xx1; if (!(w > 0.)) w = 0.;
    double h = yy2 - yy1; if (!(h > 0.)) h = 0.;
    const double wh = w * h;
    const double area_a = (a[2] - a[0]) * (a[3] - a[1]);
    const double area_b = (b[2] - b[0]) * (b[3] - b[1]);
    if (!(area_a > 0. && area_b > 0. && area_a <= kLargestDouble && area_b <= kLargestDouble)) return __builtin_nan("");
    const double lo = area_a < area_b ? area_a : area_b;
    return wh / lo;
}

struct XClassPolicy {
    const int32_t* pair_frames;               // [C][C] of the job; read at (lower class, higher class) only
    const double *pair_overlap, *pair_frac;
    const int32_t* prio;                      // [C]
    const int32_t *n, *cls;
    const double* ssum;
    int C, iomin;
    unsigned live;                            // bit c - 1: class c is in some pair that is on
    __device__ __forceinline__ static XClassPolicy make(const Layout& L, int job, const int32_t* n, const double* ssum, const int32_t* cls) {
        const int C = L.n_classes <= wt::kXClassMaxClasses ? L.n_classes : 0;          // more classes than the mask holds: nothing is live
        const size_t o = (size_t)job * L.n_classes * L.n_classes;
        XClassPolicy P = {L.job_pair_frames + o, L.job_pair_overlap + o, L.job_pair_frac + o, L.job_class_prio + (size_t)job * L.n_classes,
                          n, cls, ssum, L.n_classes, L.job_measure[job] == 1 ? 1 : 0, 0u};
        for (int a = 0; a < C; ++a)
            for (int b = a; b < C; ++b)
                if (P.pair_frames[a * C + b] > 0) P.live |= (1u << a) | (1u << b);
        return P;
    }
    __device__ __forceinline__ int at(int ca, int cb) const { return ca < cb ? (ca - 1) * C + (cb - 1) : (cb - 1) * C + (ca - 1); }
    __device__ __forceinline__ int live_class(int c) const { return c >= 1 && c <= wt::kXClassMaxClasses && ((live >> (c - 1)) & 1u) ? c : 0; }
    __device__ __forceinline__ bool pair_live(int ca, int cb) const { return pair_frames[at(ca, cb)] > 0; }
    __device__ __forceinline__ double threshold(int ca, int cb) const { return pair_overlap[at(ca, cb)]; }
    __device__ __forceinline__ int frames(int ca, int cb) const { return pair_frames[at(ca, cb)]; }
    __device__ __forceinline__ double measure(const double a[4], const double b[4]) const { return iomin ? iomin_dd(a, b) : iou_dd(a, b); }
    __device__ __forceinline__ int prio_of(int t) const {
        const int c = cls[t];
        return c >= 1 && c <= C ? prio[c - 1] : 0;
    }
    // t is stronger than u: the higher class priority, then more rows, then the higher score sum, then the lower index
    __device__ __forceinline__ bool stronger(int t, int u) const {
        const int pt = prio_of(t), pu = prio_of(u);
        if (pt != pu) return pt > pu;
        const int nt = n[t], nu = n[u];
        if (nt != nu) return nt > nu;
        const double st = ssum[t], su = ssum[u];
        if (st > su) return true;
        if (st < su) return false;
        return t < u;
    }
    // of the weaker one's rows, not of the shorter one's
    __device__ __forceinline__ double need(int ca, int cb, int, int weak) const { return pair_frac[at(ca, cb)] * (double)n[weak]; }
};

__global__ __launch_bounds__(kWave) void xclass_match_kernel(Layout L, Boxes B, dup::Workspace ws, dup::Outputs O, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    dup::match_problem<XClassPolicy>(L, B, ws, O, status, smem);
}

constexpr const char* kGridText = "%s: %d jobs, %d results x %d streams in one call";

}  // namespace

extern "C" {

void wt_xclass_tracks_limits(int32_t* lds_trajectories) {
    if (lds_trajectories) *lds_trajectories = kLdsTraj;
}

size_t wt_xclass_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj) {
    return dup::workspace_bytes(n_jobs, n_streams, n_rows, n_traj_total, max_traj);
}

int wt_xclass_tracks_rounds(const void* workspace, int32_t n_jobs, int32_t n_streams, int32_t* out_rounds) {
    return dup::read_rounds("wt_xclass_tracks_rounds", workspace, n_jobs, n_streams, out_rounds);
}

int wt_xclass_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const double* score,
                         const int32_t* category, const int32_t* local,
                         const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                         int32_t n_jobs, const int32_t* job_result, const int32_t* job_pair_frames,
                         const double* job_pair_overlap, const double* job_pair_frac, const int32_t* job_class_prio,
                         const int32_t* job_measure, int32_t n_classes,
                         int32_t* out_keep, int32_t* out_by, int32_t* out_match, int32_t* out_row_keep, int64_t* out_dropped,
                         int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    WT_TRY(wt::check_track_args("wt_xclass_tracks_dev", n_frames, n_streams, r_sets, n_rows, n_traj_total, max_traj, n_jobs, n_classes,
                                stream_frame_offsets && set_row_offsets && frame_row_offsets && x && y && w && h && score && category && local &&
                                    traj_offsets && job_result && job_pair_frames && job_pair_overlap && job_pair_frac && job_class_prio &&
                                    job_measure && out_keep && out_by && out_match && out_row_keep && out_dropped && status_dev &&
                                    n_classes <= wt::kXClassMaxClasses,
                                wt::grid_fits(n_jobs, n_streams) && wt::grid_fits(r_sets, n_streams), kGridText, (int)n_jobs, (int)r_sets, (int)n_streams));
    const wt::TrackSet dev = {n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, score,
                              category, local, nullptr, n_classes};
    Layout L;
    wt::fill_track_layout(&L, dev, n_rows, traj_offsets, n_traj_total, max_traj, n_jobs, job_result, kLdsTraj);
    L.score = score; L.job_pair_frames = job_pair_frames; L.job_pair_overlap = job_pair_overlap; L.job_pair_frac = job_pair_frac;
    L.job_class_prio = job_class_prio; L.job_measure = job_measure;
    const Boxes B = {x, y, w, h};
    const dup::Outputs O = {out_keep, out_by, out_match, out_row_keep, out_dropped};
    return dup::launch("wt_xclass_tracks_dev", xclass_match_kernel, L, B, O, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_xclass_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                          int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                          const double* x, const double* y, const double* w, const double* h, const double* score,
                          const int32_t* category, const int32_t* local,
                          const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const int32_t* job_pair_frames,
                          const double* job_pair_overlap, const double* job_pair_frac, const int32_t* job_class_prio,
                          const int32_t* job_measure, int32_t n_classes,
                          int32_t* out_keep, int32_t* out_by, int32_t* out_match, int32_t* out_row_keep, int64_t* out_dropped) {
    const wt::XClassInput in = {{n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, score,
                                 category, local, n_traj, n_classes}, n_jobs, job_result, job_pair_frames, job_pair_overlap, job_pair_frac,
                                job_class_prio, job_measure};
    int64_t max_traj = 0, n_traj_total = 0;
    WT_TRY(wt::check_xclass_layout(in, &max_traj, &n_traj_total));
    const size_t nr = (size_t)set_row_offsets[r_sets], J = (size_t)n_jobs, nt = (size_t)n_traj_total, jc = J * (size_t)n_classes, jcc = jc * (size_t)n_classes;
    if ((J * nt && !(out_keep && out_by && out_match)) || (J * nr && !out_row_keep) || (J * (size_t)n_streams && !out_dropped)) {
        wt::set_error("wt_xclass_tracks_host: bad argument");
        return WT_ERR_INVALID;
    }
    WT_TRY(wt::check_track_args("wt_xclass_tracks_host", n_frames, n_streams, r_sets, (int64_t)nr, n_traj_total, max_traj, n_jobs, n_classes, true,
                                wt::grid_fits(n_jobs, n_streams) && wt::grid_fits(r_sets, n_streams), kGridText, (int)n_jobs, (int)r_sets, (int)n_streams));
    wt::DevBuf jf, jo, jq, jp, jm;
    return dup::run_host<Layout>("wt_xclass_tracks_host", "xclass", xclass_match_kernel, in, n_jobs, job_result, n_traj_total, max_traj, [&](Layout* L) {
        WT_TRY(jf.upload(job_pair_frames, 4 * jcc)); WT_TRY(jo.upload(job_pair_overlap, 8 * jcc)); WT_TRY(jq.upload(job_pair_frac, 8 * jcc));
        WT_TRY(jp.upload(job_class_prio, 4 * jc)); WT_TRY(jm.upload(job_measure, 4 * J));
        L->job_pair_frames = jf.as<int32_t>(); L->job_pair_overlap = jo.as<double>(); L->job_pair_frac = jq.as<double>();
        L->job_class_prio = jp.as<int32_t>(); L->job_measure = jm.as<int32_t>();
        return (int)WT_OK;
    }, out_keep, out_by, out_match, out_row_keep, out_dropped);
}

}  // extern "C"
