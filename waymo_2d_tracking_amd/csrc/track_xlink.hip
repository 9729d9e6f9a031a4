// Cross-class track linking on gfx950 (include/waymotrack.h, "Cross-class track linking"; DESIGN.md section 31 has the
// definition): the repair of class flicker.  A trajectory that ends (tail) is linked to one of the same stream that begins up to
// max_link[ci][cj] slots later (head) - ci, cj the classes of the two, the pair switched on by a symmetric table - when the tail's
// extrapolated box overlaps the head's first box; the linked pieces take the id of the earliest one and the class the chain's
// rows vote for.  R tracking results come in once; J jobs each name a result and their parameters.  No row is added, removed or
// moved.
//
// The summary (with the row count per trajectory), the match in rounds, the roots and the launches are those of
// link_match_device.h, shared with track_stitch.hip; this unit gives them the rules of section 31 as a compile-time policy - a
// tail's head range is bounded by the largest max_link of its class's row of the table, and the pair's own gap and threshold are
// tested per head.  After the roots are resolved one lane per root walks its chain - once for the mask of the classes in it, once
// per class of the mask for that class's rows, once to write the winner to every member - and the wavefront labels its rows with
// root and class.
// Compile with -ffp-contract=off: the extrapolation is x + ((x - xp) / (e - p)) * n with every operation rounded on its own, and
// iou_dd is the IoU the metrics use.
#include "eval_device.h"
#include "tracks_device.h"
#include "link_match_device.h"
#include "xlink_host.h"

using namespace wtdev;
using link::kLdsTraj;

namespace {

struct Layout : link::Layout {                // device pointers
    const int32_t *job_pair_max_link, *job_class_prio;
    const double* job_pair_link_iou;
};

struct Outputs : link::Outputs {
    int32_t* cls;                             // [J * n_traj_total]
    int32_t* row_category;                    // [J * n_rows]
    int64_t* relabelled;                      // [J * n_streams]
    // no link, no root, no class
    __device__ __forceinline__ void init(long long i, long long n_traj, long long n_row) const {
        link::Outputs::init(i, n_traj, n_row);
        if (i < n_traj) cls[i] = -1;
        if (i < n_row) row_category[i] = -1;
    }
};

// Section 31: any pair of classes the job's tables switch on, with the pair's gap and threshold.
struct XLinkPolicy {
    static constexpr bool kRowCounts = true, kRounds = true;
    const int32_t* max_link;                  // the job's tables, [n_classes][n_classes]
    const double* link_iou;
    int C;
    struct Row {                              // the tail's class's row of the tables, [n_classes]
        const int32_t* max_link_row;
        const double* thr_row;
        int C;
        __device__ __forceinline__ int reach() const {
            int r = 0;
            for (int k = 0; k < C; ++k) r = max_link_row[k] > r ? max_link_row[k] : r;
            return r;
        }
        __device__ __forceinline__ bool meets(int cj) const { return cj >= 1 && cj <= C; }
        __device__ __forceinline__ int max_link(int cj) const { return max_link_row[cj - 1]; }
        __device__ __forceinline__ double threshold(int cj) const { return thr_row[cj - 1]; }
    };
    __device__ __forceinline__ static XLinkPolicy make(const Layout& L, int job) {
        const size_t o = (size_t)job * L.n_classes * L.n_classes;
        return {L.job_pair_max_link + o, L.job_pair_link_iou + o, L.n_classes};
    }
    __device__ __forceinline__ Row row(int c) const { return {max_link + (size_t)(c - 1) * C, link_iou + (size_t)(c - 1) * C, C}; }
};

__global__ __launch_bounds__(kWave) void xlink_match_kernel(Layout L, Boxes B, link::Workspace ws, Outputs O, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const size_t p = blockIdx.x;
    const link::Matched M = link::match_problem<XLinkPolicy>(L, B, ws, O, status, smem);
    if (!M.ok) {
        if (lane == 0) { O.relabelled[p] = 0; ws.rounds[p] = 0; }
        return;
    }
    const int T = M.q.T, C = L.n_classes;
    const link::Summary S = ws.sum;
    const size_t g0 = (size_t)M.q.t0;
    const int32_t *succ = M.succ, *pred = M.pred;
    const int32_t* prio = L.job_class_prio + (size_t)M.job * C;
    int32_t* chain_cls = M.spare;                                      // the matching is over: its first table holds the chain's class
    int err = M.err;
    // ---- the vote: one lane per root walks its chain; the chains are disjoint, so the lanes never meet in chain_cls ----
    for (int r = lane; r < T; r += kWave) {
        if (pred[r] >= 0) continue;
        const int rc = S.cls[g0 + r];
        unsigned mask = 0u;
        int steps = 0;
        for (int t = r; t >= 0 && steps < T; t = succ[t], ++steps) {
            const int c = S.cls[g0 + t];
            if (c >= 1 && c <= C) mask |= 1u << (c - 1);
        }
        // the class that maximises (rows, prio, is the root's class, -class): ascending classes, replaced only by a strictly better one
        int best_c = rc, best_p = 0, best_root = 0;
        long long best_n = -1;
        for (int c = 1; c <= C; ++c) {
            if (!((mask >> (c - 1)) & 1u)) continue;
            long long n = 0;
            steps = 0;
            for (int t = r; t >= 0 && steps < T; t = succ[t], ++steps)
                if (S.cls[g0 + t] == c) n += S.cnt[g0 + t];
            const int pr = prio[c - 1], is_root = c == rc ? 1 : 0;
            if (n > best_n || (n == best_n && (pr > best_p || (pr == best_p && is_root > best_root)))) { best_c = c; best_n = n; best_p = pr; best_root = is_root; }
        }
        steps = 0;
        for (int t = r; t >= 0 && steps < T; t = succ[t], ++steps) { chain_cls[t] = best_c; O.cls[M.tbase + t] = best_c; }
    }
    wsync();
    // ---- row labels ----
    long long n_rel = 0;
    for (long long d = M.q.rs0 + lane; d < M.end; d += kWave) {
        const int t = L.local[d];
        if (t < 0 || t >= T) { err = kErrCapacity; continue; }
        const int c = chain_cls[t];
        O.row_root[M.lbase + d] = M.root[t];
        O.row_category[M.lbase + d] = c;
        n_rel += c != L.category[d];
    }
    for (int o = 32; o > 0; o >>= 1) n_rel += __shfl_xor(n_rel, o, kWave);
    if (__ballot(err != 0) != 0ull && lane == 0) atomicMax(status, kErrCapacity);
    if (lane == 0) { O.links[p] = M.n_links; O.relabelled[p] = n_rel; ws.rounds[p] = M.rounds; }
}

}  // namespace

extern "C" {

void wt_xlink_tracks_limits(int32_t* lds_trajectories) {
    if (lds_trajectories) *lds_trajectories = kLdsTraj;
}

size_t wt_xlink_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj) {
    return link::workspace_bytes<XLinkPolicy>(n_jobs, n_streams, n_rows, n_traj_total, max_traj);
}

int wt_xlink_tracks_rounds(const void* workspace, int32_t n_jobs, int32_t n_streams, int32_t* out_rounds) {
    return link::read_rounds("wt_xlink_tracks_rounds", workspace, n_jobs, n_streams, out_rounds);
}

int wt_xlink_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                        int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                        const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                        const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                        int32_t n_jobs, const int32_t* job_result, const int32_t* job_pair_max_link, const double* job_pair_link_iou,
                        const int32_t* job_class_prio, const int32_t* job_motion, int32_t n_classes,
                        int32_t* out_pred, int32_t* out_root, double* out_affinity, int32_t* out_cls, int32_t* out_row_root,
                        int32_t* out_row_category, int64_t* out_links, int64_t* out_relabelled,
                        int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    WT_TRY(wt::check_track_args("wt_xlink_tracks_dev", n_frames, n_streams, r_sets, n_rows, n_traj_total, max_traj, n_jobs, n_classes,
                                stream_frame_offsets && set_row_offsets && frame_row_offsets && x && y && w && h && category && local && traj_offsets &&
                                    job_result && job_pair_max_link && job_pair_link_iou && job_class_prio && job_motion && out_pred && out_root &&
                                    out_affinity && out_cls && out_row_root && out_row_category && out_links && out_relabelled && status_dev,
                                wt::grid_fits(n_jobs, n_streams) && wt::grid_fits(r_sets, n_streams), link::kGridText, (int)n_jobs, (int)r_sets, (int)n_streams));
    if (n_classes > wt::kXLinkMaxClasses) { wt::set_error("wt_xlink_tracks_dev: %d classes, at most %d", (int)n_classes, (int)wt::kXLinkMaxClasses); return WT_ERR_INVALID; }
    const wt::TrackSet dev = {n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, nullptr,
                              category, local, nullptr, n_classes};
    Layout L;
    wt::fill_track_layout(&L, dev, n_rows, traj_offsets, n_traj_total, max_traj, n_jobs, job_result, kLdsTraj);
    L.job_pair_max_link = job_pair_max_link; L.job_pair_link_iou = job_pair_link_iou; L.job_class_prio = job_class_prio; L.job_motion = job_motion;
    const Boxes B = {x, y, w, h};
    const Outputs O = {{out_pred, out_root, out_affinity, out_row_root, out_links}, out_cls, out_row_category, out_relabelled};
    return link::launch<XLinkPolicy>("wt_xlink_tracks_dev", xlink_match_kernel, L, B, O, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_xlink_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                         const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const int32_t* job_pair_max_link,
                         const double* job_pair_link_iou, const int32_t* job_class_prio, const int32_t* job_motion, int32_t n_classes,
                         int32_t* out_pred, int32_t* out_root, double* out_affinity, int32_t* out_cls, int32_t* out_row_root,
                         int32_t* out_row_category, int64_t* out_links, int64_t* out_relabelled) {
    const wt::XLinkInput in = {{n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, nullptr,
                                category, local, n_traj, n_classes}, n_jobs, job_result, job_pair_max_link, job_pair_link_iou, job_class_prio, job_motion};
    int64_t max_traj = 0, n_traj_total = 0;
    WT_TRY(wt::check_xlink_layout(in, &max_traj, &n_traj_total));
    const size_t nr = (size_t)set_row_offsets[r_sets], J = (size_t)n_jobs, nt = (size_t)n_traj_total, C = (size_t)n_classes;
    const size_t P = J * (size_t)n_streams;
    wt::DevBuf jl, ji, jp, jm, oc, orc, orl;
    return link::run_host<XLinkPolicy, Layout, Outputs>("wt_xlink_tracks_host", "xlink", xlink_match_kernel, in, n_jobs, job_result, n_traj_total, max_traj,
                                                        [&](Layout* L, Outputs* O) {
        WT_TRY(jl.upload(job_pair_max_link, 4 * J * C * C)); WT_TRY(ji.upload(job_pair_link_iou, 8 * J * C * C));
        WT_TRY(jp.upload(job_class_prio, 4 * J * C)); WT_TRY(jm.upload(job_motion, 4 * J));
        L->job_pair_max_link = jl.as<int32_t>(); L->job_pair_link_iou = ji.as<double>(); L->job_class_prio = jp.as<int32_t>(); L->job_motion = jm.as<int32_t>();
        WT_TRY(oc.alloc(4 * J * nt)); WT_TRY(orc.alloc(4 * J * nr)); WT_TRY(orl.alloc(8 * P));
        O->cls = oc.as<int32_t>(); O->row_category = orc.as<int32_t>(); O->relabelled = orl.as<int64_t>();
        return (int)WT_OK;
    }, {out_pred, out_root, out_affinity, out_row_root, out_links},
    {{out_cls, &oc, 4 * J * nt}, {out_row_category, &orc, 4 * J * nr}, {out_relabelled, &orl, 8 * P}});
}

}  // extern "C"
