// Track smoothing on gfx950 (include/waymotrack.h, "Track smoothing"; DESIGN.md section 22 has the definition): every box of a
// trajectory becomes the weighted mean of itself and of the rows of its trajectory d = 1 .. W slots before AND after it - a distance
// counts only when both sides are there.  R tracking results come in once; J jobs each name a result, a window per class and a
// weight table per class.  No row is added, removed or moved.
//
// Two launches:
//   1. link:  per (result, stream), one 64-lane wavefront walks the slots once, the rows of a slot lane-parallel: per row the
//             distance in rows to the previous and to the next row of its trajectory, its slot and its trajectory's class.  The
//             per-trajectory table (last row, class) lives in LDS up to kLdsTraj trajectories, in the workspace beyond.  Shared by
//             all jobs of the result.
//   2. apply: one lane per (job, row).  The lane walks its trajectory's two chains with two pointers: at distance d a side is
//             there when its pointer's slot is f -/+ d, and the pointer then moves on; it stops when either chain ends.  At most
//             2 W gathers per lane, no tables.
// Compile with -ffp-contract=off: acc = acc + k[d] * (v(f - d) + v(f + d)) and den = den + (k[d] + k[d]), every operation rounded on
// its own.  The weights come from the caller: nothing here evaluates exp.
#include "eval_device.h"
#include "tracks_device.h"
#include "smooth_host.h"

using namespace wtdev;

namespace {

constexpr int kLdsTraj = 1024;                // trajectories of one (result, stream) up to which the link table stays in LDS
constexpr int kApplyBlock = 256;

struct Layout : TrackLayout {                 // device pointers; lds_traj is not used: the link table is a static one
    long long n_out;
    int n_weights;
    const int64_t* job_row_offsets;
    const int32_t* job_window;
    const double* job_weights;
};

struct Links {                                // [n_rows] each; zeroed before the link walk: a row no slot holds has no chain and class 0
    int32_t *back, *fwd;                      // rows from this one to the previous / next row of its trajectory; 0 = none
    int32_t *slot, *cls;                      // the row's slot relative to its stream's first; its trajectory's class
};

struct Workspace {
    Links ln;
    int32_t *last, *tcls;                     // [n_traj_total] the link table of the (result, stream)s above kLdsTraj
    size_t link_bytes, bytes;
};

Workspace carve(void* base, size_t n_rows, size_t n_traj_total, size_t max_traj) {
    wt::Carver cv(base);
    Workspace w;
    const size_t big = max_traj > (size_t)kLdsTraj ? n_traj_total : 0;
    w.ln.back = cv.take<int32_t>(n_rows + 1);
    w.ln.fwd = cv.take<int32_t>(n_rows + 1);
    w.ln.slot = cv.take<int32_t>(n_rows + 1);
    w.ln.cls = cv.take<int32_t>(n_rows + 1);
    w.link_bytes = cv.off;
    w.last = cv.take<int32_t>(big + 1);
    w.tcls = cv.take<int32_t>(big + 1);
    w.bytes = cv.off;
    return w;
}

__global__ __launch_bounds__(kWave) void smooth_link_kernel(Layout L, Workspace ws, int* __restrict__ status) {
    __shared__ int32_t lds_last[kLdsTraj], lds_cls[kLdsTraj];
    const int lane = threadIdx.x & 63;
    const int r = (int)(blockIdx.x / (unsigned)L.n_streams), s = (int)(blockIdx.x % (unsigned)L.n_streams);
    const Span q = span_of(L, r, s);
    if (!q.ok) {
        if (lane == 0) atomicMax(status, kErrCapacity);
        return;
    }
    const int T = q.T;
    const bool in_lds = T <= kLdsTraj;
    int32_t* last = in_lds ? lds_last : ws.last + q.t0;                 // the trajectory's latest row, relative to rs0; -1 none yet
    int32_t* tcls = in_lds ? lds_cls : ws.tcls + q.t0;
    for (int t = lane; t < T; t += kWave) { last[t] = -1; tcls[t] = 0; }
    wsync();
    int err = 0;
    for_stream_rows(q, L.local, &err, [&](long long d, int t, int fo) {
        const int row = (int)(d - q.rs0), prev = last[t];
        if (prev < 0) {
            tcls[t] = L.category[d];
        } else {
            ws.ln.back[d] = row - prev;
            ws.ln.fwd[q.rs0 + prev] = row - prev;
        }
        ws.ln.slot[d] = fo;
        ws.ln.cls[d] = tcls[t];
        last[t] = row;
    });
    if (__ballot(err != 0) != 0ull && lane == 0) atomicMax(status, kErrCapacity);
}

// first j in [0, n] with offsets[j] > v
__device__ __forceinline__ int upper_bound_offset(const int64_t* __restrict__ offsets, int n, long long v) {
    int lo = 0, hi = n + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kApplyBlock) void smooth_apply_kernel(Layout L, Boxes B, Links ln, double* __restrict__ out_bbox,
                                                                   int32_t* __restrict__ out_pairs, int* __restrict__ status) {
    const long long o = (long long)blockIdx.x * kApplyBlock + threadIdx.x;
    if (o >= L.n_out) return;
    const int j = upper_bound_offset(L.job_row_offsets, L.n_jobs, o) - 1;
    if (j < 0 || j >= L.n_jobs) { atomicMax(status, kErrCapacity); return; }        // offsets that do not cover the output rows
    const int r = L.job_result[j];
    if (r < 0 || r >= L.r_sets) { atomicMax(status, kErrCapacity); return; }
    const long long base = L.set_row_offsets[r], rend = L.set_row_offsets[r + 1];
    const long long d = base + (o - L.job_row_offsets[j]);
    if (base < 0 || rend > L.n_rows || d < base || d >= rend || L.job_row_offsets[j + 1] - L.job_row_offsets[j] != rend - base) {
        atomicMax(status, kErrCapacity);
        return;
    }
    const double* col[4] = {B.x, B.y, B.w, B.h};
    double acc[4];
    for (int v = 0; v < 4; ++v) acc[v] = col[v][d];
    const int c = ln.cls[d];
    int W = c >= 1 && c <= L.n_classes ? L.job_window[(size_t)j * L.n_classes + (c - 1)] : 0;
    if (W < 0 || W > WT_SMOOTH_MAX_WINDOW || W >= L.n_weights) { atomicMax(status, kErrCapacity); W = 0; }
    int pairs = 0;
    if (W > 0) {
        const double* __restrict__ k = L.job_weights + ((size_t)j * L.n_classes + (c - 1)) * (size_t)L.n_weights;
        const int f = ln.slot[d];
        const double k0 = k[0];
        double in[4], den = k0;
        for (int v = 0; v < 4; ++v) { in[v] = acc[v]; acc[v] = k0 * in[v]; }
        long long pb = d, pf = d;                                           // the rows whose back / fwd link leads to the next candidate
        for (int dist = 1; dist <= W; ++dist) {
            const int sb = ln.back[pb], sf = ln.fwd[pf];
            if (sb <= 0 || sf <= 0) break;                                  // a chain has ended: no pair beyond
            const long long cb = pb - sb, cf = pf + sf;
            if (cb < base || cf >= rend) { atomicMax(status, kErrCapacity); break; }
            const bool has_b = ln.slot[cb] == f - dist, has_f = ln.slot[cf] == f + dist;
            if (has_b && has_f) {
                const double kd = k[dist];
                for (int v = 0; v < 4; ++v) {
                    const double pair = col[v][cb] + col[v][cf];
                    const double term = kd * pair;
                    acc[v] = acc[v] + term;
                }
                const double two = kd + kd;
                den = den + two;
                ++pairs;
            }
            if (has_b) pb = cb;
            if (has_f) pf = cf;
        }
        for (int v = 0; v < 4; ++v) acc[v] = pairs > 0 ? acc[v] / den : in[v];
    }
    for (int v = 0; v < 4; ++v) out_bbox[o * 4 + v] = acc[v];
    out_pairs[o] = pairs;
}

constexpr const char* kGridText = "%s: %d results x %d streams, %lld output rows in one call";

bool grid_ok(int32_t r_sets, int32_t n_streams, int64_t n_out) {
    return wt::grid_fits(r_sets, n_streams) && (uint64_t)n_out <= 0x7fffffffull * kApplyBlock;
}

int launch(const char* entry, const Layout& L, const Boxes& B, double* out_bbox, int32_t* out_pairs, int32_t* status_dev, void* workspace,
           size_t workspace_bytes, hipStream_t stream) {
    WT_TRY(wt::ensure_device());
    const Workspace ws = carve(wt::align_ptr(workspace), (size_t)L.n_rows, (size_t)L.n_traj_total, (size_t)L.max_traj);
    WT_TRY(wt::check_workspace_fits(entry, workspace, workspace_bytes, ws.bytes, WT_ERR_CAPACITY));
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    WT_HIP(hipMemsetAsync(ws.ln.back, 0, ws.link_bytes, stream));
    const size_t RS = (size_t)L.r_sets * (size_t)L.n_streams;
    if (RS && L.n_jobs) hipLaunchKernelGGL(smooth_link_kernel, dim3((unsigned)RS), dim3(kWave), 0, stream, L, ws, (int*)status_dev);
    if (L.n_out && L.n_jobs)
        hipLaunchKernelGGL(smooth_apply_kernel, dim3((unsigned)((L.n_out + kApplyBlock - 1) / kApplyBlock)), dim3(kApplyBlock), 0, stream, L, B, ws.ln,
                           out_bbox, out_pairs, (int*)status_dev);
    WT_HIP(hipGetLastError());
    return WT_OK;
}

}  // namespace

extern "C" {

void wt_smooth_tracks_limits(int32_t* lds_trajectories) {
    if (lds_trajectories) *lds_trajectories = kLdsTraj;
}

size_t wt_smooth_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj) {
    if (n_jobs < 0 || n_streams < 0 || n_rows < 0 || n_traj_total < 0 || max_traj < 0) return 0;
    return carve(nullptr, (size_t)n_rows, (size_t)n_traj_total, (size_t)max_traj).bytes + 256;
}

int wt_smooth_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                         const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                         int32_t n_jobs, const int32_t* job_result, const int32_t* job_window, const double* job_weights,
                         int32_t n_weights, int32_t n_classes, const int64_t* job_row_offsets, int64_t n_out_rows,
                         double* out_bbox, int32_t* out_pairs,
                         int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    WT_TRY(wt::check_track_args("wt_smooth_tracks_dev", n_frames, n_streams, r_sets, n_rows, n_traj_total, max_traj, n_jobs, n_classes,
                                n_weights >= 1 && n_out_rows >= 0 && stream_frame_offsets && set_row_offsets && frame_row_offsets && x && y && w && h &&
                                    category && local && traj_offsets && job_result && job_window && job_weights && job_row_offsets && out_bbox &&
                                    out_pairs && status_dev,
                                grid_ok(r_sets, n_streams, n_out_rows), kGridText, (int)r_sets, (int)n_streams, (long long)n_out_rows));
    const wt::TrackSet dev = {n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, nullptr,
                              category, local, nullptr, n_classes};
    Layout L;
    wt::fill_track_layout(&L, dev, n_rows, traj_offsets, n_traj_total, max_traj, n_jobs, job_result, 0);
    L.n_out = n_out_rows; L.n_weights = n_weights; L.job_row_offsets = job_row_offsets; L.job_window = job_window; L.job_weights = job_weights;
    const Boxes B = {x, y, w, h};
    return launch("wt_smooth_tracks_dev", L, B, out_bbox, out_pairs, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_smooth_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                          int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                          const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                          const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const int32_t* job_window,
                          const double* job_weights, int32_t n_weights, int32_t n_classes,
                          double* out_bbox, int32_t* out_pairs) {
    const wt::SmoothInput in = {{n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, nullptr,
                                 category, local, n_traj, n_classes}, n_jobs, job_result, job_window, job_weights, n_weights};
    int64_t max_traj = 0, n_traj_total = 0;
    WT_TRY(wt::check_smooth_layout(in, &max_traj, &n_traj_total));
    const size_t nr = (size_t)set_row_offsets[r_sets], J = (size_t)n_jobs;
    std::vector<int64_t> job_rows(J + 1, 0);
    for (size_t j = 0; j < J; ++j) job_rows[j + 1] = job_rows[j] + (set_row_offsets[job_result[j] + 1] - set_row_offsets[job_result[j]]);
    const size_t no = (size_t)job_rows[J];
    if (no && !(out_bbox && out_pairs)) {
        wt::set_error("wt_smooth_tracks_host: bad argument");
        return WT_ERR_INVALID;
    }
    WT_TRY(wt::check_track_args("wt_smooth_tracks_host", n_frames, n_streams, r_sets, (int64_t)nr, n_traj_total, max_traj, n_jobs, n_classes, true,
                                grid_ok(r_sets, n_streams, (int64_t)no), kGridText, (int)r_sets, (int)n_streams, (long long)no));
    WT_TRY(wt::ensure_device());
    wt::StagedTrackSet st;
    wt::DevBuf jw, jk, jo, ob, op, dws;
    WT_TRY(st.upload(in, n_jobs, job_result));
    WT_TRY(jw.upload(job_window, 4 * J * (size_t)n_classes));
    WT_TRY(jk.upload(job_weights, 8 * J * (size_t)n_classes * (size_t)n_weights)); WT_TRY(jo.upload(job_rows.data(), 8 * (J + 1)));
    WT_TRY(ob.alloc(32 * no)); WT_TRY(op.alloc(4 * no));
    const size_t wsb = wt_smooth_tracks_workspace(n_jobs, n_streams, (int64_t)nr, n_traj_total, max_traj);
    WT_TRY(dws.alloc(wsb));
    Layout L;
    st.fill(&L, n_traj_total, max_traj, n_jobs, 0);
    L.n_out = (long long)no; L.n_weights = n_weights; L.job_row_offsets = jo.as<int64_t>(); L.job_window = jw.as<int32_t>(); L.job_weights = jk.as<double>();
    const Boxes B = {st.dev.x, st.dev.y, st.dev.w, st.dev.h};
    WT_TRY(launch("wt_smooth_tracks_host", L, B, ob.as<double>(), op.as<int32_t>(), st.status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(st.finish("smooth", "counts, offsets or windows"));
    if (no) {
        WT_HIP(hipMemcpy(out_bbox, ob.p, 32 * no, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_pairs, op.p, 4 * no, hipMemcpyDeviceToHost));
    }
    return WT_OK;
}

}  // extern "C"
