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
#include "eval_host.h"
#include "smooth_host.h"

using namespace wtdev;

namespace {

constexpr int kLdsTraj = 1024;                // trajectories of one (result, stream) up to which the link table stays in LDS
constexpr int kApplyBlock = 256;

struct Layout {                               // device pointers
    long long n_frames, n_rows, n_traj_total, max_traj, n_out;
    int n_streams, r_sets, n_jobs, n_classes, n_weights;
    const int64_t *stream_frame_offsets, *set_row_offsets, *frame_row_offsets, *traj_offsets, *job_row_offsets;
    const int32_t *category, *local;
    const int32_t *job_result, *job_window;
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
    const size_t rs = (size_t)r * L.n_streams + s;
    const long long t0 = L.traj_offsets[rs], t1 = L.traj_offsets[rs + 1];
    const long long f0 = L.stream_frame_offsets[s], f1 = L.stream_frame_offsets[s + 1];
    const long long base = L.set_row_offsets[r], rend = L.set_row_offsets[r + 1];
    const int64_t* fro = L.frame_row_offsets + (size_t)r * (size_t)(L.n_frames + 1);
    bool ok = t0 >= 0 && t1 >= t0 && t1 - t0 <= L.max_traj && t1 <= L.n_traj_total && f0 >= 0 && f1 >= f0 && f1 <= L.n_frames &&
              f1 - f0 < 0x3fffffffll && base >= 0 && rend >= base && rend <= L.n_rows;
    const long long rs0 = ok && f1 > f0 ? base + fro[f0] : base;
    ok = ok && rs0 >= base && rs0 <= rend;
    if (!ok) {
        if (lane == 0) atomicMax(status, kErrCapacity);
        return;
    }
    const int T = (int)(t1 - t0);
    const bool in_lds = T <= kLdsTraj;
    int32_t* last = in_lds ? lds_last : ws.last + t0;                   // the trajectory's latest row, relative to rs0; -1 none yet
    int32_t* tcls = in_lds ? lds_cls : ws.tcls + t0;
    for (int t = lane; t < T; t += kWave) { last[t] = -1; tcls[t] = 0; }
    wsync();
    int err = 0;
    for (long long f = f0; f < f1; ++f) {
        const long long r0 = base + fro[f], r1 = base + fro[f + 1];
        if (!(r0 >= rs0 && r1 >= r0 && r1 <= rend && r1 - rs0 < 0x7fffffffll)) { err = kErrCapacity; break; }
        for (long long b = r0; b < r1; b += kWave) {                    // local indices are unique inside a slot: lanes never collide
            const long long d = b + lane;
            if (d >= r1) continue;
            const int t = L.local[d];
            if (t < 0 || t >= T) { err = kErrCapacity; continue; }
            const int row = (int)(d - rs0), prev = last[t];
            if (prev < 0) {
                tcls[t] = L.category[d];
            } else {
                ws.ln.back[d] = row - prev;
                ws.ln.fwd[rs0 + prev] = row - prev;
            }
            ws.ln.slot[d] = (int)(f - f0);
            ws.ln.cls[d] = tcls[t];
            last[t] = row;
        }
        wsync();
    }
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

int check_args(const char* entry, int64_t n_frames, int32_t n_streams, int32_t r_sets, int64_t n_rows, int64_t n_traj_total, int64_t max_traj,
               int32_t n_jobs, int32_t n_weights, int32_t n_classes, int64_t n_out, bool others_ok) {
    if (n_frames < 0 || n_streams < 0 || r_sets < 1 || n_rows < 0 || n_traj_total < 0 || max_traj < 0 || n_jobs < 0 || n_weights < 1 || n_classes < 1 ||
        n_out < 0 || !others_ok) {
        wt::set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if ((uint64_t)r_sets * (uint64_t)n_streams > 0x7fffffffull || (uint64_t)n_out > 0x7fffffffull * kApplyBlock) {
        wt::set_error("%s: %d results x %d streams, %lld output rows in one call", entry, (int)r_sets, (int)n_streams, (long long)n_out);
        return WT_ERR_CAPACITY;
    }
    return WT_OK;
}

int launch(const char* entry, const Layout& L, const Boxes& B, double* out_bbox, int32_t* out_pairs, int32_t* status_dev, void* workspace,
           size_t workspace_bytes, hipStream_t stream) {
    WT_TRY(wt::ensure_device());
    const Workspace ws = carve(wt::align_ptr(workspace), (size_t)L.n_rows, (size_t)L.n_traj_total, (size_t)L.max_traj);
    if (!workspace || workspace_bytes < ws.bytes + 256) {
        wt::set_error("%s: workspace too small: need %zu bytes, have %zu", entry, ws.bytes + 256, workspace_bytes);
        return WT_ERR_CAPACITY;
    }
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
    WT_TRY(check_args("wt_smooth_tracks_dev", n_frames, n_streams, r_sets, n_rows, n_traj_total, max_traj, n_jobs, n_weights, n_classes, n_out_rows,
                      stream_frame_offsets && set_row_offsets && frame_row_offsets && x && y && w && h && category && local && traj_offsets &&
                          job_result && job_window && job_weights && job_row_offsets && out_bbox && out_pairs && status_dev));
    Layout L;
    L.n_frames = n_frames; L.n_rows = n_rows; L.n_traj_total = n_traj_total; L.max_traj = max_traj; L.n_out = n_out_rows;
    L.n_streams = n_streams; L.r_sets = r_sets; L.n_jobs = n_jobs; L.n_classes = n_classes; L.n_weights = n_weights;
    L.stream_frame_offsets = stream_frame_offsets; L.set_row_offsets = set_row_offsets; L.frame_row_offsets = frame_row_offsets;
    L.traj_offsets = traj_offsets; L.job_row_offsets = job_row_offsets; L.category = category; L.local = local;
    L.job_result = job_result; L.job_window = job_window; L.job_weights = job_weights;
    const Boxes B = {x, y, w, h};
    return launch("wt_smooth_tracks_dev", L, B, out_bbox, out_pairs, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_smooth_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                          int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                          const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                          const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const int32_t* job_window,
                          const double* job_weights, int32_t n_weights, int32_t n_classes,
                          double* out_bbox, int32_t* out_pairs) {
    const wt::SmoothInput in = {n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h,
                                category, local, n_traj, n_jobs, job_result, job_window, job_weights, n_weights, n_classes};
    int64_t max_traj = 0, n_traj_total = 0;
    WT_TRY(wt::check_smooth_layout(in, &max_traj, &n_traj_total));
    const size_t nr = (size_t)set_row_offsets[r_sets], nf = (size_t)(n_frames + 1), rs = (size_t)r_sets * (size_t)n_streams, J = (size_t)n_jobs;
    std::vector<int64_t> job_rows(J + 1, 0);
    for (size_t j = 0; j < J; ++j) job_rows[j + 1] = job_rows[j] + (set_row_offsets[job_result[j] + 1] - set_row_offsets[job_result[j]]);
    const size_t no = (size_t)job_rows[J];
    if (no && !(out_bbox && out_pairs)) {
        wt::set_error("wt_smooth_tracks_host: bad argument");
        return WT_ERR_INVALID;
    }
    WT_TRY(check_args("wt_smooth_tracks_host", n_frames, n_streams, r_sets, (int64_t)nr, n_traj_total, max_traj, n_jobs, n_weights, n_classes, (int64_t)no, true));
    WT_TRY(wt::ensure_device());
    std::vector<int64_t> traj_offsets(rs + 1, 0);
    for (size_t i = 0; i < rs; ++i) traj_offsets[i + 1] = traj_offsets[i] + n_traj[i];
    wt::DevBuf so, sr, fr, dx, dy, dw, dh, dc, dl, dt, jr, jw, jk, jo, ob, op, status, dws;
    WT_TRY(so.upload(stream_frame_offsets, 8 * (size_t)(n_streams + 1))); WT_TRY(sr.upload(set_row_offsets, 8 * (size_t)(r_sets + 1)));
    WT_TRY(fr.upload(frame_row_offsets, 8 * (size_t)r_sets * nf));
    WT_TRY(dx.upload(x, 8 * nr)); WT_TRY(dy.upload(y, 8 * nr)); WT_TRY(dw.upload(w, 8 * nr)); WT_TRY(dh.upload(h, 8 * nr));
    WT_TRY(dc.upload(category, 4 * nr)); WT_TRY(dl.upload(local, 4 * nr)); WT_TRY(dt.upload(traj_offsets.data(), 8 * (rs + 1)));
    WT_TRY(jr.upload(job_result, 4 * J)); WT_TRY(jw.upload(job_window, 4 * J * (size_t)n_classes));
    WT_TRY(jk.upload(job_weights, 8 * J * (size_t)n_classes * (size_t)n_weights)); WT_TRY(jo.upload(job_rows.data(), 8 * (J + 1)));
    WT_TRY(ob.alloc(32 * no)); WT_TRY(op.alloc(4 * no)); WT_TRY(status.alloc(16));
    const size_t wsb = wt_smooth_tracks_workspace(n_jobs, n_streams, (int64_t)nr, n_traj_total, max_traj);
    WT_TRY(dws.alloc(wsb));
    Layout L;
    L.n_frames = n_frames; L.n_rows = (long long)nr; L.n_traj_total = n_traj_total; L.max_traj = max_traj; L.n_out = (long long)no;
    L.n_streams = n_streams; L.r_sets = r_sets; L.n_jobs = n_jobs; L.n_classes = n_classes; L.n_weights = n_weights;
    L.stream_frame_offsets = so.as<int64_t>(); L.set_row_offsets = sr.as<int64_t>(); L.frame_row_offsets = fr.as<int64_t>();
    L.traj_offsets = dt.as<int64_t>(); L.job_row_offsets = jo.as<int64_t>(); L.category = dc.as<int32_t>(); L.local = dl.as<int32_t>();
    L.job_result = jr.as<int32_t>(); L.job_window = jw.as<int32_t>(); L.job_weights = jk.as<double>();
    const Boxes B = {dx.as<double>(), dy.as<double>(), dw.as<double>(), dh.as<double>()};
    WT_TRY(launch("wt_smooth_tracks_host", L, B, ob.as<double>(), op.as<int32_t>(), status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_HIP(hipDeviceSynchronize());
    int32_t st = 0;
    WT_HIP(hipMemcpy(&st, status.p, sizeof(st), hipMemcpyDeviceToHost));
    if (st) {
        wt::set_error("smooth kernel reported status %d (4 = counts, offsets or windows that do not fit the rows)", (int)st);
        return (int)st;
    }
    if (no) {
        WT_HIP(hipMemcpy(out_bbox, ob.p, 32 * no, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_pairs, op.p, 4 * no, hipMemcpyDeviceToHost));
    }
    return WT_OK;
}

}  // extern "C"
