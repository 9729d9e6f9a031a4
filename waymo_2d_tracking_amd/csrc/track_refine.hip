// Track refinement on gfx950 (include/waymotrack.h, "Track refinement"; DESIGN.md section 20 has the definition): drop the
// trajectories observed in too few frames, fill short gaps by linear interpolation, optionally give every row of a trajectory its
// mean score.  R tracking results come in once; J jobs each name a result and their parameters.
//
// Same shape as the metric kernels: one 64-lane wavefront owns one independent problem = (job j, stream s) and walks the stream's
// frame slots in order, the rows of a slot lane-parallel.  Three launches:
//   1. link:  per trajectory the last row, the observation count, the running score sum and the rows its fillable gaps will add
//             (tables in LDS up to kLdsTraj trajectories, in the workspace beyond); per row the next observation of its
//             trajectory and that observation's slot; per problem the rows it will emit.
//   2. scan:  exclusive scan of those counts = every problem's first output row; per job the totals (job_row_offsets).
//   3. emit:  walk again; per slot the surviving observed rows in input order (compact_wave), then the trajectories that are in a
//             fillable gap at this slot in ascending index (ballot + popcount over chunks of 64 trajectories).
// Compile with -ffp-contract=off: a fill is va + (vb - va) * (j / n) with every operation rounded on its own.
#include "eval_device.h"
#include "tracks_device.h"
#include "refine_host.h"

using namespace wtdev;

namespace {

constexpr int kLdsTraj = 1024;                // trajectories of one (result, stream) up to which the tables stay in LDS

struct Layout : TrackLayout {                 // device pointers; what both walks read
    const int32_t *job_max_gap, *job_min_len;
};

struct Workspace {                            // device pointers carved from one block
    int32_t *nxt_row, *nxt_slot;              // [J * n_rows] per job and row: the trajectory's next observation (row relative to the stream's first) and its slot, -1 none
    int32_t* tgap;                            // [J * n_traj_total] max_gap of the trajectory's class, -1 when the length filter removed it
    double* tmean;                            // [J * n_traj_total] mean observed score
    int64_t *emitted, *out_base;              // [J * n_streams] rows the problem emits, and where they start
    int32_t* tab_i;                           // [J * n_streams * 5 * max_traj] the tables of the problems above kLdsTraj
    double* tab_d;                            // [J * n_streams * max_traj]
    size_t bytes;
};

Workspace carve(void* base, size_t n_jobs, size_t n_streams, size_t n_rows, size_t n_traj_total, size_t max_traj) {
    wt::Carver cv(base);
    Workspace w;
    const size_t P = n_jobs * n_streams, big = max_traj > (size_t)kLdsTraj ? max_traj : 0;
    w.nxt_row = cv.take<int32_t>(n_jobs * n_rows + 1);
    w.nxt_slot = cv.take<int32_t>(n_jobs * n_rows + 1);
    w.tgap = cv.take<int32_t>(n_jobs * n_traj_total + 1);
    w.tmean = cv.take<double>(n_jobs * n_traj_total + 1);
    w.emitted = cv.take<int64_t>(P + 1);
    w.out_base = cv.take<int64_t>(P + 1);
    w.tab_i = cv.take<int32_t>(P * 5 * big + 1);
    w.tab_d = cv.take<double>(P * big + 1);
    w.bytes = cv.off;
    return w;
}

__global__ __launch_bounds__(kWave) void refine_link_kernel(Layout L, const double* __restrict__ score, Workspace ws, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const size_t p = blockIdx.x;
    int j, s;
    decode_job_stream(p, L.n_streams, &j, &s);
    const Span q = span_of(L, L.job_result[j], s);
    if (!q.ok) {
        if (lane == 0) { atomicMax(status, kErrCapacity); ws.emitted[p] = 0; }
        return;
    }
    const int T = q.T, C = L.n_classes;
    const size_t tbase = (size_t)j * (size_t)L.n_traj_total + (size_t)q.t0, lbase = (size_t)j * (size_t)L.n_rows;
    const bool in_lds = T <= L.lds_traj;
    const size_t stride = in_lds ? (size_t)L.lds_traj : (size_t)L.max_traj;
    double* sum = in_lds ? reinterpret_cast<double*>(smem) : ws.tab_d + p * stride;
    int* last = in_lds ? reinterpret_cast<int*>(smem + stride * sizeof(double)) : ws.tab_i + p * 5 * stride;
    int* last_slot = last + stride;
    int* cnt = last + 2 * stride;
    int* fill = last + 3 * stride;
    int* cls = last + 4 * stride;
    for (int t = lane; t < T; t += kWave) { sum[t] = 0.; last[t] = -1; last_slot[t] = -1; cnt[t] = 0; fill[t] = 0; cls[t] = 0; }
    wsync();
    const int32_t* gaps = L.job_max_gap + (size_t)j * C;
    const int32_t* lens = L.job_min_len + (size_t)j * C;
    int err = 0;
    for_stream_rows(q, L.local, &err, [&](long long d, int t, int fo) {
        ws.nxt_row[lbase + d] = -1;
        ws.nxt_slot[lbase + d] = -1;
        const int prev = last[t];
        if (prev < 0) {
            cls[t] = L.category[d];
            sum[t] = score[d];
        } else {
            ws.nxt_row[lbase + q.rs0 + prev] = (int)(d - q.rs0);
            ws.nxt_slot[lbase + q.rs0 + prev] = fo;
            const int c = cls[t], holes = fo - last_slot[t] - 1;
            if (c >= 1 && c <= C && holes >= 1 && holes <= gaps[c - 1]) fill[t] += holes;
            sum[t] = sum[t] + score[d];                               // ascending slot order: part of the definition
        }
        last[t] = (int)(d - q.rs0);
        last_slot[t] = fo;
        cnt[t] += 1;
    });
    long long emit = 0;
    for (int t = lane; t < T; t += kWave) {
        const int c = cls[t], n = cnt[t];
        const bool known = c >= 1 && c <= C;
        if (n > 0 && !known) err = kErrCapacity;
        const bool kept = n > 0 && known && n >= lens[c - 1];
        ws.tgap[tbase + t] = kept ? gaps[c - 1] : -1;
        ws.tmean[tbase + t] = n > 0 ? sum[t] / (double)n : 0.;
        if (kept) emit += (long long)n + fill[t];
    }
    for (int o = 32; o > 0; o >>= 1) emit += __shfl_xor(emit, o, kWave);
    if (__ballot(err != 0) != 0ull && lane == 0) atomicMax(status, kErrCapacity);
    if (lane == 0) ws.emitted[p] = emit;
}

// one wavefront: out_base = exclusive scan of emitted; job_row_offsets[j] = out_base of the job's first problem, [J] = the total
__global__ __launch_bounds__(kWave) void refine_scan_kernel(Workspace ws, int n_jobs, int n_streams, int64_t* __restrict__ job_row_offsets) {
    const int lane = threadIdx.x & 63;
    const long long P = (long long)n_jobs * n_streams;
    long long running = 0;
    for (long long b = 0; b < P; b += kWave) {
        const long long i = b + lane;
        const long long v = i < P ? ws.emitted[i] : 0;
        long long incl = v;
        for (int o = 1; o < kWave; o <<= 1) {
            const long long u = __shfl_up(incl, o, kWave);
            if (lane >= o) incl += u;
        }
        if (i < P) {
            ws.out_base[i] = running + incl - v;
            if (i % n_streams == 0) job_row_offsets[i / n_streams] = running + incl - v;
        }
        running += __shfl(incl, kWave - 1, kWave);
    }
    if (n_streams == 0)
        for (int j = lane; j < n_jobs; j += kWave) job_row_offsets[j] = 0;
    if (lane == 0) job_row_offsets[n_jobs] = running;
}

struct Outputs {
    int64_t* frame;
    int32_t* category;
    double *bbox, *score;
    int32_t* local;
    int64_t *source, *frame_row_offsets;
};

__global__ __launch_bounds__(kWave) void refine_emit_kernel(Layout L, Boxes B, const double* __restrict__ score, const int32_t* __restrict__ job_score_mode,
                                                            Workspace ws, const int64_t* __restrict__ job_row_offsets, long long out_cap, Outputs O,
                                                            int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = lanemask_lt();
    const size_t p = blockIdx.x;
    int j, s;
    decode_job_stream(p, L.n_streams, &j, &s);
    const Span q = span_of(L, L.job_result[j], s);
    if (!q.ok) {
        if (lane == 0) atomicMax(status, kErrCapacity);
        return;
    }
    const int T = q.T;
    const size_t tbase = (size_t)j * (size_t)L.n_traj_total + (size_t)q.t0, lbase = (size_t)j * (size_t)L.n_rows;
    const bool in_lds = T <= L.lds_traj;
    const size_t stride = in_lds ? (size_t)L.lds_traj : (size_t)L.max_traj;
    int* idx = reinterpret_cast<int*>(smem);                           // [kWave] the chunk's surviving rows
    int* cur = in_lds ? idx + kWave : ws.tab_i + p * 5 * stride;       // the trajectory's latest observation (row relative to the stream's first), -1 none yet
    int* cur_slot = cur + stride;
    int* nxt_slot = cur + 2 * stride;                                  // the slot of the observation after it, -1 none
    int* gap = cur + 3 * stride;
    for (int t = lane; t < T; t += kWave) { cur[t] = -1; cur_slot[t] = -1; nxt_slot[t] = -1; gap[t] = ws.tgap[tbase + t]; }
    wsync();
    const bool mean = job_score_mode[j] == 1;
    const long long jb = job_row_offsets[j];
    long long pos = ws.out_base[p];                                    // wave-uniform
    long long pend = pos + ws.emitted[p];                              // nothing is written at or beyond it
    if (pend > out_cap) pend = out_cap;
    int err = 0;
    int64_t* ofro = O.frame_row_offsets + (size_t)j * (size_t)(L.n_frames + 1);
    // Not for_stream_rows: the whole wavefront compacts every chunk, rows with an index outside [0, T) included, advances pos
    // between the chunks, and the gap pass follows the rows of a slot before the next slot begins.
    for (long long f = q.f0; f < q.f1; ++f) {
        const int fo = (int)(f - q.f0);
        long long r0, r1;
        if (!slot_rows(q, f, &r0, &r1)) { err = kErrCapacity; break; }
        if (lane == 0) ofro[f] = pos - jb;
        // ---- the surviving observed rows, in input order ----
        for (long long b = r0; b < r1; b += kWave) {
            const long long hi = (b + kWave < r1) ? b + kWave : r1;
            const int n = compact_wave(b, hi, [=](long long d) { const int t = L.local[d]; return t >= 0 && t < T && gap[t] >= 0; }, idx, kWave);
            wsync();
            if (lane < n && pos + lane < pend) {
                const long long d = b + idx[lane], o = pos + lane;
                O.frame[o] = f;
                O.category[o] = L.category[d];
                O.bbox[o * 4 + 0] = B.x[d]; O.bbox[o * 4 + 1] = B.y[d]; O.bbox[o * 4 + 2] = B.w[d]; O.bbox[o * 4 + 3] = B.h[d];
                O.score[o] = mean ? ws.tmean[tbase + L.local[d]] : score[d];
                O.local[o] = L.local[d];
                O.source[o] = d - q.base;
            }
            pos += n;
            const long long d = b + lane;
            if (d < hi) {
                const int t = L.local[d];
                if (t >= 0 && t < T) { cur[t] = (int)(d - q.rs0); cur_slot[t] = fo; nxt_slot[t] = ws.nxt_slot[lbase + d]; }
            }
            wsync();
        }
        // ---- the trajectories in a fillable gap at this slot, in ascending index ----
        for (int tb = 0; tb < T; tb += kWave) {
            const int t = tb + lane;
            bool in_gap = false;
            int cs = 0, ns = 0;
            if (t < T) {
                cs = cur_slot[t];
                ns = nxt_slot[t];
                const int g = gap[t];
                in_gap = g >= 0 && cs >= 0 && cs < fo && ns > fo && ns - cs - 1 <= g;
            }
            const unsigned long long m = __ballot(in_gap);
            if (in_gap) {
                const long long o = pos + __popcll(m & lt);
                const long long a = q.rs0 + cur[t];
                const long long nb = ws.nxt_row[lbase + a];
                if (o < pend && nb >= 0 && q.rs0 + nb < q.rend) {
                    const long long b = q.rs0 + nb;
                    const double w = (double)(fo - cs) / (double)(ns - cs);
                    O.frame[o] = f;
                    O.category[o] = L.category[a];
                    O.bbox[o * 4 + 0] = B.x[a] + (B.x[b] - B.x[a]) * w;
                    O.bbox[o * 4 + 1] = B.y[a] + (B.y[b] - B.y[a]) * w;
                    O.bbox[o * 4 + 2] = B.w[a] + (B.w[b] - B.w[a]) * w;
                    O.bbox[o * 4 + 3] = B.h[a] + (B.h[b] - B.h[a]) * w;
                    O.score[o] = mean ? ws.tmean[tbase + t] : score[a] + (score[b] - score[a]) * w;
                    O.local[o] = t;
                    O.source[o] = -1 - (b - q.base);
                }
            }
            pos += __popcll(m);
        }
        wsync();
    }
    if (pos != ws.out_base[p] + ws.emitted[p]) err = kErrCapacity;      // the plan and the walk disagree, or out_cap cut it
    if (err && lane == 0) atomicMax(status, err);
    if (s == L.n_streams - 1 && lane == 0) ofro[L.n_frames] = job_row_offsets[j + 1] - jb;
}

constexpr const char* kGridText = "%s: %d jobs x %d streams in one call";

Layout make_layout(const wt::TrackSet& dev, int64_t n_rows, const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj, int32_t n_jobs,
                   const int32_t* job_result, const int32_t* job_max_gap, const int32_t* job_min_len) {
    Layout L;
    wt::fill_track_layout(&L, dev, n_rows, traj_offsets, n_traj_total, max_traj, n_jobs, job_result, kLdsTraj);
    L.job_max_gap = job_max_gap; L.job_min_len = job_min_len;
    return L;
}

int get_workspace(const char* entry, const Layout& L, void* workspace, size_t workspace_bytes, Workspace* ws) {
    *ws = carve(wt::align_ptr(workspace), (size_t)L.n_jobs, (size_t)L.n_streams, (size_t)L.n_rows, (size_t)L.n_traj_total, (size_t)L.max_traj);
    return wt::check_workspace_fits(entry, workspace, workspace_bytes, ws->bytes, WT_ERR_INVALID);
}

int launch_plan(const Layout& L, const double* score, int64_t* job_row_offsets, int32_t* status_dev, void* workspace, size_t workspace_bytes,
                hipStream_t stream) {
    WT_TRY(wt::ensure_device());
    Workspace ws;
    WT_TRY(get_workspace("wt_refine_tracks_plan_dev", L, workspace, workspace_bytes, &ws));
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    const size_t P = (size_t)L.n_jobs * (size_t)L.n_streams;
    if (P) {
        const size_t lds = (size_t)L.lds_traj * (sizeof(double) + 5 * sizeof(int));
        hipLaunchKernelGGL(refine_link_kernel, dim3((unsigned)P), dim3(kWave), lds, stream, L, score, ws, (int*)status_dev);
    }
    hipLaunchKernelGGL(refine_scan_kernel, dim3(1), dim3(kWave), 0, stream, ws, (int)L.n_jobs, (int)L.n_streams, job_row_offsets);
    WT_HIP(hipGetLastError());
    return WT_OK;
}

int launch_emit(const Layout& L, const Boxes& B, const double* score, const int32_t* job_score_mode, const int64_t* job_row_offsets,
                int64_t out_cap, const Outputs& O, int32_t* status_dev, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    WT_TRY(wt::ensure_device());
    Workspace ws;
    WT_TRY(get_workspace("wt_refine_tracks_emit_dev", L, workspace, workspace_bytes, &ws));
    int64_t planned = 0;                                               // the one place the device form waits: the planned size decides whether anything is launched
    WT_HIP(hipMemcpyAsync(&planned, job_row_offsets + L.n_jobs, sizeof(planned), hipMemcpyDeviceToHost, stream));
    WT_HIP(hipStreamSynchronize(stream));
    if (out_cap < planned) {
        wt::set_error("wt_refine_tracks_emit_dev: %lld rows are planned, the output holds %lld", (long long)planned, (long long)out_cap);
        return WT_ERR_CAPACITY;
    }
    const size_t P = (size_t)L.n_jobs * (size_t)L.n_streams;
    if (L.n_jobs) WT_HIP(hipMemsetAsync(O.frame_row_offsets, 0, sizeof(int64_t) * (size_t)L.n_jobs * (size_t)(L.n_frames + 1), stream));
    if (P) {
        const size_t lds = (size_t)kWave * sizeof(int) + (size_t)L.lds_traj * 4 * sizeof(int);
        hipLaunchKernelGGL(refine_emit_kernel, dim3((unsigned)P), dim3(kWave), lds, stream, L, B, score, job_score_mode, ws, job_row_offsets,
                           (long long)out_cap, O, (int*)status_dev);
    }
    WT_HIP(hipGetLastError());
    return WT_OK;
}

}  // namespace

extern "C" {

void wt_refine_tracks_limits(int32_t* lds_trajectories) {
    if (lds_trajectories) *lds_trajectories = kLdsTraj;
}

size_t wt_refine_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj) {
    if (n_jobs < 0 || n_streams < 0 || n_rows < 0 || n_traj_total < 0 || max_traj < 0) return 0;
    return carve(nullptr, (size_t)n_jobs, (size_t)n_streams, (size_t)n_rows, (size_t)n_traj_total, (size_t)(max_traj > 0 ? max_traj : 1)).bytes + 256;
}

int wt_refine_tracks_plan_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                              int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                              const double* score, const int32_t* category, const int32_t* local,
                              const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                              int32_t n_jobs, const int32_t* job_result, const int32_t* job_max_gap, const int32_t* job_min_len, int32_t n_classes,
                              int64_t* job_row_offsets, int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    WT_TRY(wt::check_track_args("wt_refine_tracks_plan_dev", n_frames, n_streams, r_sets, n_rows, n_traj_total, max_traj, n_jobs, n_classes,
                                stream_frame_offsets && set_row_offsets && frame_row_offsets && score && category && local && traj_offsets &&
                                    job_result && job_max_gap && job_min_len && job_row_offsets && status_dev,
                                wt::grid_fits(n_jobs, n_streams), kGridText, (int)n_jobs, (int)n_streams));
    const wt::TrackSet dev = {n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, nullptr, nullptr, nullptr, nullptr,
                              score, category, local, nullptr, n_classes};
    const Layout L = make_layout(dev, n_rows, traj_offsets, n_traj_total, max_traj, n_jobs, job_result, job_max_gap, job_min_len);
    return launch_plan(L, score, job_row_offsets, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_refine_tracks_emit_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                              int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                              const double* x, const double* y, const double* w, const double* h, const double* score,
                              const int32_t* category, const int32_t* local,
                              const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                              int32_t n_jobs, const int32_t* job_result, const int32_t* job_max_gap, const int32_t* job_min_len,
                              const int32_t* job_score_mode, int32_t n_classes, const int64_t* job_row_offsets, int64_t out_cap,
                              int64_t* out_frame, int32_t* out_category, double* out_bbox, double* out_score, int32_t* out_local,
                              int64_t* out_source, int64_t* out_frame_row_offsets,
                              int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    WT_TRY(wt::check_track_args("wt_refine_tracks_emit_dev", n_frames, n_streams, r_sets, n_rows, n_traj_total, max_traj, n_jobs, n_classes,
                                stream_frame_offsets && set_row_offsets && frame_row_offsets && x && y && w && h && score && category && local &&
                                    traj_offsets && job_result && job_max_gap && job_min_len && job_score_mode && job_row_offsets && out_cap >= 0 &&
                                    out_frame && out_category && out_bbox && out_score && out_local && out_source && out_frame_row_offsets && status_dev,
                                wt::grid_fits(n_jobs, n_streams), kGridText, (int)n_jobs, (int)n_streams));
    const wt::TrackSet dev = {n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h,
                              score, category, local, nullptr, n_classes};
    const Layout L = make_layout(dev, n_rows, traj_offsets, n_traj_total, max_traj, n_jobs, job_result, job_max_gap, job_min_len);
    const Boxes B = {x, y, w, h};
    const Outputs O = {out_frame, out_category, out_bbox, out_score, out_local, out_source, out_frame_row_offsets};
    return launch_emit(L, B, score, job_score_mode, job_row_offsets, out_cap, O, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_refine_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                          int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                          const double* x, const double* y, const double* w, const double* h, const double* score,
                          const int32_t* category, const int32_t* local, const int32_t* n_traj,
                          int32_t n_jobs, const int32_t* job_result, const int32_t* job_max_gap, const int32_t* job_min_len,
                          const int32_t* job_score_mode, int32_t n_classes, int64_t out_cap,
                          int64_t* out_frame, int32_t* out_category, double* out_bbox, double* out_score, int32_t* out_local,
                          int64_t* out_source, int64_t* out_frame_row_offsets, int64_t* job_row_offsets) {
    const wt::RefineInput in = {{n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, score,
                                 category, local, n_traj, n_classes}, n_jobs, job_result, job_max_gap, job_min_len, job_score_mode};
    if (!job_row_offsets || out_cap < 0 || (out_cap > 0 && !(out_frame && out_category && out_bbox && out_score && out_local && out_source && out_frame_row_offsets))) {
        wt::set_error("wt_refine_tracks_host: bad argument");
        return WT_ERR_INVALID;
    }
    int64_t max_traj = 0, n_traj_total = 0;
    WT_TRY(wt::check_refine_layout(in, &max_traj, &n_traj_total));
    WT_TRY(wt::check_track_args("wt_refine_tracks_host", n_frames, n_streams, r_sets, set_row_offsets[r_sets], n_traj_total, max_traj, n_jobs, n_classes,
                                true, wt::grid_fits(n_jobs, n_streams), kGridText, (int)n_jobs, (int)n_streams));
    WT_TRY(wt::ensure_device());
    const size_t nf = (size_t)(n_frames + 1), J = (size_t)n_jobs;
    wt::StagedTrackSet st;
    wt::DevBuf jg, jl, jm, djo, dws;
    WT_TRY(st.upload(in, n_jobs, job_result));
    WT_TRY(jg.upload(job_max_gap, 4 * J * (size_t)n_classes)); WT_TRY(jl.upload(job_min_len, 4 * J * (size_t)n_classes));
    WT_TRY(jm.upload(job_score_mode, 4 * J));
    WT_TRY(djo.alloc(8 * (J + 1)));
    const size_t wsb = wt_refine_tracks_workspace(n_jobs, n_streams, st.n_rows, n_traj_total, max_traj);
    WT_TRY(dws.alloc(wsb));
    const Layout L = make_layout(st.dev, st.n_rows, st.dt.as<int64_t>(), n_traj_total, max_traj, n_jobs, st.jr.as<int32_t>(), jg.as<int32_t>(),
                                 jl.as<int32_t>());
    WT_TRY(launch_plan(L, st.dev.score, djo.as<int64_t>(), st.status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(st.finish("refine plan", "counts or offsets"));
    WT_HIP(hipMemcpy(job_row_offsets, djo.p, 8 * (J + 1), hipMemcpyDeviceToHost));
    if (out_cap == 0) return WT_OK;                                    // the sizing call
    const int64_t n_out = job_row_offsets[J];
    if (out_cap < n_out) {
        wt::set_error("wt_refine_tracks_host: %lld rows are planned, the output holds %lld", (long long)n_out, (long long)out_cap);
        return WT_ERR_CAPACITY;
    }
    const size_t no = (size_t)n_out;
    wt::DevBuf of, oc, ob, os, ol, osrc, ofro;
    WT_TRY(of.alloc(8 * no)); WT_TRY(oc.alloc(4 * no)); WT_TRY(ob.alloc(32 * no)); WT_TRY(os.alloc(8 * no)); WT_TRY(ol.alloc(4 * no));
    WT_TRY(osrc.alloc(8 * no)); WT_TRY(ofro.alloc(8 * J * nf));
    const Boxes B = {st.dev.x, st.dev.y, st.dev.w, st.dev.h};
    const Outputs O = {of.as<int64_t>(), oc.as<int32_t>(), ob.as<double>(), os.as<double>(), ol.as<int32_t>(), osrc.as<int64_t>(), ofro.as<int64_t>()};
    WT_TRY(launch_emit(L, B, st.dev.score, jm.as<int32_t>(), djo.as<int64_t>(), n_out, O, st.status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(st.finish("refine emit", "counts or offsets"));
    if (no) {
        WT_HIP(hipMemcpy(out_frame, of.p, 8 * no, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(out_category, oc.p, 4 * no, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_bbox, ob.p, 32 * no, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(out_score, os.p, 8 * no, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_local, ol.p, 4 * no, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(out_source, osrc.p, 8 * no, hipMemcpyDeviceToHost));
    }
    if (J * nf) WT_HIP(hipMemcpy(out_frame_row_offsets, ofro.p, 8 * J * nf, hipMemcpyDeviceToHost));
    return WT_OK;
}

}  // extern "C"
