// Track splitting on gfx950 (include/waymotrack.h, "Track splitting"; DESIGN.md section 25 has the definition): a trajectory is
// cut between two consecutive observations when the gap between them is longer than split_gap slots, or when every motion test
// that exists for the pair - the box extrapolated forward from the two rows before it, the box extrapolated backward from the two
// rows after it, the held box when there is neither - overlaps the other side by less than split_iou.  Piece 0 keeps the identity;
// the other pieces of a result are numbered in the order (stream, local index, piece).  R tracking results come in once; J jobs
// each name a result and their parameters.  No row is added, removed or moved.
//
// Four launches:
//   1. link:  per (result, stream), one 64-lane wavefront walks the slots once, the rows of a slot lane-parallel: per row the
//             distance in rows to the previous and to the next row of its trajectory, its slot and its trajectory's class.  The
//             per-trajectory table (last row, class) lives in LDS up to kLdsTraj trajectories, in the workspace beyond.  Shared by
//             all jobs of the result.
//   2. test:  one lane per (job, row).  It gathers the rows i - 2 .. i + 1 of its trajectory through the link distances, computes
//             the tests of the pair that ends at the row and writes them and the break bit (into out_piece, which the count walk
//             turns into the piece in place).  The same launch gives every output of a result the job does not name its -1.
//   3. count: per (job, stream), one wavefront walks the slots with a counter per trajectory (LDS up to kLdsTraj trajectories, the
//             workspace beyond): the piece of every row, the breaks of every trajectory, their exclusive scan over the stream's
//             trajectories and the stream's total.
//   4. rank:  per (job, stream), one wavefront sums the totals of the streams before its own and numbers the rows of its new pieces.
// Compile with -ffp-contract=off: the extrapolation is x + ((x - xo) / slots) * n with every operation rounded on its own, and
// iou_dd is the IoU the metrics use.
#include "eval_device.h"
#include "tracks_device.h"
#include "split_host.h"

using namespace wtdev;

namespace {

constexpr int kLdsTraj = 2048;                // trajectories of one (result, stream) up to which the per-trajectory tables stay in LDS
constexpr int kTestBlock = 256;

struct Layout : TrackLayout {                 // device pointers
    const double* job_split_iou;
    const int32_t *job_split_gap, *job_motion;
};

struct Links {                                // [n_rows] each; zeroed before the link walk: a row no slot holds has no chain and class 0
    int32_t *back, *fwd;                      // rows from this one to the previous / next row of its trajectory; 0 = none
    int32_t *slot, *cls;                      // the row's slot relative to its stream's first; its trajectory's class
};

struct Workspace {
    Links ln;
    int32_t *last, *tcls;                     // [n_traj_total] the link table of the (result, stream)s above kLdsTraj
    int32_t* before;                          // [J * n_traj_total] the breaks of the stream's trajectories before this one (above kLdsTraj: the counter first)
    size_t link_bytes, bytes;
};

Workspace carve(void* base, size_t n_jobs, size_t n_rows, size_t n_traj_total, size_t max_traj) {
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
    w.before = cv.take<int32_t>(n_jobs * n_traj_total + 1);
    w.bytes = cv.off;
    return w;
}

__global__ __launch_bounds__(kWave) void split_link_kernel(Layout L, Workspace ws, int* __restrict__ status) {
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

struct Outputs {
    int32_t* piece;                           // [J * n_rows]
    int64_t* fresh;                           // [J * n_rows] out_new
    double* test;                             // [J * n_rows * 2]
    int32_t* breaks;                          // [J * n_traj_total]
    int64_t* new_pieces;                      // [J * n_streams]
};

// v + ((v - other) / slots) * n, every operation rounded on its own
__device__ __forceinline__ double extrapolate(double v, double other, int slots, int n) {
    const double step = v - other;
    const double rate = step / (double)slots;
    const double move = rate * (double)n;
    return v + move;
}

// index i: entry i of the (J, n_traj_total) output and (job, row) i of the (J, n_rows) outputs
__global__ __launch_bounds__(kTestBlock) void split_test_kernel(Layout L, Boxes B, Links ln, Outputs O, long long n_traj, long long n_row,
                                                               int* __restrict__ status) {
    const long long o = (long long)blockIdx.x * kTestBlock + threadIdx.x;
    if (o < n_traj) O.breaks[o] = -1;
    if (o >= n_row) return;
    double first = -1.0, second = -1.0;
    int brk = -1;                                                       // -1: not a row of the job's result
    const int j = (int)(o / L.n_rows);
    const long long d = o - (long long)j * L.n_rows;
    const int r = L.job_result[j];
    long long base = 0, rend = 0;
    if (r < 0 || r >= L.r_sets) {
        atomicMax(status, kErrCapacity);
    } else {
        base = L.set_row_offsets[r];
        rend = L.set_row_offsets[r + 1];
        if (base < 0 || rend < base || rend > L.n_rows) { atomicMax(status, kErrCapacity); base = rend = 0; }
    }
    const int c = d >= base && d < rend ? ln.cls[d] : 0;                // 0: a row no slot holds
    if (c >= 1 && c <= L.n_classes) {
        brk = 0;
        const int b1 = ln.back[d];
        const long long i1 = d - b1;                                    // row i - 1
        if (b1 > 0 && i1 < base) atomicMax(status, kErrCapacity);
        if (b1 > 0 && i1 >= base) {
            const double thr = L.job_split_iou[(size_t)j * L.n_classes + (c - 1)];
            const int gap = L.job_split_gap[(size_t)j * L.n_classes + (c - 1)];
            const int n = ln.slot[d] - ln.slot[i1];
            if (gap > 0 && n > gap) brk = 1;
            if (thr > 0.) {
                const bool linear = L.job_motion[j] == 1;
                double cur[4], prev[4];
                B.get(d, cur);
                B.get(i1, prev);
                bool fails = true;                                      // every test that exists gives a < thr
                bool any = false;
                const int b2 = ln.back[i1], f1 = ln.fwd[d];
                if (linear && b2 > 0) {
                    const long long i2 = i1 - b2;                       // row i - 2
                    if (i2 < base) {
                        atomicMax(status, kErrCapacity);
                    } else {
                        const int p = ln.slot[i1] - ln.slot[i2];
                        const double px = extrapolate(B.x[i1], B.x[i2], p, n), py = extrapolate(B.y[i1], B.y[i2], p, n);
                        const double pb[4] = {px, py, px + B.w[i1], py + B.h[i1]};
                        first = iou_dd(pb, cur);
                        fails = fails && first < thr;
                        any = true;
                    }
                }
                if (linear && f1 > 0) {
                    const long long nx = d + f1;                        // row i + 1
                    if (nx >= rend) {
                        atomicMax(status, kErrCapacity);
                    } else {
                        const int qn = ln.slot[nx] - ln.slot[d];
                        const double px = extrapolate(B.x[d], B.x[nx], qn, n), py = extrapolate(B.y[d], B.y[nx], qn, n);
                        const double pb[4] = {px, py, px + B.w[d], py + B.h[d]};
                        second = iou_dd(pb, prev);
                        fails = fails && second < thr;
                        any = true;
                    }
                }
                if (!any) {
                    first = iou_dd(prev, cur);
                    fails = first < thr;
                }
                if (fails) brk = 1;
            }
        }
    }
    O.test[o * 2] = first;
    O.test[o * 2 + 1] = second;
    O.piece[o] = brk;
    O.fresh[o] = -1;
}

__global__ __launch_bounds__(kWave) void split_count_kernel(Layout L, Workspace ws, Outputs O, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const size_t p = blockIdx.x;
    int j_, s_;
    decode_job_stream(p, L.n_streams, &j_, &s_);
    const int job = j_, s = s_;
    const Span q = span_of(L, L.job_result[job], s);
    if (!q.ok) {
        if (lane == 0) { atomicMax(status, kErrCapacity); O.new_pieces[p] = 0; }
        return;
    }
    const int T = q.T;
    const size_t tbase = (size_t)job * (size_t)L.n_traj_total + (size_t)q.t0;
    const size_t lbase = (size_t)job * (size_t)L.n_rows;
    int32_t* before = ws.before + tbase;
    int32_t* count = T <= L.lds_traj ? reinterpret_cast<int32_t*>(smem) : before;     // the trajectory's breaks so far
    for (int t = lane; t < T; t += kWave) count[t] = 0;
    wsync();
    int err = 0;
    for_stream_rows(q, L.local, &err, [&](long long d, int t, int) {
        const int brk = O.piece[lbase + d];                             // the test launch's bit; -1: the link walk did not reach the row
        if (brk < 0) err = kErrCapacity;
        const int c = count[t] + (brk > 0);
        count[t] = c;
        O.piece[lbase + d] = c;
    });
    long long total = 0;                                                // of the trajectories before this chunk
    for (int tb = 0; tb < T; tb += kWave) {
        const int t = tb + lane;
        const int mine = t < T ? count[t] : 0;
        long long incl = mine;
        for (int o = 1; o < kWave; o <<= 1) {
            const long long up = __shfl_up(incl, o, kWave);
            if (lane >= o) incl += up;
        }
        const long long excl = total + incl - mine;
        if (t < T) {
            if (excl > 0x7fffffffll) err = kErrCapacity;
            O.breaks[tbase + t] = mine;
            before[t] = (int32_t)excl;
        }
        total += __shfl(incl, kWave - 1, kWave);
    }
    if (__ballot(err != 0) != 0ull && lane == 0) atomicMax(status, kErrCapacity);
    if (lane == 0) O.new_pieces[p] = total;
}

__global__ __launch_bounds__(kWave) void split_rank_kernel(Layout L, Workspace ws, Outputs O, int* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const size_t p = blockIdx.x;
    int j_, s_;
    decode_job_stream(p, L.n_streams, &j_, &s_);
    const int job = j_, s = s_;
    const Span q = span_of(L, L.job_result[job], s);
    if (!q.ok) return;                                                  // the count walk has reported it
    long long offset = 0;                                               // the new pieces of the streams before this one
    for (int sb = 0; sb < s; sb += kWave)
        if (sb + lane < s) offset += O.new_pieces[(size_t)job * L.n_streams + sb + lane];
    for (int o = 32; o > 0; o >>= 1) offset += __shfl_xor(offset, o, kWave);
    const int32_t* before = ws.before + (size_t)job * (size_t)L.n_traj_total + (size_t)q.t0;
    const size_t lbase = (size_t)job * (size_t)L.n_rows;
    int err = 0;
    const long long end = stream_end(q, &err);
    for (long long d = q.rs0 + lane; d < end; d += kWave) {
        const int t = L.local[d];
        if (t < 0 || t >= q.T) { err = kErrCapacity; continue; }
        const int piece = O.piece[lbase + d];
        if (piece > 0) O.fresh[lbase + d] = offset + before[t] + (piece - 1);
    }
    if (__ballot(err != 0) != 0ull && lane == 0) atomicMax(status, kErrCapacity);
}

constexpr const char* kGridText = "%s: %d jobs, %d results x %d streams, %lld rows in one call";

bool grid_ok(int32_t n_jobs, int32_t r_sets, int32_t n_streams, int64_t n_rows, int64_t n_traj_total) {
    const uint64_t most = (uint64_t)(n_rows > n_traj_total ? n_rows : n_traj_total);
    return wt::grid_fits(n_jobs, n_streams) && wt::grid_fits(r_sets, n_streams) && (n_jobs == 0 || most <= 0x7fffffffull * kTestBlock / (uint64_t)n_jobs);
}

int launch(const char* entry, const Layout& L, const Boxes& B, const Outputs& O, int32_t* status_dev, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    WT_TRY(wt::ensure_device());
    const Workspace ws = carve(wt::align_ptr(workspace), (size_t)L.n_jobs, (size_t)L.n_rows, (size_t)L.n_traj_total, (size_t)L.max_traj);
    WT_TRY(wt::check_workspace_fits(entry, workspace, workspace_bytes, ws.bytes, WT_ERR_CAPACITY));
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    const size_t P = (size_t)L.n_jobs * (size_t)L.n_streams, RS = (size_t)L.r_sets * (size_t)L.n_streams;
    const long long n_traj = (long long)L.n_jobs * L.n_traj_total, n_row = (long long)L.n_jobs * L.n_rows;
    const long long n_test = n_traj > n_row ? n_traj : n_row;
    if (n_test) WT_HIP(hipMemsetAsync(ws.ln.back, 0, ws.link_bytes, stream));
    if (P) {
        hipLaunchKernelGGL(split_link_kernel, dim3((unsigned)RS), dim3(kWave), 0, stream, L, ws, (int*)status_dev);
    }
    if (n_test)
        hipLaunchKernelGGL(split_test_kernel, dim3((unsigned)((n_test + kTestBlock - 1) / kTestBlock)), dim3(kTestBlock), 0, stream, L, B, ws.ln, O,
                           n_traj, n_row, (int*)status_dev);
    if (P) {
        hipLaunchKernelGGL(split_count_kernel, dim3((unsigned)P), dim3(kWave), (size_t)L.lds_traj * sizeof(int32_t), stream, L, ws, O, (int*)status_dev);
        hipLaunchKernelGGL(split_rank_kernel, dim3((unsigned)P), dim3(kWave), 0, stream, L, ws, O, (int*)status_dev);
    }
    WT_HIP(hipGetLastError());
    return WT_OK;
}

}  // namespace

extern "C" {

void wt_split_tracks_limits(int32_t* lds_trajectories) {
    if (lds_trajectories) *lds_trajectories = kLdsTraj;
}

size_t wt_split_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj) {
    if (n_jobs < 0 || n_streams < 0 || n_rows < 0 || n_traj_total < 0 || max_traj < 0) return 0;
    return carve(nullptr, (size_t)n_jobs, (size_t)n_rows, (size_t)n_traj_total, (size_t)(max_traj > 0 ? max_traj : 1)).bytes + 256;
}

int wt_split_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                        int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                        const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                        const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                        int32_t n_jobs, const int32_t* job_result, const double* job_split_iou, const int32_t* job_split_gap,
                        const int32_t* job_motion, int32_t n_classes,
                        int32_t* out_piece, int64_t* out_new, double* out_test, int32_t* out_breaks, int64_t* out_new_pieces,
                        int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    WT_TRY(wt::check_track_args("wt_split_tracks_dev", n_frames, n_streams, r_sets, n_rows, n_traj_total, max_traj, n_jobs, n_classes,
                                stream_frame_offsets && set_row_offsets && frame_row_offsets && x && y && w && h && category && local && traj_offsets &&
                                    job_result && job_split_iou && job_split_gap && job_motion && out_piece && out_new && out_test && out_breaks &&
                                    out_new_pieces && status_dev,
                                grid_ok(n_jobs, r_sets, n_streams, n_rows, n_traj_total), kGridText, (int)n_jobs, (int)r_sets, (int)n_streams, (long long)n_rows));
    const wt::TrackSet dev = {n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, nullptr,
                              category, local, nullptr, n_classes};
    Layout L;
    wt::fill_track_layout(&L, dev, n_rows, traj_offsets, n_traj_total, max_traj, n_jobs, job_result, kLdsTraj);
    L.job_split_iou = job_split_iou; L.job_split_gap = job_split_gap; L.job_motion = job_motion;
    const Boxes B = {x, y, w, h};
    const Outputs O = {out_piece, out_new, out_test, out_breaks, out_new_pieces};
    return launch("wt_split_tracks_dev", L, B, O, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_split_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                         const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const double* job_split_iou,
                         const int32_t* job_split_gap, const int32_t* job_motion, int32_t n_classes,
                         int32_t* out_piece, int64_t* out_new, double* out_test, int32_t* out_breaks, int64_t* out_new_pieces) {
    const wt::SplitInput in = {{n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, nullptr,
                                category, local, n_traj, n_classes}, n_jobs, job_result, job_split_iou, job_split_gap, job_motion};
    int64_t max_traj = 0, n_traj_total = 0;
    WT_TRY(wt::check_split_layout(in, &max_traj, &n_traj_total));
    const size_t nr = (size_t)set_row_offsets[r_sets], J = (size_t)n_jobs, nt = (size_t)n_traj_total;
    if ((J * nr && !(out_piece && out_new && out_test)) || (J * nt && !out_breaks) || (J * (size_t)n_streams && !out_new_pieces)) {
        wt::set_error("wt_split_tracks_host: bad argument");
        return WT_ERR_INVALID;
    }
    WT_TRY(wt::check_track_args("wt_split_tracks_host", n_frames, n_streams, r_sets, (int64_t)nr, n_traj_total, max_traj, n_jobs, n_classes, true,
                                grid_ok(n_jobs, r_sets, n_streams, (int64_t)nr, n_traj_total), kGridText, (int)n_jobs, (int)r_sets, (int)n_streams, (long long)nr));
    WT_TRY(wt::ensure_device());
    wt::StagedTrackSet st;
    wt::DevBuf ji, jg, jm, op, on, ot, ob, os, dws;
    WT_TRY(st.upload(in, n_jobs, job_result));
    WT_TRY(ji.upload(job_split_iou, 8 * J * (size_t)n_classes));
    WT_TRY(jg.upload(job_split_gap, 4 * J * (size_t)n_classes)); WT_TRY(jm.upload(job_motion, 4 * J));
    WT_TRY(op.alloc(4 * J * nr)); WT_TRY(on.alloc(8 * J * nr)); WT_TRY(ot.alloc(16 * J * nr)); WT_TRY(ob.alloc(4 * J * nt));
    WT_TRY(os.alloc(8 * J * (size_t)n_streams));
    const size_t wsb = wt_split_tracks_workspace(n_jobs, n_streams, (int64_t)nr, n_traj_total, max_traj);
    WT_TRY(dws.alloc(wsb));
    Layout L;
    st.fill(&L, n_traj_total, max_traj, n_jobs, kLdsTraj);
    L.job_split_iou = ji.as<double>(); L.job_split_gap = jg.as<int32_t>(); L.job_motion = jm.as<int32_t>();
    const Boxes B = {st.dev.x, st.dev.y, st.dev.w, st.dev.h};
    const Outputs O = {op.as<int32_t>(), on.as<int64_t>(), ot.as<double>(), ob.as<int32_t>(), os.as<int64_t>()};
    WT_TRY(launch("wt_split_tracks_host", L, B, O, st.status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(st.finish("split", "counts or offsets"));
    if (J * nr) {
        WT_HIP(hipMemcpy(out_piece, op.p, 4 * J * nr, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(out_new, on.p, 8 * J * nr, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_test, ot.p, 16 * J * nr, hipMemcpyDeviceToHost));
    }
    if (J * nt) WT_HIP(hipMemcpy(out_breaks, ob.p, 4 * J * nt, hipMemcpyDeviceToHost));
    if (J * (size_t)n_streams) WT_HIP(hipMemcpy(out_new_pieces, os.p, 8 * J * (size_t)n_streams, hipMemcpyDeviceToHost));
    return WT_OK;
}

}  // extern "C"
