// Trajectory coverage (MT / PT / ML and fragmentations per ground-truth trajectory) of tracking results on gfx950
// (include/waymotrack.h, "MOT trajectory coverage"; DESIGN.md section 27 has the definition).
//
// A consumer of what wt_mot_eval_dev leaves in HBM: hyp_match / hyp_switch per result row.  Integers only.  Three passes:
//   mark   one lane per result row: a matched row stores the byte 1 | switch << 1 at mark[set][ground-truth row].  Two result
//          rows of a set never match the same ground-truth row, so the stores do not collide.
//   link   one wavefront per (stream, class), once per call (it does not depend on the results): walks the stream's frames in
//          order and chains every row of the class to the next row of its trajectory (next_row), head[trajectory] = its first
//          row.  The last row seen of every trajectory is a table in LDS (4096 ints).
//   walk   one lane per (result set, trajectory): follows the chain, reads the mark bytes, keeps both levels' len / tracked /
//          frag / idsw and run state in registers, writes its traj_stats row and adds its class into cov_counts: per wavefront
//          and (problem, level) one ballot + popcount per class, one shuffle sum for frag, one integer atomic per field.
#include "eval_device.h"
#include "coverage_host.h"

using namespace wtdev;

namespace {

constexpr int kMaxTraj = wt::kCoverageMaxTraj;
constexpr long long kMaxFrames = wt::kCoverageMaxFrames;
constexpr int kFields = 5;                   // traj, mt, pt, ml, frag

struct Workspace {                           // device pointers carved from one block
    unsigned char* mark;                     // [K][n_gt] 1 | switch << 1 where a result row of the set matches the row
    int* next_row;                           // [n_gt] the next row of the row's trajectory, -1 at its end
    int* head;                               // [total_traj] first row, -1 when the trajectory has none
    int* bad;                                // [n_streams * n_classes] 1 where the link pass refused the problem
    size_t bytes;
};

Workspace carve(void* base, size_t k_sets, size_t n_gt, size_t total_traj, size_t n_sc) {
    wt::Carver cv(base);
    Workspace w;
    w.mark = cv.take<unsigned char>(k_sets * n_gt + 1);
    w.next_row = cv.take<int>(n_gt + 1);
    w.head = cv.take<int>(total_traj + 1);
    w.bad = cv.take<int>(n_sc + 1);
    w.bytes = cv.off;
    return w;
}

// ---- mark ----
__global__ __launch_bounds__(256) void coverage_mark_kernel(long long n_hyp, long long n_gt, int K, const int64_t* __restrict__ set_row_offsets,
                                                            const int64_t* __restrict__ hyp_match, const uint8_t* __restrict__ hyp_switch,
                                                            unsigned char* __restrict__ mark, int* __restrict__ status) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_hyp) return;
    const long long m = hyp_match[i];
    if (m < 0) return;
    int lo = 0, hi = K;                                        // the set k with set_row_offsets[k] <= i < set_row_offsets[k + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (set_row_offsets[mid] <= i) lo = mid; else hi = mid;
    }
    if (m >= n_gt || i < set_row_offsets[lo] || i >= set_row_offsets[lo + 1]) { atomicMax(status, kErrCapacity); return; }
    mark[(size_t)lo * (size_t)n_gt + (size_t)m] = (unsigned char)(1 | ((hyp_switch[i] & 1) << 1));
}

// ---- link ----
__global__ __launch_bounds__(kWave) void coverage_link_kernel(
    long long n_gt, const int32_t* __restrict__ g_cat, const int32_t* __restrict__ g_traj, long long n_frames,
    const int64_t* __restrict__ frame_gt_offsets, int C, const int64_t* __restrict__ stream_frame_offsets,
    const int32_t* __restrict__ g_ntraj, const int64_t* __restrict__ traj_offsets, long long total_traj, Workspace ws, int* __restrict__ status) {
    __shared__ int last_row[kMaxTraj];
    const int lane = threadIdx.x & 63;
    const size_t sc = blockIdx.x;
    const int s = (int)(sc / C), c = (int)(sc % C) + 1;
    const int nT = g_ntraj[sc];
    const long long t0 = traj_offsets[sc], t1 = traj_offsets[sc + 1];
    const long long f0 = stream_frame_offsets[s], f1 = stream_frame_offsets[s + 1];
    bool err = nT < 0 || nT > kMaxTraj || t0 < 0 || t1 - t0 != nT || t1 > total_traj || f0 < 0 || f1 < f0 || f1 > n_frames || f1 - f0 > kMaxFrames;
    if (err) { if (lane == 0) { ws.bad[sc] = 1; atomicMax(status, kErrCapacity); } return; }
    for (int t = lane; t < nT; t += kWave) last_row[t] = -1;
    wsync();
    int* head = ws.head + t0;
    // the offsets of 63 frames at a time, one per lane, so that a frame's rows do not wait for a load of its offsets
    for (long long fb = f0; fb < f1 && !err; fb += kWave - 1) {
        const long long fl = fb + lane;
        const long long off = frame_gt_offsets[fl <= f1 ? fl : f1];
        const int nf = (int)((f1 - fb) < (kWave - 1) ? (f1 - fb) : (kWave - 1));
        for (int j = 0; j < nf && !err; ++j) {
            const long long g0 = (long long)readlane64((unsigned long long)off, j), g1 = (long long)readlane64((unsigned long long)off, j + 1);
            if (g0 < 0 || g1 < g0 || g1 > n_gt) { err = true; break; }
            for (long long base = g0; base < g1; base += kWave) {      // a trajectory occurs at most once per frame: the lanes' trajectories differ
                const long long row = base + lane;
                bool bad_row = false;
                if (row < g1 && g_cat[row] == c) {
                    const int t = g_traj[row];
                    if (t < 0 || t >= nT) bad_row = true;
                    else {
                        const int prev = last_row[t];
                        if (prev < 0) head[t] = (int)row; else ws.next_row[prev] = (int)row;
                        last_row[t] = (int)row;
                    }
                }
                if (__ballot(bad_row) != 0ull) { err = true; break; }
                wsync();
            }
        }
    }
    if (err && lane == 0) { ws.bad[sc] = 1; atomicMax(status, kErrCapacity); }
}

// ---- walk ----
struct Run {                                 // one level of one trajectory
    int len = 0, tracked = 0, frag = 0, idsw = 0;
    bool seen = false, gap = false;          // a matched row lies behind; unmatched rows since then
    __device__ __forceinline__ void row(int m) {
        ++len;
        if (m & 1) {
            ++tracked;
            idsw += (m >> 1) & 1;
            frag += gap ? 1 : 0;
            gap = false;
            seen = true;
        } else {
            gap = seen;
        }
    }
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__global__ __launch_bounds__(256) void coverage_walk_kernel(
    long long n_gt, const int32_t* __restrict__ g_level, int K, int n_sc, const int64_t* __restrict__ traj_offsets, long long total_traj,
    Workspace ws, int64_t* __restrict__ cov_counts, int32_t* __restrict__ traj_stats) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < (long long)K * total_traj;
    const int k = act ? (int)(i / total_traj) : 0;
    const long long t = act ? i % total_traj : 0;
    int sc = -1;
    Run r1, r2;                                                // LEVEL_1 (rows whose level is not 2), LEVEL_2 (every row)
    if (act) {
        int lo = 0, hi = n_sc;                                 // the (stream, class) with traj_offsets[sc] <= t < traj_offsets[sc + 1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (traj_offsets[mid] <= t) lo = mid; else hi = mid;
        }
        if (traj_offsets[lo] <= t && t < traj_offsets[lo + 1] && !ws.bad[lo]) sc = lo;
    }
    if (sc >= 0) {
        const unsigned char* mark = ws.mark + (size_t)k * (size_t)n_gt;
        int row = ws.head[t], steps = 0;
        while (row >= 0 && steps <= kMaxFrames) {              // the chain ascends, one row per frame at most
            const int nxt = ws.next_row[row];
            const int m = mark[row];
            const bool easy = g_level[row] != 2;
            r2.row(m);
            if (easy) r1.row(m);
            row = nxt;
            ++steps;
        }
    }
    if (act && traj_stats) {
        int4* o = reinterpret_cast<int4*>(traj_stats + (size_t)i * 8);
        o[0] = make_int4(r1.len, r1.tracked, r1.frag, r1.idsw);
        o[1] = make_int4(r2.len, r2.tracked, r2.frag, r2.idsw);
    }
    // the lanes of one wavefront that share a problem add their counts together: one atomic per (problem, level, field)
    const int prob = sc >= 0 ? k * n_sc + sc : -1;
    unsigned long long todo = __ballot(prob >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int pl = __builtin_amdgcn_readlane(prob, uni(leader));
        const bool mine = prob == pl;
        todo &= ~__ballot(mine);
#pragma unroll
        for (int lv = 0; lv < 2; ++lv) {
            const Run& r = lv ? r2 : r1;
            const bool is = mine && r.len > 0;
            const bool mt = is && 5 * r.tracked >= 4 * r.len, ml = is && 5 * r.tracked < r.len;
            const int n_traj = __popcll(__ballot(is)), n_mt = __popcll(__ballot(mt)), n_ml = __popcll(__ballot(ml));
            const int n_frag = wave_sum(is ? r.frag : 0);
            if (lane == leader && n_traj) {
                unsigned long long* o = reinterpret_cast<unsigned long long*>(cov_counts) + ((size_t)pl * 2 + lv) * kFields;
                atomicAdd(o + 0, (unsigned long long)n_traj);
                if (n_mt) atomicAdd(o + 1, (unsigned long long)n_mt);
                if (n_traj - n_mt - n_ml) atomicAdd(o + 2, (unsigned long long)(n_traj - n_mt - n_ml));
                if (n_ml) atomicAdd(o + 3, (unsigned long long)n_ml);
                if (n_frag) atomicAdd(o + 4, (unsigned long long)n_frag);
            }
        }
    }
}

struct Args {                                // wt_mot_coverage_dev's arguments, device pointers
    int64_t n_gt;
    const int32_t *g_category, *g_level, *g_traj;
    int64_t n_frames;
    const int64_t* frame_gt_offsets;
    int32_t n_streams;
    const int64_t* stream_frame_offsets;
    int32_t n_classes;
    const int32_t* g_ntraj;
    const int64_t* traj_offsets;
    int64_t total_traj;
    int32_t k_sets;
    int64_t n_hyp;
    const int64_t* set_row_offsets;
    const int64_t* hyp_match;
    const uint8_t* hyp_switch;
};

int launch(const Args& a, int64_t* cov_counts, int32_t* traj_stats, int32_t* status_dev, void* workspace, size_t workspace_bytes,
           hipStream_t stream, hipEvent_t* pass_events) {
    WT_TRY(wt::ensure_device());
    if (a.k_sets < 1 || a.n_streams < 0 || a.n_frames < 0 || a.n_gt < 0 || a.n_hyp < 0 || a.total_traj < 0 || !cov_counts || !status_dev ||
        !a.g_category || !a.g_level || !a.g_traj || !a.frame_gt_offsets || !a.stream_frame_offsets || !a.g_ntraj || !a.traj_offsets ||
        !a.set_row_offsets || !a.hyp_match || !a.hyp_switch) {
        wt::set_error("wt_mot_coverage: bad argument");
        return WT_ERR_INVALID;
    }
    if (a.n_classes < 1 || a.n_classes > kMaxClasses) { wt::set_error("wt_mot_coverage: n_classes must be 1..%d", kMaxClasses); return WT_ERR_INVALID; }
    const size_t n_sc = (size_t)a.n_streams * (size_t)a.n_classes, n_problems = n_sc * (size_t)a.k_sets;
    const size_t lanes = (size_t)a.k_sets * (size_t)a.total_traj;
    if (a.n_gt > 0x7fffffffll || n_problems > 0x7fffffffull || lanes > (0x7fffffffull << 8) || a.n_hyp > (0x7fffffffll << 8)) {
        wt::set_error("wt_mot_coverage: %lld ground-truth rows, %zu problems, %zu trajectories: too many for one call", (long long)a.n_gt, n_problems, lanes);
        return WT_ERR_CAPACITY;
    }
    Workspace ws = carve(wt::align_ptr(workspace), (size_t)a.k_sets, (size_t)a.n_gt, (size_t)a.total_traj, n_sc);
    if (!workspace || workspace_bytes < ws.bytes + 256) {
        wt::set_error("coverage workspace too small: need %zu bytes, have %zu", ws.bytes + 256, workspace_bytes);
        return WT_ERR_INVALID;
    }
    if (pass_events) WT_HIP(hipEventRecord(pass_events[0], stream));      // [0, 1): the clears and the mark pass, [1, 2): link, [2, 3): walk
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    if (n_problems) WT_HIP(hipMemsetAsync(cov_counts, 0, n_problems * 2 * kFields * sizeof(int64_t), stream));
    // mark = 0, next_row = head = -1, bad = 0: the carved arrays follow each other
    WT_HIP(hipMemsetAsync(ws.mark, 0, (size_t)((char*)ws.next_row - (char*)ws.mark), stream));
    WT_HIP(hipMemsetAsync(ws.next_row, 0xff, (size_t)((char*)ws.bad - (char*)ws.next_row), stream));
    WT_HIP(hipMemsetAsync(ws.bad, 0, (n_sc + 1) * sizeof(int), stream));
    if (a.n_hyp > 0)
        hipLaunchKernelGGL(coverage_mark_kernel, dim3((unsigned)((a.n_hyp + 255) / 256)), dim3(256), 0, stream, (long long)a.n_hyp, (long long)a.n_gt,
                           (int)a.k_sets, a.set_row_offsets, a.hyp_match, a.hyp_switch, ws.mark, (int*)status_dev);
    if (pass_events) WT_HIP(hipEventRecord(pass_events[1], stream));
    if (n_sc)
        hipLaunchKernelGGL(coverage_link_kernel, dim3((unsigned)n_sc), dim3(kWave), 0, stream, (long long)a.n_gt, a.g_category, a.g_traj,
                           (long long)a.n_frames, a.frame_gt_offsets, (int)a.n_classes, a.stream_frame_offsets, a.g_ntraj, a.traj_offsets,
                           (long long)a.total_traj, ws, (int*)status_dev);
    if (pass_events) WT_HIP(hipEventRecord(pass_events[2], stream));
    if (lanes && n_sc)
        hipLaunchKernelGGL(coverage_walk_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, (long long)a.n_gt, a.g_level,
                           (int)a.k_sets, (int)n_sc, a.traj_offsets, (long long)a.total_traj, ws, cov_counts, traj_stats);
    if (pass_events) WT_HIP(hipEventRecord(pass_events[3], stream));
    WT_HIP(hipGetLastError());
    return WT_OK;
}

}  // namespace

extern "C" {

size_t wt_mot_coverage_workspace(int32_t k_sets, int32_t n_streams, int32_t n_classes, int64_t n_gt, int64_t total_traj) {
    if (k_sets < 1 || n_streams < 0 || n_classes < 1 || n_gt < 0 || total_traj < 0) return 0;
    return carve(nullptr, (size_t)k_sets, (size_t)n_gt, (size_t)total_traj, (size_t)n_streams * (size_t)n_classes).bytes + 256;
}

int wt_mot_coverage_dev(int64_t n_gt, const int32_t* g_category, const int32_t* g_level, const int32_t* g_traj,
                        int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                        int32_t n_classes, const int32_t* g_ntraj, const int64_t* traj_offsets, int64_t total_traj,
                        int32_t k_sets, int64_t n_hyp, const int64_t* set_row_offsets, const int64_t* hyp_match, const uint8_t* hyp_switch,
                        int64_t* cov_counts, int32_t* traj_stats, int32_t* status_dev,
                        void* workspace, size_t workspace_bytes, void* stream_, void* const* pass_events) {
    const Args a = {n_gt, g_category, g_level, g_traj, n_frames, frame_gt_offsets, n_streams, stream_frame_offsets, n_classes, g_ntraj, traj_offsets,
                    total_traj, k_sets, n_hyp, set_row_offsets, hyp_match, hyp_switch};
    return launch(a, cov_counts, traj_stats, status_dev, workspace, workspace_bytes, (hipStream_t)stream_, (hipEvent_t*)pass_events);
}

int wt_mot_coverage_host(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                         const int32_t* g_category, const int32_t* g_level, const int32_t* g_id, const int32_t* g_traj,
                         int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t k_sets, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                         const double* hx, const double* hy, const double* hw, const double* hh,
                         const int32_t* h_category, const int32_t* h_id,
                         const int32_t* g_ntraj, int32_t n_classes, const double* thr,
                         int64_t* cov_counts, int32_t* traj_stats) {
    const wt::TrackInput in = {n_gt, gx, gy, gw, gh, g_category, g_level, g_id, n_frames, frame_gt_offsets, n_streams, stream_frame_offsets,
                               k_sets, set_row_offsets, frame_hyp_offsets, hx, hy, hw, hh, h_category, h_id, n_classes};
    if (!thr || !cov_counts) { wt::set_error("wt_mot_coverage_host: bad argument"); return WT_ERR_INVALID; }
    int64_t max_traj = 0, total_traj = 0;
    WT_TRY(wt::check_coverage_layout({in, g_traj, g_ntraj}, &max_traj, &total_traj));
    int64_t max_boxes = 0;
    int32_t max_gt_ids = 0;
    wt::coverage_eval_bounds(in, &max_boxes, &max_gt_ids);
    const size_t n_sc = (size_t)n_streams * (size_t)n_classes, n_problems = n_sc * (size_t)k_sets;
    std::vector<int64_t> traj_offsets(n_sc + 1, 0);
    for (size_t i = 0; i < n_sc; ++i) traj_offsets[i + 1] = traj_offsets[i] + g_ntraj[i];
    const size_t eval_wsb = wt_mot_eval_workspace(k_sets, n_streams, n_classes, max_boxes, max_gt_ids);
    const size_t wsb = wt_mot_coverage_workspace(k_sets, n_streams, n_classes, n_gt, total_traj);
    if (!eval_wsb || !wsb) {
        wt::set_error("wt_mot_coverage_host: %lld boxes of one class in one frame: the evaluation takes no more than 4096", (long long)max_boxes);
        return WT_ERR_CAPACITY;
    }
    WT_TRY(wt::ensure_device());
    wt::StagedTrackInput staged;
    WT_TRY(staged.upload(in));
    const size_t nh = (size_t)staged.n_hyp;
    wt::DevBuf dtraj, dnt, dto, dcnt, dsum, dmatch, dswitch, dews, dcov, dstats, dstatus, dws;
    WT_TRY(dtraj.upload(g_traj, 4 * (size_t)n_gt)); WT_TRY(dnt.upload(g_ntraj, 4 * n_sc)); WT_TRY(dto.upload(traj_offsets.data(), 8 * (n_sc + 1)));
    WT_TRY(dcnt.alloc(8 * n_problems * 10)); WT_TRY(dsum.alloc(8 * n_problems * 2));
    WT_TRY(dmatch.alloc(8 * nh)); WT_TRY(dswitch.alloc(nh)); WT_TRY(dews.alloc(eval_wsb));
    WT_TRY(dcov.alloc(8 * n_problems * 2 * kFields)); WT_TRY(dstatus.alloc(16)); WT_TRY(dws.alloc(wsb));
    const size_t stats_bytes = 4 * (size_t)k_sets * (size_t)total_traj * 8;
    if (traj_stats) WT_TRY(dstats.alloc(stats_bytes));
    const wt::TrackInput& d = staged.dev;
    WT_TRY(wt_mot_eval_dev(n_gt, d.gx, d.gy, d.gw, d.gh, d.g_category, d.g_level, d.g_id, n_frames, d.frame_gt_offsets, n_streams,
                           d.stream_frame_offsets, k_sets, staged.n_hyp, d.set_row_offsets, d.frame_hyp_offsets, d.hx, d.hy, d.hw, d.hh,
                           d.h_category, d.h_id, n_classes, thr, max_boxes, max_gt_ids, dcnt.as<int64_t>(), dsum.as<double>(),
                           dmatch.as<int64_t>(), dswitch.as<uint8_t>(), staged.status.as<int32_t>(), dews.p, eval_wsb, nullptr));
    const Args a = {n_gt, d.g_category, d.g_level, dtraj.as<int32_t>(), n_frames, d.frame_gt_offsets, n_streams, d.stream_frame_offsets, n_classes,
                    dnt.as<int32_t>(), dto.as<int64_t>(), total_traj, k_sets, staged.n_hyp, d.set_row_offsets, dmatch.as<int64_t>(), dswitch.as<uint8_t>()};
    WT_TRY(launch(a, dcov.as<int64_t>(), traj_stats ? dstats.as<int32_t>() : nullptr, dstatus.as<int32_t>(), dws.p, wsb, nullptr, nullptr));
    WT_TRY(staged.finish("evaluation"));
    int32_t st = 0;
    WT_HIP(hipMemcpy(&st, dstatus.p, sizeof(st), hipMemcpyDeviceToHost));
    if (st) { wt::set_error("coverage kernel reported status %d (4 = capacity)", (int)st); return (int)st; }
    if (n_problems) WT_HIP(hipMemcpy(cov_counts, dcov.p, 8 * n_problems * 2 * kFields, hipMemcpyDeviceToHost));
    if (traj_stats && stats_bytes) WT_HIP(hipMemcpy(traj_stats, dstats.p, stats_bytes, hipMemcpyDeviceToHost));
    return WT_OK;
}

}  // extern "C"
