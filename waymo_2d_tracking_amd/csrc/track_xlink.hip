// Cross-class track linking on gfx950 (include/waymotrack.h, "Cross-class track linking"; DESIGN.md section 31 has the
// definition): the repair of class flicker.  A trajectory that ends (tail) is linked to one of the same stream that begins up to
// max_link[ci][cj] slots later (head) - ci, cj the classes of the two, the pair switched on by a symmetric table - when the tail's
// extrapolated box overlaps the head's first box; the linked pieces take the id of the earliest one and the class the chain's
// rows vote for.  R tracking results come in once; J jobs each name a result and their parameters.  No row is added, removed or
// moved.
//
// Two launches, one 64-lane wavefront per independent problem:
//   1. summary: per (result, stream), walk the slots once: per trajectory the first slot and row, the last slot and row, the slot
//               and row before the last, the class and the row count.  Shared by all jobs of the result.
//   2. match:   per (job, stream).  The rounds of locally dominant pairs of track_stitch.hip - scan A, scan B, accept - with one
//               difference: a tail's head range is bounded by the largest max_link of its class's row of the table, and the
//               pair's own gap and threshold are tested per head.  After the roots are resolved one lane per root walks its
//               chain - once for the mask of the classes in it, once per class of the mask for that class's rows, once to write
//               the winner to every member - and the wavefront labels its rows with root and class.
// The rounds are this unit's own copy: track_stitch.hip is byte for byte what it was (profiles/track_xlink.txt says why).
// The tables of the match (36 bytes per trajectory) live in LDS up to kLdsTraj trajectories, in the workspace beyond.
// Compile with -ffp-contract=off: the extrapolation is x + ((x - xp) / (e - p)) * n with every operation rounded on its own, and
// iou_dd is the IoU the metrics use.
#include "eval_device.h"
#include "tracks_device.h"
#include "xlink_host.h"

using namespace wtdev;

namespace {

constexpr int kLdsTraj = 1024;                // trajectories of one (result, stream) up to which the match tables stay in LDS
constexpr int kTableBytes = 36;               // per trajectory: two uint64, one double, three int32

struct Layout : TrackLayout {                 // device pointers
    const int32_t *job_pair_max_link, *job_class_prio, *job_motion;
    const double* job_pair_link_iou;
};

struct Summary {                              // [n_traj_total] each; slots relative to the stream's first, rows to the stream's first row; -1 none
    int32_t *first_slot, *first_row, *last_slot, *last_row, *prev_slot, *prev_row, *cls, *cnt;
};

struct Workspace {
    int32_t* rounds;                          // [J * n_streams] the rounds the match of each problem took; first in the workspace
    Summary sum;
    unsigned long long *head_a, *head_k;      // [J * n_traj_total] the tables of the problems above kLdsTraj (all six)
    double* tail_a;
    int32_t *tail_j, *succ, *pred;
    size_t bytes;
};

Workspace carve(void* base, size_t n_jobs, size_t n_streams, size_t n_traj_total, size_t max_traj) {
    wt::Carver cv(base);
    Workspace w;
    const size_t big = max_traj > (size_t)kLdsTraj ? n_jobs * n_traj_total : 0;
    w.rounds = cv.take<int32_t>(n_jobs * n_streams + 1);
    int32_t** cols[8] = {&w.sum.first_slot, &w.sum.first_row, &w.sum.last_slot, &w.sum.last_row, &w.sum.prev_slot, &w.sum.prev_row, &w.sum.cls, &w.sum.cnt};
    for (auto c : cols) *c = cv.take<int32_t>(n_traj_total + 1);
    w.head_a = cv.take<unsigned long long>(big + 1);
    w.head_k = cv.take<unsigned long long>(big + 1);
    w.tail_a = cv.take<double>(big + 1);
    w.tail_j = cv.take<int32_t>(big + 1);
    w.succ = cv.take<int32_t>(big + 1);
    w.pred = cv.take<int32_t>(big + 1);
    w.bytes = cv.off;
    return w;
}

__global__ __launch_bounds__(kWave) void xlink_summary_kernel(Layout L, Summary S, int* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int r = (int)(blockIdx.x / (unsigned)L.n_streams), s = (int)(blockIdx.x % (unsigned)L.n_streams);
    const Span q = span_of(L, r, s);
    if (!q.ok) {
        if (lane == 0) atomicMax(status, kErrCapacity);
        return;
    }
    const int T = q.T;
    for (int t = lane; t < T; t += kWave) {
        const size_t g = (size_t)q.t0 + t;
        S.first_slot[g] = -1; S.first_row[g] = -1; S.last_slot[g] = -1; S.last_row[g] = -1; S.prev_slot[g] = -1; S.prev_row[g] = -1; S.cls[g] = 0;
        S.cnt[g] = 0;
    }
    wsync();
    int err = 0;
    for_stream_rows(q, L.local, &err, [&](long long d, int t, int fo) {
        const size_t g = (size_t)q.t0 + t;
        const int row = (int)(d - q.rs0);
        if (S.first_slot[g] < 0) { S.first_slot[g] = fo; S.first_row[g] = row; S.cls[g] = L.category[d]; }
        S.prev_slot[g] = S.last_slot[g];
        S.prev_row[g] = S.last_row[g];
        S.last_slot[g] = fo;
        S.last_row[g] = row;
        S.cnt[g] += 1;
    });
    if (__ballot(err != 0) != 0ull && lane == 0) atomicMax(status, kErrCapacity);
}

struct Outputs {
    int32_t *pred, *root;                     // [J * n_traj_total]
    double* affinity;                         // [J * n_traj_total]
    int32_t* cls;                             // [J * n_traj_total]
    int32_t *row_root, *row_category;         // [J * n_rows]
    int64_t *links, *relabelled;              // [J * n_streams]
};

// every entry: no link, no root, no class; the match kernel fills those of its job's result
__global__ void xlink_init_kernel(Outputs O, long long n_traj, long long n_row) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_traj) { O.pred[i] = -1; O.root[i] = -1; O.affinity[i] = -1.0; O.cls[i] = -1; }
    if (i < n_row) { O.row_root[i] = -1; O.row_category[i] = -1; }
}

// first t in [0, T) with slot[t] >= v (slot is non-decreasing where the local indices are by first appearance); always inside [0, T]
__device__ __forceinline__ int lower_bound_slot(const int32_t* __restrict__ slot, int T, int v) {
    int lo = 0, hi = T;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (slot[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The candidate heads of one free tail, in ascending index: visit(j, n, a) for every free head j, n = its gap, a = the affinity,
// when the pair is a candidate (rule 1 of the definition): gap and threshold are those of the pair (tail's class, head's class).
struct Tail {
    int e, lo, hi;
    const int32_t* max_link;                  // the tail's class's row of the job's tables, [n_classes]
    const double* thr;
    double px0, py0, vx, vy, w, h;
    bool linear;
};

template <class Visit>
__device__ __forceinline__ void scan_heads(const Tail& t, const Summary& S, size_t g0, int C, const Boxes& B, long long rs0, long long n_stream_rows,
                                           const int32_t* pred, Visit visit) {
    for (int j = t.lo; j < t.hi; ++j) {
        if (pred[j] >= 0) continue;
        const int cj = S.cls[g0 + j];
        if (cj < 1 || cj > C) continue;
        const int n = S.first_slot[g0 + j] - t.e, fr = S.first_row[g0 + j];
        if (n < 1 || n > t.max_link[cj - 1] || fr < 0 || fr >= n_stream_rows) continue;
        double px = t.px0, py = t.py0;
        if (t.linear) { px = t.px0 + t.vx * (double)n; py = t.py0 + t.vy * (double)n; }
        const double pb[4] = {px, py, px + t.w, py + t.h};
        double hb[4];
        B.get(rs0 + fr, hb);
        const double a = iou_dd(pb, hb);
        if (a >= t.thr[cj - 1] && a > 0.) visit(j, n, a);
    }
}

__global__ __launch_bounds__(kWave) void xlink_match_kernel(Layout L, Boxes B, Workspace ws, Outputs O, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const size_t p = blockIdx.x;
    int j_, s_;
    decode_job_stream(p, L.n_streams, &j_, &s_);
    const int job = j_, s = s_;
    const Span q = span_of(L, L.job_result[job], s);
    if (!q.ok) {
        if (lane == 0) { atomicMax(status, kErrCapacity); O.links[p] = 0; O.relabelled[p] = 0; ws.rounds[p] = 0; }
        return;
    }
    const int T = q.T, C = L.n_classes;
    const Summary S = ws.sum;
    const size_t g0 = (size_t)q.t0;
    const size_t tbase = (size_t)job * (size_t)L.n_traj_total + g0;
    const size_t lbase = (size_t)job * (size_t)L.n_rows;
    const bool in_lds = T <= L.lds_traj;
    const size_t stride = (size_t)L.lds_traj;
    unsigned long long* head_a = in_lds ? reinterpret_cast<unsigned long long*>(smem) : ws.head_a + tbase;
    unsigned long long* head_k = in_lds ? head_a + stride : ws.head_k + tbase;
    double* tail_a = in_lds ? reinterpret_cast<double*>(head_k + stride) : ws.tail_a + tbase;
    int32_t* tail_j = in_lds ? reinterpret_cast<int32_t*>(tail_a + stride) : ws.tail_j + tbase;   // after the matching: the root
    int32_t* succ = in_lds ? tail_j + stride : ws.succ + tbase;                                      // the head linked to this tail, -1 free, -2 no candidate left
    int32_t* pred = in_lds ? succ + stride : ws.pred + tbase;                                        // the tail linked to this head, -1 free
    const int32_t* links = L.job_pair_max_link + (size_t)job * C * C;
    const double* thrs = L.job_pair_link_iou + (size_t)job * C * C;
    const int32_t* prio = L.job_class_prio + (size_t)job * C;
    const bool linear = L.job_motion[job] == 1;
    int err = 0;
    const long long end = stream_end(q, &err);
    const long long n_stream_rows = end - q.rs0;
    for (int t = lane; t < T; t += kWave) { succ[t] = -1; pred[t] = -1; }
    wsync();

    // what a free tail needs for its scans; false: it can never link
    auto make_tail = [&](int i, Tail* t) {
        const int c = S.cls[g0 + i];
        if (c < 1 || c > C) return false;
        t->max_link = links + (size_t)(c - 1) * C;
        t->thr = thrs + (size_t)(c - 1) * C;
        int reach = 0;                                                 // the largest gap any pair of the tail's class allows
        for (int k = 0; k < C; ++k) reach = t->max_link[k] > reach ? t->max_link[k] : reach;
        const int e = S.last_slot[g0 + i], row = S.last_row[g0 + i];
        if (reach < 1 || e < 0 || row < 0 || row >= n_stream_rows) return false;
        t->e = e;
        const long long hi_slot = (long long)e + reach + 1;
        t->lo = lower_bound_slot(S.first_slot + g0, T, e + 1);
        t->hi = lower_bound_slot(S.first_slot + g0, T, hi_slot > 0x7fffffffll ? 0x7fffffff : (int)hi_slot);
        const long long d = q.rs0 + row;
        t->px0 = B.x[d]; t->py0 = B.y[d]; t->w = B.w[d]; t->h = B.h[d];
        const int ps = S.prev_slot[g0 + i], prow = S.prev_row[g0 + i];
        t->linear = linear && ps >= 0 && prow >= 0 && prow < n_stream_rows && e > ps;
        t->vx = 0.; t->vy = 0.;
        if (t->linear) {
            const long long dp = q.rs0 + prow;
            t->vx = (t->px0 - B.x[dp]) / (double)(e - ps);
            t->vy = (t->py0 - B.y[dp]) / (double)(e - ps);
        }
        return t->lo < t->hi;
    };

    int rounds = 0;
    for (int round = 0; round <= T; ++round) {                         // every round but the last accepts a pair: at most T rounds
        for (int t = lane; t < T; t += kWave) { head_a[t] = 0ull; head_k[t] = ~0ull; }
        wsync();
        // ---- scan A: per head the highest affinity offered, per tail its best head ----
        for (int ib = 0; ib < T; ib += kWave) {
            const int i = ib + lane;
            if (i >= T || succ[i] != -1) continue;
            Tail t;
            int bj = -1;
            double ba = 0.;
            if (make_tail(i, &t))
                scan_heads(t, S, g0, C, B, q.rs0, n_stream_rows, pred, [&](int j, int n, double a) {
                    atomicMax(&head_a[j], (unsigned long long)__double_as_longlong(a));
                    if (a > ba) { ba = a; bj = j; }                    // ascending j is ascending n: the first of equal affinities is the best
                });
            tail_a[i] = ba;
            tail_j[i] = bj;
            if (bj < 0) succ[i] = -2;                                  // the free heads only get fewer
        }
        wsync();
        // ---- scan B: per head the smallest (n, i) among the tails that offer exactly its highest affinity ----
        for (int ib = 0; ib < T; ib += kWave) {
            const int i = ib + lane;
            if (i >= T || succ[i] != -1) continue;
            Tail t;
            if (make_tail(i, &t))
                scan_heads(t, S, g0, C, B, q.rs0, n_stream_rows, pred, [&](int j, int n, double a) {
                    if ((unsigned long long)__double_as_longlong(a) == head_a[j])
                        atomicMin(&head_k[j], ((unsigned long long)(unsigned)n << 32) | (unsigned)i);
                });
        }
        wsync();
        // ---- accept the pairs that are best on both sides ----
        bool any = false;
        for (int ib = 0; ib < T; ib += kWave) {
            const int i = ib + lane;
            bool mine = false;
            if (i < T && succ[i] == -1) {
                const int j = tail_j[i];
                const int n = S.first_slot[g0 + j] - S.last_slot[g0 + i];
                mine = (unsigned long long)__double_as_longlong(tail_a[i]) == head_a[j] &&
                       head_k[j] == (((unsigned long long)(unsigned)n << 32) | (unsigned)i);
                if (mine) { succ[i] = j; pred[j] = i; O.affinity[tbase + j] = tail_a[i]; }
            }
            any = any || __ballot(mine) != 0ull;
        }
        wsync();
        if (!any) break;
        ++rounds;
        if (round == T) err = kErrCapacity;                            // cannot happen: a round that accepts uses up a tail
    }

    // ---- roots and link count ----
    int32_t* root = tail_j;
    int32_t* chain_cls = reinterpret_cast<int32_t*>(head_a);          // the matching is over: its first table holds the chain's class
    long long n_links = 0;
    for (int t = lane; t < T; t += kWave) {
        int r = t, steps = 0;
        while (pred[r] >= 0 && steps < T) { r = pred[r]; ++steps; }
        if (pred[r] >= 0) err = kErrCapacity;                          // a cycle: links go forward in time, so there is none
        root[t] = r;
        O.pred[tbase + t] = pred[t];
        O.root[tbase + t] = r;
        n_links += pred[t] >= 0;
    }
    for (int o = 32; o > 0; o >>= 1) n_links += __shfl_xor(n_links, o, kWave);
    wsync();
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
        for (int t = r; t >= 0 && steps < T; t = succ[t], ++steps) { chain_cls[t] = best_c; O.cls[tbase + t] = best_c; }
    }
    wsync();
    // ---- row labels ----
    long long n_rel = 0;
    for (long long d = q.rs0 + lane; d < end; d += kWave) {
        const int t = L.local[d];
        if (t < 0 || t >= T) { err = kErrCapacity; continue; }
        const int c = chain_cls[t];
        O.row_root[lbase + d] = root[t];
        O.row_category[lbase + d] = c;
        n_rel += c != L.category[d];
    }
    for (int o = 32; o > 0; o >>= 1) n_rel += __shfl_xor(n_rel, o, kWave);
    if (__ballot(err != 0) != 0ull && lane == 0) atomicMax(status, kErrCapacity);
    if (lane == 0) { O.links[p] = n_links; O.relabelled[p] = n_rel; ws.rounds[p] = rounds; }
}

constexpr const char* kGridText = "%s: %d jobs, %d results x %d streams in one call";

int launch(const char* entry, const Layout& L, const Boxes& B, const Outputs& O, int32_t* status_dev, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    WT_TRY(wt::ensure_device());
    const Workspace ws = carve(wt::align_ptr(workspace), (size_t)L.n_jobs, (size_t)L.n_streams, (size_t)L.n_traj_total, (size_t)L.max_traj);
    WT_TRY(wt::check_workspace_fits(entry, workspace, workspace_bytes, ws.bytes, WT_ERR_CAPACITY));
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    const size_t P = (size_t)L.n_jobs * (size_t)L.n_streams, RS = (size_t)L.r_sets * (size_t)L.n_streams;
    const long long n_traj = (long long)L.n_jobs * L.n_traj_total, n_row = (long long)L.n_jobs * L.n_rows;
    const long long n_init = n_traj > n_row ? n_traj : n_row;
    if (n_init > 0x7fffffffll * 256) { wt::set_error("%s: %d jobs over %lld rows in one call", entry, (int)L.n_jobs, (long long)L.n_rows); return WT_ERR_CAPACITY; }
    if (n_init) hipLaunchKernelGGL(xlink_init_kernel, dim3((unsigned)((n_init + 255) / 256)), dim3(256), 0, stream, O, n_traj, n_row);
    if (P) {
        hipLaunchKernelGGL(xlink_summary_kernel, dim3((unsigned)RS), dim3(kWave), 0, stream, L, ws.sum, (int*)status_dev);
        hipLaunchKernelGGL(xlink_match_kernel, dim3((unsigned)P), dim3(kWave), (size_t)L.lds_traj * kTableBytes, stream, L, B, ws, O, (int*)status_dev);
    }
    WT_HIP(hipGetLastError());
    return WT_OK;
}

}  // namespace

extern "C" {

void wt_xlink_tracks_limits(int32_t* lds_trajectories) {
    if (lds_trajectories) *lds_trajectories = kLdsTraj;
}

size_t wt_xlink_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj) {
    if (n_jobs < 0 || n_streams < 0 || n_rows < 0 || n_traj_total < 0 || max_traj < 0) return 0;
    return carve(nullptr, (size_t)n_jobs, (size_t)n_streams, (size_t)n_traj_total, (size_t)(max_traj > 0 ? max_traj : 1)).bytes + 256;
}

int wt_xlink_tracks_rounds(const void* workspace, int32_t n_jobs, int32_t n_streams, int32_t* out_rounds) {
    const size_t P = (size_t)(n_jobs > 0 ? n_jobs : 0) * (size_t)(n_streams > 0 ? n_streams : 0);
    if (!workspace || n_jobs < 0 || n_streams < 0 || (P && !out_rounds)) {
        wt::set_error("wt_xlink_tracks_rounds: bad argument");
        return WT_ERR_INVALID;
    }
    if (P) WT_HIP(hipMemcpy(out_rounds, wt::align_ptr(const_cast<void*>(workspace)), 4 * P, hipMemcpyDeviceToHost));
    return WT_OK;
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
                                wt::grid_fits(n_jobs, n_streams) && wt::grid_fits(r_sets, n_streams), kGridText, (int)n_jobs, (int)r_sets, (int)n_streams));
    if (n_classes > wt::kXLinkMaxClasses) { wt::set_error("wt_xlink_tracks_dev: %d classes, at most %d", (int)n_classes, (int)wt::kXLinkMaxClasses); return WT_ERR_INVALID; }
    const wt::TrackSet dev = {n_frames, n_streams, stream_frame_offsets, r_sets, set_row_offsets, frame_row_offsets, x, y, w, h, nullptr,
                              category, local, nullptr, n_classes};
    Layout L;
    wt::fill_track_layout(&L, dev, n_rows, traj_offsets, n_traj_total, max_traj, n_jobs, job_result, kLdsTraj);
    L.job_pair_max_link = job_pair_max_link; L.job_pair_link_iou = job_pair_link_iou; L.job_class_prio = job_class_prio; L.job_motion = job_motion;
    const Boxes B = {x, y, w, h};
    const Outputs O = {out_pred, out_root, out_affinity, out_cls, out_row_root, out_row_category, out_links, out_relabelled};
    return launch("wt_xlink_tracks_dev", L, B, O, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
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
    if ((J * nt && !(out_pred && out_root && out_affinity && out_cls)) || (J * nr && !(out_row_root && out_row_category)) ||
        (J * (size_t)n_streams && !(out_links && out_relabelled))) {
        wt::set_error("wt_xlink_tracks_host: bad argument");
        return WT_ERR_INVALID;
    }
    WT_TRY(wt::check_track_args("wt_xlink_tracks_host", n_frames, n_streams, r_sets, (int64_t)nr, n_traj_total, max_traj, n_jobs, n_classes, true,
                                wt::grid_fits(n_jobs, n_streams) && wt::grid_fits(r_sets, n_streams), kGridText, (int)n_jobs, (int)r_sets, (int)n_streams));
    WT_TRY(wt::ensure_device());
    wt::StagedTrackSet st;
    wt::DevBuf jl, ji, jp, jm, op, oo, oa, oc, orr, orc, ol, orl, dws;
    WT_TRY(st.upload(in, n_jobs, job_result));
    WT_TRY(jl.upload(job_pair_max_link, 4 * J * C * C)); WT_TRY(ji.upload(job_pair_link_iou, 8 * J * C * C));
    WT_TRY(jp.upload(job_class_prio, 4 * J * C)); WT_TRY(jm.upload(job_motion, 4 * J));
    WT_TRY(op.alloc(4 * J * nt)); WT_TRY(oo.alloc(4 * J * nt)); WT_TRY(oa.alloc(8 * J * nt)); WT_TRY(oc.alloc(4 * J * nt));
    WT_TRY(orr.alloc(4 * J * nr)); WT_TRY(orc.alloc(4 * J * nr));
    WT_TRY(ol.alloc(8 * J * (size_t)n_streams)); WT_TRY(orl.alloc(8 * J * (size_t)n_streams));
    const size_t wsb = wt_xlink_tracks_workspace(n_jobs, n_streams, (int64_t)nr, n_traj_total, max_traj);
    WT_TRY(dws.alloc(wsb));
    Layout L;
    st.fill(&L, n_traj_total, max_traj, n_jobs, kLdsTraj);
    L.job_pair_max_link = jl.as<int32_t>(); L.job_pair_link_iou = ji.as<double>(); L.job_class_prio = jp.as<int32_t>(); L.job_motion = jm.as<int32_t>();
    const Boxes B = {st.dev.x, st.dev.y, st.dev.w, st.dev.h};
    const Outputs O = {op.as<int32_t>(), oo.as<int32_t>(), oa.as<double>(), oc.as<int32_t>(), orr.as<int32_t>(), orc.as<int32_t>(), ol.as<int64_t>(),
                       orl.as<int64_t>()};
    WT_TRY(launch("wt_xlink_tracks_host", L, B, O, st.status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(st.finish("xlink", "counts or offsets"));
    if (J * nt) {
        WT_HIP(hipMemcpy(out_pred, op.p, 4 * J * nt, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(out_root, oo.p, 4 * J * nt, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_affinity, oa.p, 8 * J * nt, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(out_cls, oc.p, 4 * J * nt, hipMemcpyDeviceToHost));
    }
    if (J * nr) {
        WT_HIP(hipMemcpy(out_row_root, orr.p, 4 * J * nr, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_row_category, orc.p, 4 * J * nr, hipMemcpyDeviceToHost));
    }
    if (J * (size_t)n_streams) {
        WT_HIP(hipMemcpy(out_links, ol.p, 8 * J * (size_t)n_streams, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_relabelled, orl.p, 8 * J * (size_t)n_streams, hipMemcpyDeviceToHost));
    }
    return WT_OK;
}

}  // extern "C"
