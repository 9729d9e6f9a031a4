// Linking of trajectories across gaps, shared by track_stitch.hip (links inside a class) and
// track_xlink.hip (links across classes, section 31): the summary of a (result, stream), the match of a (job, stream) in rounds
// without a table of pairs, the workspace both carve and the three launches.  A trajectory that ends (tail) is linked to one of the
// same stream that begins up to max_link slots later (head) when the tail's extrapolated box overlaps the head's first box.  What
// differs between the two passes is a Policy, a small struct the match is compiled for - no flag is read at run time on its account:
//   static constexpr bool kRowCounts, kRounds           whether the summary counts the rows of every trajectory (Summary::cnt) and
//                                                       whether the workspace keeps the rounds of every problem (Workspace::rounds)
//   static Policy make(const PassLayout& L, int job)    the job's parameters
//   Row row(int c)                                      what a tail of class c (1..n_classes) carries through its scans:
//     int reach()                                         the largest gap the tail may cross to any head, 0 when it can never link
//     bool meets(int cj)                                  whether a head of class cj can be a candidate at all; where it cannot, nothing
//                                                         else of the head is read
//     int max_link(int cj)                                the largest gap to a head of class cj, 0 when the pair is off; asked only where
//     double threshold(int cj)                            meets(cj), as is what the affinity has to reach
// Two launches, one 64-lane wavefront per independent problem:
//   1. summary: per (result, stream), walk the slots once: per trajectory the first slot and row, the last slot and row, the slot
//               and row before the last, the class and - for a pass that asks - the row count.  Shared by all jobs of the result.
//   2. match:   per (job, stream).  The answer is the greedy walk of all candidate pairs in the strict order (-a, n, i, j); it is
//               computed in rounds of locally dominant pairs, without a table of pairs: a lane owns a free tail and scans its heads -
//               local indices are by first appearance, so the heads whose first slot lies in [e + 1, e + reach] are a contiguous
//               range found by two binary searches.  Scan A gives every head the highest affinity any free tail offers it (64-bit
//               atomic max on the bits of a positive double) and every tail its best head; scan B gives every head the smallest
//               (n, i) among the tails that offer exactly that affinity; a pair that is its tail's best and its head's best is
//               accepted.  The smallest free pair always is one, so a round without an acceptance ends the matching.  The same
//               wavefront then resolves the roots and counts the links (match_problem); the pass's kernel goes on from there with
//               what is its own - the row labels, and whatever it makes of the chains.
// The tables of the match (36 bytes per trajectory) live in LDS up to kLdsTraj trajectories, in the workspace beyond.
// Include it only from units compiled with -ffp-contract=off: the extrapolation is x + ((x - xp) / (e - p)) * n with every
// operation rounded on its own, and iou_dd is the IoU the metrics use.
#pragma once
#include "eval_device.h"
#include "tracks_device.h"
#include "tracks_host.h"

namespace wtdev {
namespace link {

constexpr int kLdsTraj = 1024;                // trajectories of one (result, stream) up to which the match tables stay in LDS
constexpr int kTableBytes = 36;               // per trajectory: two uint64, one double, three int32
constexpr const char* kGridText = "%s: %d jobs, %d results x %d streams in one call";

struct Layout : TrackLayout {                 // device pointers; a pass's Layout is this plus its own job parameters
    const int32_t* job_motion;                // [J] 0 hold, 1 linear
};

struct Summary {                              // [n_traj_total] each; slots relative to the stream's first, rows to the stream's first row; -1 none
    int32_t *first_slot, *first_row, *last_slot, *last_row, *prev_slot, *prev_row, *cls;
    int32_t* cnt;                             // the rows of the trajectory; NULL for a pass that does not ask for it
};

struct Workspace {
    int32_t* rounds;                          // [J * n_streams] the rounds the match of each problem took, first in the workspace; NULL for a pass without
    Summary sum;
    unsigned long long *head_a, *head_k;      // [J * n_traj_total] the tables of the problems above kLdsTraj (all six)
    double* tail_a;
    int32_t *tail_j, *succ, *pred;
    size_t bytes;
};

// with_rounds / with_counts: the pass's Policy::kRounds / kRowCounts; what a pass does not ask for takes no byte
inline Workspace carve(void* base, bool with_rounds, bool with_counts, size_t n_jobs, size_t n_streams, size_t n_traj_total, size_t max_traj) {
    wt::Carver cv(base);
    Workspace w;
    const size_t big = max_traj > (size_t)kLdsTraj ? n_jobs * n_traj_total : 0;
    w.rounds = with_rounds ? cv.take<int32_t>(n_jobs * n_streams + 1) : nullptr;
    int32_t** cols[7] = {&w.sum.first_slot, &w.sum.first_row, &w.sum.last_slot, &w.sum.last_row, &w.sum.prev_slot, &w.sum.prev_row, &w.sum.cls};
    for (auto c : cols) *c = cv.take<int32_t>(n_traj_total + 1);
    w.sum.cnt = with_counts ? cv.take<int32_t>(n_traj_total + 1) : nullptr;
    w.head_a = cv.take<unsigned long long>(big + 1);
    w.head_k = cv.take<unsigned long long>(big + 1);
    w.tail_a = cv.take<double>(big + 1);
    w.tail_j = cv.take<int32_t>(big + 1);
    w.succ = cv.take<int32_t>(big + 1);
    w.pred = cv.take<int32_t>(big + 1);
    w.bytes = cv.off;
    return w;
}

template <bool kRowCounts>
static __global__ __launch_bounds__(kWave) void link_summary_kernel(Layout L, Summary S, int* __restrict__ status) {
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
        if (kRowCounts) S.cnt[g] = 0;
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
        if (kRowCounts) S.cnt[g] += 1;
    });
    if (__ballot(err != 0) != 0ull && lane == 0) atomicMax(status, kErrCapacity);
}

struct Outputs {                              // a pass's Outputs is this, or this plus its own with an init() that also calls this one
    int32_t *pred, *root;                     // [J * n_traj_total]
    double* affinity;                         // [J * n_traj_total]
    int32_t* row_root;                        // [J * n_rows]
    int64_t* links;                           // [J * n_streams]
    // entry i of every per-trajectory and per-row output: no link, no root
    __device__ __forceinline__ void init(long long i, long long n_traj, long long n_row) const {
        if (i < n_traj) { pred[i] = -1; root[i] = -1; affinity[i] = -1.0; }
        if (i < n_row) row_root[i] = -1;
    }
};

// every entry: nothing; the match kernel fills those of its job's result
template <class PassOutputs>
static __global__ void link_init_kernel(PassOutputs O, long long n_traj, long long n_row) {
    O.init((long long)blockIdx.x * blockDim.x + threadIdx.x, n_traj, n_row);
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
// when the pair is a candidate (rule 1 of the definitions): gap and threshold are those the tail's row gives for the head's class.
template <class Row>
struct Tail {
    int e, lo, hi;
    Row row;
    double px0, py0, vx, vy, w, h;
    bool linear;
};

template <class Row, class Visit>
__device__ __forceinline__ void scan_heads(const Tail<Row>& t, const Summary& S, size_t g0, const Boxes& B, long long rs0, long long n_stream_rows,
                                           const int32_t* pred, Visit visit) {
    for (int j = t.lo; j < t.hi; ++j) {
        if (pred[j] >= 0) continue;
        const int cj = S.cls[g0 + j];
        if (!t.row.meets(cj)) continue;
        const int n = S.first_slot[g0 + j] - t.e, fr = S.first_row[g0 + j];
        if (n < 1 || n > t.row.max_link(cj) || fr < 0 || fr >= n_stream_rows) continue;
        double px = t.px0, py = t.py0;
        if (t.linear) { px = t.px0 + t.vx * (double)n; py = t.py0 + t.vy * (double)n; }
        const double pb[4] = {px, py, px + t.w, py + t.h};
        double hb[4];
        B.get(rs0 + fr, hb);
        const double a = iou_dd(pb, hb);
        if (a >= t.row.threshold(cj) && a > 0.) visit(j, n, a);
    }
}

// What match_problem leaves for the pass's epilogue.  ok = false: the problem's numbers do not fit; status and O.links are
// written and nothing else is valid.
struct Matched {
    bool ok;
    int job, rounds, err;                     // rounds: those that accepted a pair; err != 0 in the lanes that met numbers that do not fit
    Span q;
    long long end, n_links;                   // one past the stream's last row
    size_t tbase, lbase;                      // the problem's first entry of the per-trajectory outputs, the job's first of the per-row ones
    int32_t *root, *succ, *pred;              // [T] the chain's first, the head linked to this tail (< 0 none), the tail linked to this head (-1 none)
    int32_t* spare;                           // [T] the first table of the match, free now
};

// The match of problem blockIdx.x = (job, stream) by one wavefront: the rounds, the roots, the link count; it writes O.pred, O.root
// and O.affinity of the problem.  smem: lds_traj * kTableBytes bytes of dynamic LDS.  The wavefront is synchronised on return.
template <class Policy, class PassLayout>
__device__ __forceinline__ Matched match_problem(const PassLayout& L, const Boxes& B, const Workspace& ws, const Outputs& O, int* __restrict__ status, char* smem) {
    const int lane = threadIdx.x & 63;
    const size_t p = blockIdx.x;
    int j_, s_;
    decode_job_stream(p, L.n_streams, &j_, &s_);
    const int job = j_, s = s_;
    Matched M;
    M.job = job;
    M.q = span_of(L, L.job_result[job], s);
    M.ok = M.q.ok;
    if (!M.ok) {
        if (lane == 0) { atomicMax(status, kErrCapacity); O.links[p] = 0; }
        return M;
    }
    const Span& q = M.q;
    const int T = q.T, C = L.n_classes;
    const Summary S = ws.sum;
    const size_t g0 = (size_t)q.t0;
    const size_t tbase = (size_t)job * (size_t)L.n_traj_total + g0;
    const bool in_lds = T <= L.lds_traj;
    const size_t stride = (size_t)L.lds_traj;
    unsigned long long* head_a = in_lds ? reinterpret_cast<unsigned long long*>(smem) : ws.head_a + tbase;
    unsigned long long* head_k = in_lds ? head_a + stride : ws.head_k + tbase;
    double* tail_a = in_lds ? reinterpret_cast<double*>(head_k + stride) : ws.tail_a + tbase;
    int32_t* tail_j = in_lds ? reinterpret_cast<int32_t*>(tail_a + stride) : ws.tail_j + tbase;   // after the matching: the root
    int32_t* succ = in_lds ? tail_j + stride : ws.succ + tbase;                                      // the head linked to this tail, -1 free, -2 no candidate left
    int32_t* pred = in_lds ? succ + stride : ws.pred + tbase;                                        // the tail linked to this head, -1 free
    const Policy P = Policy::make(L, job);
    using TailT = Tail<decltype(P.row(1))>;
    const bool linear = L.job_motion[job] == 1;
    int err = 0;
    const long long end = stream_end(q, &err);
    const long long n_stream_rows = end - q.rs0;
    for (int t = lane; t < T; t += kWave) { succ[t] = -1; pred[t] = -1; }
    wsync();

    // what a free tail needs for its scans; false: it can never link
    auto make_tail = [&](int i, TailT* t) {
        const int c = S.cls[g0 + i];
        if (c < 1 || c > C) return false;
        t->row = P.row(c);
        const int reach = t->row.reach();
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
            TailT t;
            int bj = -1;
            double ba = 0.;
            if (make_tail(i, &t))
                scan_heads(t, S, g0, B, q.rs0, n_stream_rows, pred, [&](int j, int n, double a) {
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
            TailT t;
            if (make_tail(i, &t))
                scan_heads(t, S, g0, B, q.rs0, n_stream_rows, pred, [&](int j, int n, double a) {
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
    M.end = end; M.tbase = tbase; M.lbase = (size_t)job * (size_t)L.n_rows;
    M.root = root; M.succ = succ; M.pred = pred; M.spare = reinterpret_cast<int32_t*>(head_a);
    M.n_links = n_links; M.rounds = rounds; M.err = err;
    return M;
}

// The three launches of a pass on `stream`; match_kernel(L, B, ws, O, status) is the pass's kernel around match_problem<Policy>.
template <class Policy, class PassLayout, class PassOutputs, class MatchKernel>
int launch(const char* entry, MatchKernel match_kernel, const PassLayout& L, const Boxes& B, const PassOutputs& O, int32_t* status_dev, void* workspace,
           size_t workspace_bytes, hipStream_t stream) {
    WT_TRY(wt::ensure_device());
    const Workspace ws = carve(wt::align_ptr(workspace), Policy::kRounds, Policy::kRowCounts, (size_t)L.n_jobs, (size_t)L.n_streams, (size_t)L.n_traj_total,
                               (size_t)L.max_traj);
    WT_TRY(wt::check_workspace_fits(entry, workspace, workspace_bytes, ws.bytes, WT_ERR_CAPACITY));
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    const size_t P = (size_t)L.n_jobs * (size_t)L.n_streams, RS = (size_t)L.r_sets * (size_t)L.n_streams;
    const long long n_traj = (long long)L.n_jobs * L.n_traj_total, n_row = (long long)L.n_jobs * L.n_rows;
    const long long n_init = n_traj > n_row ? n_traj : n_row;
    if (n_init > 0x7fffffffll * 256) { wt::set_error("%s: %d jobs over %lld rows in one call", entry, (int)L.n_jobs, (long long)L.n_rows); return WT_ERR_CAPACITY; }
    if (n_init) hipLaunchKernelGGL(link_init_kernel<PassOutputs>, dim3((unsigned)((n_init + 255) / 256)), dim3(256), 0, stream, O, n_traj, n_row);
    if (P) {
        const Layout& base = L;
        hipLaunchKernelGGL(link_summary_kernel<Policy::kRowCounts>, dim3((unsigned)RS), dim3(kWave), 0, stream, base, ws.sum, (int*)status_dev);
        hipLaunchKernelGGL(match_kernel, dim3((unsigned)P), dim3(kWave), (size_t)L.lds_traj * kTableBytes, stream, L, B, ws, O, (int*)status_dev);
    }
    WT_HIP(hipGetLastError());
    return WT_OK;
}

template <class Policy>
size_t workspace_bytes(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj) {
    if (n_jobs < 0 || n_streams < 0 || n_rows < 0 || n_traj_total < 0 || max_traj < 0) return 0;
    return carve(nullptr, Policy::kRounds, Policy::kRowCounts, (size_t)n_jobs, (size_t)n_streams, (size_t)n_traj_total, (size_t)(max_traj > 0 ? max_traj : 1)).bytes + 256;
}

// the rounds of a finished call of a pass with Policy::kRounds on `workspace` into the host array out_rounds (J, n_streams); it synchronises
inline int read_rounds(const char* entry, const void* workspace, int32_t n_jobs, int32_t n_streams, int32_t* out_rounds) {
    const size_t P = (size_t)(n_jobs > 0 ? n_jobs : 0) * (size_t)(n_streams > 0 ? n_streams : 0);
    if (!workspace || n_jobs < 0 || n_streams < 0 || (P && !out_rounds)) {
        wt::set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if (P) WT_HIP(hipMemcpy(out_rounds, wt::align_ptr(const_cast<void*>(workspace)), 4 * P, hipMemcpyDeviceToHost));
    return WT_OK;
}

struct MoreOut {                              // an output a pass has beyond the five: the caller's array, the device buffer the pass's prepare() allocated, its bytes
    void* host;
    const wt::DevBuf* dev;
    size_t bytes;
};

// Checks the caller's output arrays and the grids, stages a checked host-side input, launches, waits and copies the outputs back:
// the body of a wt_*_tracks_host after its layout check.  prepare(&L, &O) uploads the pass's job arrays and sets the pass's fields
// of L (job_motion among them), and allocates and sets whatever O has beyond the five; `out` holds the caller's five arrays,
// `more` those beyond.
template <class Policy, class PassLayout, class PassOutputs, class MatchKernel, class Prepare>
int run_host(const char* entry, const char* what, MatchKernel match_kernel, const wt::TrackSet& in, int32_t n_jobs, const int32_t* job_result,
             int64_t n_traj_total, int64_t max_traj, Prepare prepare, const Outputs& out, std::initializer_list<MoreOut> more = {}) {
    const size_t nr = (size_t)in.set_row_offsets[in.r_sets], J = (size_t)n_jobs, nt = (size_t)n_traj_total, S = (size_t)in.n_streams;
    bool there = !(J * nt && !(out.pred && out.root && out.affinity)) && !(J * nr && !out.row_root) && !(J * S && !out.links);
    for (const MoreOut& m : more) there = there && (m.host || !m.bytes);
    if (!there) { wt::set_error("%s: bad argument", entry); return WT_ERR_INVALID; }
    WT_TRY(wt::check_track_args(entry, in.n_frames, in.n_streams, in.r_sets, (int64_t)nr, n_traj_total, max_traj, n_jobs, in.n_classes, true,
                                wt::grid_fits(n_jobs, in.n_streams) && wt::grid_fits(in.r_sets, in.n_streams), kGridText, (int)n_jobs, (int)in.r_sets,
                                (int)in.n_streams));
    WT_TRY(wt::ensure_device());
    wt::StagedTrackSet st;
    wt::DevBuf op, oo, oa, orr, ol, dws;
    WT_TRY(st.upload(in, n_jobs, job_result));
    WT_TRY(op.alloc(4 * J * nt)); WT_TRY(oo.alloc(4 * J * nt)); WT_TRY(oa.alloc(8 * J * nt)); WT_TRY(orr.alloc(4 * J * nr));
    WT_TRY(ol.alloc(8 * J * S));
    PassLayout L;
    st.fill(&L, n_traj_total, max_traj, n_jobs, kLdsTraj);
    PassOutputs O;
    static_cast<Outputs&>(O) = {op.as<int32_t>(), oo.as<int32_t>(), oa.as<double>(), orr.as<int32_t>(), ol.as<int64_t>()};
    WT_TRY(prepare(&L, &O));
    const size_t wsb = workspace_bytes<Policy>(n_jobs, in.n_streams, (int64_t)nr, n_traj_total, max_traj);
    WT_TRY(dws.alloc(wsb));
    const Boxes B = {st.dev.x, st.dev.y, st.dev.w, st.dev.h};
    WT_TRY(launch<Policy>(entry, match_kernel, L, B, O, st.status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(st.finish(what, "counts or offsets"));
    if (J * nt) {
        WT_HIP(hipMemcpy(out.pred, op.p, 4 * J * nt, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(out.root, oo.p, 4 * J * nt, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out.affinity, oa.p, 8 * J * nt, hipMemcpyDeviceToHost));
    }
    if (J * nr) WT_HIP(hipMemcpy(out.row_root, orr.p, 4 * J * nr, hipMemcpyDeviceToHost));
    if (J * S) WT_HIP(hipMemcpy(out.links, ol.p, 8 * J * S, hipMemcpyDeviceToHost));
    for (const MoreOut& m : more)
        if (m.bytes) WT_HIP(hipMemcpy(m.host, m.dev->p, m.bytes, hipMemcpyDeviceToHost));
    return WT_OK;
}

}  // namespace link
}  // namespace wtdev
