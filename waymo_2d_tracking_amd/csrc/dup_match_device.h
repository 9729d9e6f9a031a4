// Suppression of trajectories that are the same object, shared by track_dedup.hip (duplicates inside a class, DESIGN.md section
// 23) and track_xclass.hip (duplicates across classes, section 26): the summary of a (result, stream), the match of a
// (job, stream) in rounds without a table of pairs, the workspace both carve and the three launches.  What differs between the
// two passes is a Policy, a small struct the match is compiled for - no flag is read at run time on its account:
//   static Policy make(const Layout& L, int job, const int32_t* n, const double* ssum, const int32_t* cls)   the job's parameters; n, ssum
//                                                       and cls are the row counts, score sums and classes of the stream's
//                                                       trajectories by local index
//   int  live_class(int c)                              c when a trajectory of class c can be in a pair at all, 0 otherwise
//   bool pair_live(int ca, int cb)                      whether two live classes are compared
//   double threshold(int ca, int cb)                    what the measure of two boxes has to reach in a slot
//   int  frames(int ca, int cb)                         the slots that have to match
//   double measure(const double a[4], const double b[4])   of two boxes [x1, y1, x2, y2]; a slot matches when v >= threshold and v > 0
//   bool stronger(int t, int u)                         a strict total order of the stream's trajectories
//   double need(int ca, int cb, int strong, int weak)   what (double)m has to reach
// Two launches, one 64-lane wavefront per independent problem:
//   1. summary: per (result, stream), walk the slots once, the rows of a slot lane-parallel: per trajectory its row count, score
//               sum (row after row in slot order), class and first row; per row its slot and the distance in rows to the previous
//               and next row of its trajectory.  Shared by all jobs of the result; it does not depend on the policy.
//   2. match:   per (job, stream), in rounds.  A round walks the slots; a lane takes a row of the slot and meets every later row
//               of it (64 of them at a time, held in registers and passed from lane to lane).  A pair of rows whose boxes match
//               belongs to its lanes only at the pair's FIRST matching slot (both chains are walked back until an earlier
//               matching slot or their start); the owner walks both chains forward as a merge join for m and decides whether the
//               two trajectories are the same object.  A trajectory is undecided, kept or suppressed: a pair whose stronger side
//               is kept proposes it as suppressor (compare-and-swap, the stronger proposal stays), one whose stronger side is
//               undecided marks the weaker side pending.  After the sweep an undecided trajectory that is not pending is
//               suppressed when it has a proposal and kept otherwise.  The strongest undecided trajectory is never pending -
//               whatever the strict total order is - so every round decides one: the rounds are bounded by the longest chain,
//               and by T.  The same wavefront then writes by, match, the row mask and the count.
// The tables of the match (12 bytes per trajectory) live in LDS up to kLdsTraj trajectories, in the workspace beyond.
// Include it only from units compiled with -ffp-contract=off.
#pragma once
#include "eval_device.h"
#include "tracks_device.h"
#include "tracks_host.h"

namespace wtdev {
namespace dup {

constexpr int kLdsTraj = 1024;                // trajectories of one (result, stream) up to which the match tables stay in LDS
constexpr int kTableBytes = 12;               // per trajectory: three int32
constexpr int kUndecided = 0, kKept = 1, kSuppressed = 2;

struct Layout : TrackLayout {                 // device pointers; a pass's Layout is this plus its own job parameters
    const double* score;
};

struct Summary {
    int32_t *n, *cls, *first_row, *last_row;  // [n_traj_total]; rows relative to the stream's first row, -1 none
    double* ssum;                             // [n_traj_total]
    int32_t *back, *fwd, *slot;               // [n_rows]; rows from this one to the previous / next row of its trajectory, 0 = none
};

struct Workspace {
    int32_t* rounds;                          // [J * n_streams] the sweeps the match of each problem took; first in the workspace
    Summary sum;
    int32_t *state, *prop, *pend;             // [J * n_traj_total] the tables of the problems above kLdsTraj
    size_t bytes;
};

inline Workspace carve(void* base, size_t n_jobs, size_t n_streams, size_t n_rows, size_t n_traj_total, size_t max_traj) {
    wt::Carver cv(base);
    Workspace w;
    const size_t big = max_traj > (size_t)kLdsTraj ? n_jobs * n_traj_total : 0;
    w.rounds = cv.take<int32_t>(n_jobs * n_streams + 1);
    w.sum.n = cv.take<int32_t>(n_traj_total + 1);
    w.sum.cls = cv.take<int32_t>(n_traj_total + 1);
    w.sum.first_row = cv.take<int32_t>(n_traj_total + 1);
    w.sum.last_row = cv.take<int32_t>(n_traj_total + 1);
    w.sum.ssum = cv.take<double>(n_traj_total + 1);
    w.sum.back = cv.take<int32_t>(n_rows + 1);
    w.sum.fwd = cv.take<int32_t>(n_rows + 1);
    w.sum.slot = cv.take<int32_t>(n_rows + 1);
    w.state = cv.take<int32_t>(big + 1);
    w.prop = cv.take<int32_t>(big + 1);
    w.pend = cv.take<int32_t>(big + 1);
    w.bytes = cv.off;
    return w;
}

static __global__ __launch_bounds__(kWave) void dup_summary_kernel(Layout L, Summary S, int* __restrict__ status) {
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
        S.n[g] = 0; S.cls[g] = 0; S.first_row[g] = -1; S.last_row[g] = -1; S.ssum[g] = 0.0;
    }
    wsync();
    int err = 0;
    for_stream_rows(q, L.local, &err, [&](long long d, int t, int fo) {
        S.back[d] = 0; S.fwd[d] = 0; S.slot[d] = fo;
        const size_t g = (size_t)q.t0 + t;
        const int row = (int)(d - q.rs0), prev = S.last_row[g];
        if (prev < 0) {
            S.first_row[g] = row;
            S.cls[g] = L.category[d];
        } else {
            S.back[d] = row - prev;
            S.fwd[q.rs0 + prev] = row - prev;
        }
        S.last_row[g] = row;
        S.n[g] = S.n[g] + 1;
        S.ssum[g] = S.ssum[g] + L.score[d];                            // one by one in slot order
    });
    if (__ballot(err != 0) != 0ull && lane == 0) atomicMax(status, kErrCapacity);
}

struct Outputs {
    int32_t *keep, *by, *match;               // [J * n_traj_total]
    int32_t* row_keep;                        // [J * n_rows]
    int64_t* dropped;                         // [J * n_streams]
};

// every entry: not named; the match kernel fills those of its job's result
static __global__ void dup_init_kernel(Outputs O, long long n_traj, long long n_row) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_traj) { O.keep[i] = -1; O.by[i] = -1; O.match[i] = -1; }
    if (i < n_row) O.row_keep[i] = -1;
}

// The chains of one stream: rows as absolute indices inside [rs0, end); -1 = the chain has ended.
struct Chains {
    const int32_t *back, *fwd, *slot;
    long long rs0, end;
    __device__ __forceinline__ long long prev(long long d) const {
        const int b = back[d];
        return b > 0 && d - b >= rs0 ? d - b : -1;
    }
    __device__ __forceinline__ long long next(long long d) const {
        const int f = fwd[d];
        return f > 0 && d + f < end ? d + f : -1;
    }
};

template <class Policy>
__device__ __forceinline__ bool boxes_match(const Policy& P, const Boxes& B, long long a, long long b, double thr) {
    double ba[4], bb[4];
    B.get(a, ba);
    B.get(b, bb);
    const double v = P.measure(ba, bb);
    return v >= thr && v > 0.;
}

// m of the two chains from rows a and b on: the slots that hold a row of both whose boxes match
template <class Policy>
__device__ __forceinline__ int count_matches(const Policy& P, const Chains& ch, const Boxes& B, long long a, long long b, double thr) {
    int m = 0;
    while (a >= 0 && b >= 0) {
        const int sa = ch.slot[a], sb = ch.slot[b];
        if (sa == sb) {
            m += boxes_match(P, B, a, b, thr) ? 1 : 0;
            a = ch.next(a);
            b = ch.next(b);
        } else if (sa < sb) {
            a = ch.next(a);
        } else {
            b = ch.next(b);
        }
    }
    return m;
}

// whether a slot before the one of rows a and b holds a row of both whose boxes match
template <class Policy>
__device__ __forceinline__ bool matched_before(const Policy& P, const Chains& ch, const Boxes& B, long long a, long long b, double thr) {
    a = ch.prev(a);
    b = ch.prev(b);
    while (a >= 0 && b >= 0) {
        const int sa = ch.slot[a], sb = ch.slot[b];
        if (sa == sb) {
            if (boxes_match(P, B, a, b, thr)) return true;
            a = ch.prev(a);
            b = ch.prev(b);
        } else if (sa > sb) {
            a = ch.prev(a);
        } else {
            b = ch.prev(b);
        }
    }
    return false;
}

// The match of problem blockIdx.x = (job, stream) by one wavefront; smem: lds_traj * kTableBytes bytes of dynamic LDS.
template <class Policy, class PassLayout>
__device__ __forceinline__ void match_problem(const PassLayout& L, const Boxes& B, const Workspace& ws, const Outputs& O, int* __restrict__ status, char* smem) {
    const int lane = threadIdx.x & 63;
    const size_t p = blockIdx.x;
    int j_, s_;
    decode_job_stream(p, L.n_streams, &j_, &s_);
    const int job = j_, s = s_;
    const Span q = span_of(L, L.job_result[job], s);
    if (!q.ok) {
        if (lane == 0) { atomicMax(status, kErrCapacity); O.dropped[p] = 0; ws.rounds[p] = 0; }
        return;
    }
    const int T = q.T;
    const Summary S = ws.sum;
    const size_t g0 = (size_t)q.t0;
    const size_t tbase = (size_t)job * (size_t)L.n_traj_total + g0;
    const size_t lbase = (size_t)job * (size_t)L.n_rows;
    const bool in_lds = T <= L.lds_traj;
    const size_t stride = (size_t)L.lds_traj;
    int32_t* state = in_lds ? reinterpret_cast<int32_t*>(smem) : ws.state + tbase;
    int32_t* prop = in_lds ? state + stride : ws.prop + tbase;          // the strongest kept match proposed so far, -1 none
    int32_t* pend = in_lds ? prop + stride : ws.pend + tbase;           // 1: a stronger match is still undecided
    const Policy P = Policy::make(L, job, S.n + g0, S.ssum + g0, S.cls + g0);
    int err = 0;
    const long long end = stream_end(q, &err);
    const Chains ch = {S.back, S.fwd, S.slot, q.rs0, end};
    for (int t = lane; t < T; t += kWave) { state[t] = kUndecided; prop[t] = -1; pend[t] = 0; }
    wsync();

    // the class of trajectory t when the job can put it in a pair, 0 otherwise
    auto live_class = [&](int t) { return P.live_class(S.cls[g0 + t]); };

    int rounds = 0;
    bool undecided = T > 0 && !err;
    for (int round = 0; round <= T && undecided; ++round) {    // every round decides a trajectory: at most T rounds
        ++rounds;
        for (long long f = q.f0; f < q.f1; ++f) {
            long long r0, r1;
            if (!slot_rows(q, f, &r0, &r1) || r1 > end) { err = kErrCapacity; break; }
            for (long long b = r0; b + 1 < r1; b += kWave) {
                const long long di = b + lane;
                int ti = -1, ci = 0, si = kSuppressed;
                double bi[4] = {0., 0., 0., 0.};
                if (di < r1) {
                    ti = L.local[di];
                    if (ti < 0 || ti >= T) { err = kErrCapacity; ti = -1; }
                    else { ci = live_class(ti); si = state[ti]; B.get(di, bi); }
                }
                const bool active = ti >= 0 && ci > 0 && si != kSuppressed;  // a suppressed trajectory neither suppresses nor is asked again
                if (__ballot(active) == 0ull) continue;
                for (long long jb = b; jb < r1; jb += kWave) {              // the later rows of the slot, 64 at a time in registers
                    const long long dl = jb + lane;
                    int tl = -1, cl = 0, sl = kSuppressed;
                    double bl[4] = {0., 0., 0., 0.};
                    if (dl < r1) {
                        tl = L.local[dl];
                        if (tl < 0 || tl >= T) { err = kErrCapacity; tl = -1; }
                        else { cl = live_class(tl); sl = state[tl]; B.get(dl, bl); }
                    }
                    unsigned long long live = __ballot(tl >= 0 && cl > 0 && sl != kSuppressed);
                    while (live) {                                          // the same row for every lane
                        const int jj = __builtin_ctzll(live);
                        live &= live - 1ull;
                        const long long dj = jb + jj;
                        const int tj = __builtin_amdgcn_readlane(tl, jj), cj = __builtin_amdgcn_readlane(cl, jj), sj = __builtin_amdgcn_readlane(sl, jj);
                        const double bj[4] = {bcast_d(bl[0], jj), bcast_d(bl[1], jj), bcast_d(bl[2], jj), bcast_d(bl[3], jj)};
                        if (!active || dj <= di || !P.pair_live(ci, cj) || tj == ti || (si != kUndecided && sj != kUndecided)) continue;
                        const double thr = P.threshold(ci, cj);
                        const double a = P.measure(bi, bj);                   // in registers: before anything that reads memory
                        if (!(a >= thr && a > 0.)) continue;
                        const bool i_strong = P.stronger(ti, tj);
                        const int strong = i_strong ? ti : tj, weak = i_strong ? tj : ti;
                        if ((i_strong ? sj : si) != kUndecided) continue;     // the weaker side is decided: nothing to do
                        if (matched_before(P, ch, B, di, dj, thr)) continue;  // the pair belongs to its first matching slot
                        const int m = count_matches(P, ch, B, di, dj, thr);
                        const double need = P.need(i_strong ? ci : cj, i_strong ? cj : ci, strong, weak);
                        if (m < P.frames(ci, cj) || !((double)m >= need)) continue;
                        if ((i_strong ? si : sj) == kKept) {
                            int cur = prop[weak];
                            while (cur < 0 || (cur != strong && P.stronger(strong, cur))) {
                                const int old = atomicCAS(&prop[weak], cur, strong);
                                if (old == cur) break;
                                cur = old;
                            }
                        } else {
                            pend[weak] = 1;
                        }
                    }
                }
            }
        }
        wsync();
        undecided = false;
        for (int tb = 0; tb < T; tb += kWave) {
            const int t = tb + lane;
            bool left = false;
            if (t < T && state[t] == kUndecided) {
                if (pend[t]) { pend[t] = 0; left = true; }
                else state[t] = prop[t] >= 0 ? kSuppressed : kKept;
            }
            undecided = undecided || __ballot(left) != 0ull;
        }
        wsync();
        if (undecided && round == T) err = kErrCapacity;               // cannot happen: the strongest undecided one is never pending
        if (__ballot(err != 0) != 0ull) break;
    }

    // ---- by, match, count, row mask ----
    long long n_dropped = 0;
    for (int t = lane; t < T; t += kWave) {
        const bool gone = state[t] == kSuppressed;
        int by = -1, m = 0;
        if (gone) {
            by = prop[t];
            const int c = live_class(t), cb = by >= 0 && by < T ? live_class(by) : 0;
            const int fa = S.first_row[g0 + t], fb = by >= 0 && by < T ? S.first_row[g0 + by] : -1;
            if (c > 0 && cb > 0 && fa >= 0 && fb >= 0 && q.rs0 + fa < end && q.rs0 + fb < end)
                m = count_matches(P, ch, B, q.rs0 + fa, q.rs0 + fb, P.threshold(c, cb));
            else
                err = kErrCapacity;
        }
        O.keep[tbase + t] = gone ? 0 : 1;
        O.by[tbase + t] = by;
        O.match[tbase + t] = m;
        n_dropped += gone;
    }
    for (int o = 32; o > 0; o >>= 1) n_dropped += __shfl_xor(n_dropped, o, kWave);
    for (long long d = q.rs0 + lane; d < end; d += kWave) {
        const int t = L.local[d];
        if (t < 0 || t >= T) { err = kErrCapacity; continue; }
        O.row_keep[lbase + d] = state[t] == kSuppressed ? 0 : 1;
    }
    if (__ballot(err != 0) != 0ull && lane == 0) atomicMax(status, kErrCapacity);
    if (lane == 0) { O.dropped[p] = n_dropped; ws.rounds[p] = rounds; }
}

// The three launches of a pass on `stream`; match_kernel(L, B, ws, O, status) is the pass's instantiation of match_problem.
template <class PassLayout, class MatchKernel>
int launch(const char* entry, MatchKernel match_kernel, const PassLayout& L, const Boxes& B, const Outputs& O, int32_t* status_dev, void* workspace,
           size_t workspace_bytes, hipStream_t stream) {
    WT_TRY(wt::ensure_device());
    const Workspace ws = carve(wt::align_ptr(workspace), (size_t)L.n_jobs, (size_t)L.n_streams, (size_t)L.n_rows, (size_t)L.n_traj_total, (size_t)L.max_traj);
    WT_TRY(wt::check_workspace_fits(entry, workspace, workspace_bytes, ws.bytes, WT_ERR_CAPACITY));
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    const size_t P = (size_t)L.n_jobs * (size_t)L.n_streams, RS = (size_t)L.r_sets * (size_t)L.n_streams;
    const long long n_traj = (long long)L.n_jobs * L.n_traj_total, n_row = (long long)L.n_jobs * L.n_rows;
    const long long n_init = n_traj > n_row ? n_traj : n_row;
    if (n_init > 0x7fffffffll * 256) { wt::set_error("%s: %d jobs over %lld rows in one call", entry, (int)L.n_jobs, (long long)L.n_rows); return WT_ERR_CAPACITY; }
    if (n_init) hipLaunchKernelGGL(dup_init_kernel, dim3((unsigned)((n_init + 255) / 256)), dim3(256), 0, stream, O, n_traj, n_row);
    if (P) {
        const Layout& base = L;
        hipLaunchKernelGGL(dup_summary_kernel, dim3((unsigned)RS), dim3(kWave), 0, stream, base, ws.sum, (int*)status_dev);
        hipLaunchKernelGGL(match_kernel, dim3((unsigned)P), dim3(kWave), (size_t)L.lds_traj * kTableBytes, stream, L, B, ws, O, (int*)status_dev);
    }
    WT_HIP(hipGetLastError());
    return WT_OK;
}

inline size_t workspace_bytes(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj) {
    if (n_jobs < 0 || n_streams < 0 || n_rows < 0 || n_traj_total < 0 || max_traj < 0) return 0;
    return carve(nullptr, (size_t)n_jobs, (size_t)n_streams, (size_t)n_rows, (size_t)n_traj_total, (size_t)(max_traj > 0 ? max_traj : 1)).bytes + 256;
}

// the rounds of a finished call on `workspace` into the host array out_rounds (J, n_streams); it synchronises
inline int read_rounds(const char* entry, const void* workspace, int32_t n_jobs, int32_t n_streams, int32_t* out_rounds) {
    const size_t P = (size_t)(n_jobs > 0 ? n_jobs : 0) * (size_t)(n_streams > 0 ? n_streams : 0);
    if (!workspace || n_jobs < 0 || n_streams < 0 || (P && !out_rounds)) {
        wt::set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if (P) WT_HIP(hipMemcpy(out_rounds, wt::align_ptr(const_cast<void*>(workspace)), 4 * P, hipMemcpyDeviceToHost));
    return WT_OK;
}

// Stages a checked host-side input, launches, waits and copies the five outputs back: the body of a wt_*_tracks_host after its
// own checks.  upload_jobs(&L) uploads the pass's job arrays and sets the pass's fields of L.
template <class PassLayout, class MatchKernel, class UploadJobs>
int run_host(const char* entry, const char* what, MatchKernel match_kernel, const wt::TrackSet& in, int32_t n_jobs, const int32_t* job_result,
             int64_t n_traj_total, int64_t max_traj, UploadJobs upload_jobs, int32_t* out_keep, int32_t* out_by, int32_t* out_match,
             int32_t* out_row_keep, int64_t* out_dropped) {
    const size_t nr = (size_t)in.set_row_offsets[in.r_sets], J = (size_t)n_jobs, nt = (size_t)n_traj_total, S = (size_t)in.n_streams;
    WT_TRY(wt::ensure_device());
    wt::StagedTrackSet st;
    wt::DevBuf ok, ob, om, orr, od, dws;
    WT_TRY(st.upload(in, n_jobs, job_result));
    PassLayout L;
    st.fill(&L, n_traj_total, max_traj, n_jobs, kLdsTraj);
    L.score = st.dev.score;
    WT_TRY(upload_jobs(&L));
    WT_TRY(ok.alloc(4 * J * nt)); WT_TRY(ob.alloc(4 * J * nt)); WT_TRY(om.alloc(4 * J * nt)); WT_TRY(orr.alloc(4 * J * nr));
    WT_TRY(od.alloc(8 * J * S));
    const size_t wsb = workspace_bytes(n_jobs, in.n_streams, (int64_t)nr, n_traj_total, max_traj);
    WT_TRY(dws.alloc(wsb));
    const Boxes B = {st.dev.x, st.dev.y, st.dev.w, st.dev.h};
    const Outputs O = {ok.as<int32_t>(), ob.as<int32_t>(), om.as<int32_t>(), orr.as<int32_t>(), od.as<int64_t>()};
    WT_TRY(launch(entry, match_kernel, L, B, O, st.status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(st.finish(what, "counts or offsets"));
    if (J * nt) {
        WT_HIP(hipMemcpy(out_keep, ok.p, 4 * J * nt, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(out_by, ob.p, 4 * J * nt, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_match, om.p, 4 * J * nt, hipMemcpyDeviceToHost));
    }
    if (J * nr) WT_HIP(hipMemcpy(out_row_keep, orr.p, 4 * J * nr, hipMemcpyDeviceToHost));
    if (J * S) WT_HIP(hipMemcpy(out_dropped, od.p, 8 * J * S, hipMemcpyDeviceToHost));
    return WT_OK;
}

}  // namespace dup
}  // namespace wtdev
