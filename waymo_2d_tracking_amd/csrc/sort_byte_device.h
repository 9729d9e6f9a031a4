// One frame of one tracker with a second association over low-score detections (ByteTrack, Zhang et al., ECCV 2022; DESIGN.md
// "second association").  The frame of sort_device.h's tracker_step, with step 4 added:
//   1 predict, drop tracks whose predicted box is not finite                                   (sort.py:256-265)
//   2 the caller hands the class's detections as one list: indices 0 .. NH-1 the high ones, NH .. NH+NL-1 the low ones
//   3 associate(H, all predicted tracks, iou_thr)                                              (sort.py:193-230)
//   4 R = the list positions left without a match, ascending; associate(L, predicted boxes of R, low_iou) when both are
//     non-empty; a low detection that stays without a track is dropped
//   5 births from H only; 6 emit newest first, reap                                            (sort.py:276-293)
// Both associations are ONE piece of code run twice (a two-trip loop around one call site of munkres_wave), on the same cost
// buffer, Munkres state, det_match and trk_match: the passes are sequential, so neither LDS nor the per-tracker scratch grows
// beyond the list of remaining positions (`rem`, cap ints).  Kalman filter, IoU and assignment are sort_device.h's own, so
// every number is the one tracker_step would compute from the same operands.  Single wave: no helper waves here.
#pragma once
#include "sort_device.h"

namespace wtdev {

// The cost matrix goes to munkres_wave through a pointer type of this header's own, so that the assignment code is instantiated
// for tracker_step_byte alone: sharing munkres_wave<false, float*> with tracker_step changed the code the compiler emits for the
// plain kernels (and cost them 1.7 % on the 64-segment batch).
struct ByteCostPtr {
    float* p;
    __device__ __forceinline__ float& operator[](int i) const { return p[i]; }
    __device__ __forceinline__ explicit operator float*() const { return p; }
};

// dets.get(k, float[4]) serves k in 0 .. NH+NL-1; M.det_match and the caller's det_idx hold NH+NL <= M.capN entries.
template <class Dets, class Emit>
__device__ int tracker_step_byte(const TrackerMem& M, TrackerState& S, const MunkresMem& L, float* lds_cost, int lds_cost_cap,
                                 const Dets& dets, int NH, int NL, int* rem, double iou_thr, double low_iou, int max_age,
                                 int min_hits, int frame_global, long long id_base, Emit& emit, int* n_births, int* n_rows) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = lanemask_lt();
    const int cap = M.cap;
    S.frame_count += 1;
    // ---- predict; tracks with a non-finite predicted box are dropped (sort.py:256-265) ----
    int T = 0;
    {
        const int T0 = S.n_tracks;
        for (int base = 0; base < T0; base += kWave) {
            const int i = base + lane;
            const bool act = i < T0;
            int slot = 0;
            bool ok = false;
            double b[4] = {0., 0., 0., 0.};
            if (act) {
                slot = M.order[i];
                kalman_predict(M, slot, b);
                const int tsu = M.tsu[slot];
                if (tsu > 0) M.streak[slot] = 0;
                M.tsu[slot] = tsu + 1;
                ok = finite_d(b[0]) && finite_d(b[1]) && finite_d(b[2]) && finite_d(b[3]);
            }
            const unsigned long long good = __ballot(act && ok);
            const unsigned long long bad = __ballot(act && !ok);
            if (act && ok) {
                const int np = T + __popcll(good & lt);
                M.order[np] = slot;
#pragma unroll
                for (int c = 0; c < 4; ++c) M.pbox[c * cap + np] = b[c];
            }
            if (act && !ok) M.freel[S.n_free + __popcll(bad & lt)] = slot;
            T += __popcll(good);
            S.n_free += __popcll(bad);
        }
    }
    for (int i = lane; i < T; i += kWave) M.trk_match[i] = -1;
    for (int k = lane; k < NH + NL; k += kWave) M.det_match[k] = -1;
    wsync();
    // ---- associate twice (sort.py:193-230): pass 0 = H x all tracks, pass 1 = L x remaining tracks ----
    for (int pass = 0; pass < 2; ++pass) {
        const int off = pass ? NH : 0;                     // first detection of the pass in the combined list
        const int N = pass ? NL : NH;
        int Tp = T;
        if (pass) {
            if (N == 0 || T == 0) break;
            Tp = 0;                                        // list positions without a match, ascending, whatever their time_since_update
            for (int base = 0; base < T; base += kWave) {
                const int i = base + lane;
                const bool left = (i < T) && (M.trk_match[i] < 0);
                const unsigned long long mask = __ballot(left);
                if (left) rem[Tp + __popcll(mask & lt)] = i;
                Tp += __popcll(mask);
            }
            wsync();
        }
        if (Tp == 0 || N == 0) continue;
        const double thr = pass ? low_iou : iou_thr;
        const bool transposed = Tp < N;                    // Munkres works on rows <= cols
        const int n = transposed ? Tp : N, m = transposed ? N : Tp;
        const int ld = munkres_ld(m);
        const bool in_lds = (long)n * ld <= (long)lds_cost_cap;
        if (!in_lds && !M.cost_g) return kErrCapacity;
        float* C = in_lds ? lds_cost : M.cost_g;
        // lane = detection, the pass's predicted boxes held lane-wise and broadcast one by one (tracker_step's fill)
        for (int dbase = 0; dbase < N; dbase += kWave) {
            const int d = dbase + lane;
            float db[4] = {0.f, 0.f, 0.f, 0.f};
            if (d < N) dets.get(off + d, db);
            for (int tbase = 0; tbase < Tp; tbase += kWave) {
                const int tl = tbase + lane;
                double tbx[4] = {0., 0., 0., 0.};
                if (tl < Tp) {
                    const int p = pass ? rem[tl] : tl;
#pragma unroll
                    for (int q = 0; q < 4; ++q) tbx[q] = M.pbox[q * cap + p];
                }
                const int tcnt = (Tp - tbase) < kWave ? (Tp - tbase) : kWave;
                for (int tt = 0; tt < tcnt; ++tt) {
                    double tb[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const unsigned long long bits = readlane64((unsigned long long)__double_as_longlong(tbx[q]), tt);
                        tb[q] = __longlong_as_double((long long)bits);
                    }
                    const float v = (float)iou_det_trk(db, tb);      // stored float32 (sort.py:201,205)
                    if (d < N) {
                        const int t = tbase + tt;
                        const int r = transposed ? t : d, c = transposed ? d : t;
                        C[r * ld + c] = -v;                            // linear_assignment(-iou_matrix)
                    }
                }
            }
        }
        wsync();
        MunkresMem L2 = L;
        L2.cost_in_lds = in_lds ? 1 : 0;
        const int rc = in_lds ? munkres_wave<false>(ByteCostPtr{lds_cost}, n, m, ld, L2) : munkres_wave<false>(ByteCostPtr{M.cost_g}, n, m, ld, L2);
        if (rc) return rc;
        for (int d = lane; d < N; d += kWave) {
            const int t = transposed ? L.col_star[d] : L.row_star[d];
            if (t >= 0) {
                const int p = pass ? rem[t] : t;
                float db[4];
                dets.get(off + d, db);
                double tb[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) tb[q] = M.pbox[q * cap + p];
                const float v = (float)iou_det_trk(db, tb);
                if ((double)v < thr) {                                 // sort.py:220 (f32 value vs python float)
                    M.det_match[off + d] = -2;
                } else {
                    M.det_match[off + d] = p;
                    M.trk_match[p] = off + d;
                }
            }
        }
        wsync();
    }
    // ---- update matched tracks, by a high or a low detection alike (sort.py:270-273) ----
    for (int i = lane; i < T; i += kWave) {
        const int d = M.trk_match[i];
        if (d >= 0) {
            const int slot = M.order[i];
            float db[4];
            dets.get(d, db);
            M.tsu[slot] = 0;
            M.streak[slot] = M.streak[slot] + 1;
            kalman_update(M, slot, db);
        }
    }
    // ---- births from H only (sort.py:276-278): never-assigned detections ascending, then threshold-rejected ones ----
    int nb = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int want = pass == 0 ? -1 : -2;
        for (int base = 0; base < NH; base += kWave) {
            const int k = base + lane;
            const bool f = (k < NH) && (M.det_match[k] == want);
            const unsigned long long mask = __ballot(f);
            if (f) M.new_list[nb + __popcll(mask & lt)] = k;
            nb += __popcll(mask);
        }
    }
    if (T + nb > cap || nb > S.n_free) return kErrCapacity;
    wsync();
    for (int k = lane; k < nb; k += kWave) {
        const int slot = M.freel[S.n_free - 1 - k];
        M.order[T + k] = slot;
        float db[4];
        dets.get(M.new_list[k], db);
        track_init(M, slot, db);
        M.gid[slot] = id_base + S.next_local + k;
        M.tsu[slot] = 0;
        M.streak[slot] = 0;
        M.bframe[slot] = frame_global;
        M.bk[slot] = k;
    }
    S.n_free -= nb;
    S.next_local += nb;
    const int T2 = T + nb;
    wsync();
    // ---- emit newest first (sort.py:279-290) ----
    int K = 0;
    for (int top = T2; top > 0; top -= kWave) {
        const int i = top - 1 - lane;
        bool e = false;
        double b[4] = {0., 0., 0., 0.}, conf = 0.;
        int slot = 0;
        if (i >= 0) {
            slot = M.order[i];
            if (M.tsu[slot] < 1 && (M.streak[slot] >= min_hits || S.frame_count <= min_hits)) {
                x_to_bbox(M.kx[0 * cap + slot], M.kx[1 * cap + slot], M.kx[2 * cap + slot], M.kx[3 * cap + slot], b);
                const double err = ((M.kP[0 * cap + slot] + M.kP[8 * cap + slot]) + M.kP[16 * cap + slot]) / 3.0;
                conf = exp(-err * 0.1);
                e = emit.accept(b, conf);
            }
        }
        const unsigned long long mask = __ballot(e);
        if (e) emit.write(K + __popcll(mask & lt), b, conf, M.gid[slot], M.bframe[slot], M.bk[slot]);
        K += __popcll(mask);
    }
    // ---- reap (sort.py:291-293) ----
    int Tn = 0;
    for (int base = 0; base < T2; base += kWave) {
        const int i = base + lane;
        const bool act = i < T2;
        int slot = 0;
        bool live = false;
        if (act) { slot = M.order[i]; live = !(M.tsu[slot] > max_age); }
        const unsigned long long good = __ballot(act && live);
        const unsigned long long bad = __ballot(act && !live);
        if (act && live) M.order[Tn + __popcll(good & lt)] = slot;
        if (act && !live) M.freel[S.n_free + __popcll(bad & lt)] = slot;
        Tn += __popcll(good);
        S.n_free += __popcll(bad);
    }
    S.n_tracks = Tn;
    *n_births = nb;
    *n_rows = K;
    wsync();
    return 0;
}

}  // namespace wtdev
