// HOTA (Luiten et al., IJCV 2021: DetA / AssA / LocA over 19 localisation thresholds) of tracking results on gfx950
// (include/waymotrack.h, "MOT HOTA evaluation"; DESIGN.md section 19 has the definition).
//
// Same shape as mot_eval.hip and mot_identity.hip, with the difficulty level in the block index: one 64-lane wavefront owns
// one (result set k, stream s, class c, level) and runs the same code on that level's boxes (LEVEL_1 = ground truth without
// the level-2 rows, hypotheses without those that only reach a removed box; the rule is evaluated per frame as the wave walks).
//   staging          per frame and pass, the boxes and trajectory indices of the frame's rows go to LDS once (workspace when a frame
//                    can hold more than kStageRows boxes a side): the looped side of every sweep below is a broadcast read.
//   alignment pass   walk the frames in order, compact the class's rows, row[i] with lane = ground-truth row over the hypotheses,
//                    col[j] with lane = hypothesis over the ground-truth rows: both sums run in file order without a cross-lane
//                    reduction.  Where S > 0, one lane adds S / ((row + col) - S) to the float64 cell (trajectory of the object,
//                    trajectory of the hypothesis) of the problem's matrix P: plain load / add / store, a cell gets at most one
//                    addend per frame and one wave walks the frames in order.  P becomes A = P / ((cg + ch) - P) in place.
//   matching pass    per frame the float32 matrix (float)(A * S), the Munkres of sort_device.h on its negative (LDS when it fits,
//                    workspace otherwise), and for every pair kept the number b of thresholds its IoU passes: lane a keeps tp[a]
//                    and loc[a] (matches added one after the other in ground-truth row order), the cell's histogram takes b.
//   association      lanes stride over the cells, suffix-sum the histogram to the 19 counts c_a and add the three terms per
//                    threshold; the 64 partial sums are added in lane order.
// Compile with -ffp-contract=off (IoU in the operation order of tracking/sort/sort.py:34-47; eval_device.h has it).
#include "eval_device.h"
#include "eval_host.h"

using namespace wtdev;

namespace {

constexpr int kMaxBoxes = 4096;               // per side and (frame, class): the limit of munkres_wave
constexpr int kMaxTraj = 4096;                // trajectories per side of one problem
constexpr int kMaxStreamFrames = 65535;       // a cell's histogram entry is a uint16 and grows by at most one per frame
constexpr int kAlphas = 19;                   // alpha_a = (a + 1) / 20
constexpr int kLdsCostFloats = 8192;          // 32 KiB of cost matrix in LDS per wave, the share of mot_eval.hip
constexpr size_t kLdsZmaskMax = 32 * 1024;    // zero bitmaps stay in LDS up to here, in the workspace beyond
constexpr int kPartDoubles = 3 * kAlphas * kWave;   // per-lane partial association sums of one wave
constexpr int kStageRows = 256;               // the frame's boxes and trajectory indices are staged in LDS up to this many a side

struct Caps {
    int capN;                // boxes per side of one (frame, class)
    int capG, capH;          // trajectories per side of one problem
    int lds_cost;            // floats of cost matrix in LDS
    bool cost_g, zmask_g, stage_g;
    size_t lds_bytes;
};

struct Workspace {                       // device pointers carved from one block; everything but P / hist is [wave][cap]
    int *gidx, *hidx;                    // [capN] rows of this class in the frame, relative to the frame's first row
    int *gsel, *hsel, *hkeep;            // [capN] LEVEL_1: the rows that stay, and the per-hypothesis flag of the removal rule
    double* rowsum;                      // [capN] row[i] of the frame
    int *cg, *ch;                        // [capG], [capH] boxes per trajectory at the wave's level
    float* cost_g;                       // [capN * (capN | 1)] when the matrix can outgrow the LDS share
    unsigned long long* zmask_g;         // [capN * ceil(capN / 64)] when the bitmaps can
    double* part;                        // [3 * 19 * 64]
    double* stage_box;                   // [2 * capN * 4] the frame's boxes [x1, y1, x2, y2], ground truth then hypotheses, when capN > kStageRows
    int* stage_traj;                     // [2 * capN] their trajectory indices
    double* P;                           // every problem's two n_g x n_h matrices (LEVEL_1, LEVEL_2), at mat_offsets[p]
    uint16_t* hist;                      // 19 per cell of P: matches of the cell that pass exactly b = index + 1 thresholds (used where A > 0)
    size_t bytes;
};

int pick_caps(int64_t max_frame_boxes, int64_t max_gt_traj, int64_t max_hyp_traj, Caps* c) {
    if (max_frame_boxes > kMaxBoxes) {
        wt::set_error("%lld boxes of one class in one frame: the assignment kernel takes at most %d a side", (long long)max_frame_boxes, kMaxBoxes);
        return WT_ERR_CAPACITY;
    }
    if (max_gt_traj > kMaxTraj || max_hyp_traj > kMaxTraj) {
        wt::set_error("%lld trajectories of one class in one stream: the HOTA kernel takes at most %d a side",
                      (long long)std::max(max_gt_traj, max_hyp_traj), kMaxTraj);
        return WT_ERR_CAPACITY;
    }
    if (max_frame_boxes < 0 || max_gt_traj < 0 || max_hyp_traj < 0) { wt::set_error("wt_mot_hota: a box or trajectory count is negative"); return WT_ERR_INVALID; }
    c->capN = (int)(max_frame_boxes > 0 ? max_frame_boxes : 1);
    c->capG = (int)(max_gt_traj > 0 ? max_gt_traj : 1);
    c->capH = (int)(max_hyp_traj > 0 ? max_hyp_traj : 1);
    const int64_t full = (int64_t)c->capN * (c->capN | 1);
    c->lds_cost = (int)(full < kLdsCostFloats ? full : kLdsCostFloats);
    c->cost_g = full > kLdsCostFloats;
    const size_t W = (size_t)(c->capN + 63) / 64;
    c->zmask_g = (size_t)c->capN * W * 8 > kLdsZmaskMax;
    const size_t stars = wt::align_up((size_t)3 * c->capN * sizeof(int), 16);
    c->stage_g = c->capN > kStageRows;
    const size_t stage = c->stage_g ? 0 : wt::align_up((size_t)2 * c->capN * (4 * sizeof(double) + sizeof(int)), 16);
    c->lds_bytes = wt::align_up((size_t)c->lds_cost * sizeof(float), 16) + stars + (c->zmask_g ? 0 : (size_t)c->capN * W * 8) + stage + 16;
    return WT_OK;
}

Workspace carve(void* base, size_t n_waves, const Caps& c, size_t matrix_cells) {
    wt::Carver cv(base);
    Workspace w;
    const size_t W = (size_t)(c.capN + 63) / 64;
    w.gidx = cv.take<int>(n_waves * c.capN);
    w.hidx = cv.take<int>(n_waves * c.capN);
    w.gsel = cv.take<int>(n_waves * c.capN);
    w.hsel = cv.take<int>(n_waves * c.capN);
    w.hkeep = cv.take<int>(n_waves * c.capN);
    w.rowsum = cv.take<double>(n_waves * c.capN);
    w.cg = cv.take<int>(n_waves * c.capG);
    w.ch = cv.take<int>(n_waves * c.capH);
    w.cost_g = cv.take<float>(c.cost_g ? n_waves * (size_t)c.capN * (c.capN | 1) : 1);
    w.zmask_g = cv.take<unsigned long long>(c.zmask_g ? n_waves * (size_t)c.capN * W : 1);
    w.part = cv.take<double>(n_waves * kPartDoubles);
    w.stage_box = cv.take<double>(c.stage_g ? n_waves * (size_t)c.capN * 8 : 1);
    w.stage_traj = cv.take<int>(c.stage_g ? n_waves * (size_t)c.capN * 2 : 1);
    w.P = cv.take<double>(matrix_cells ? matrix_cells : 1);
    w.hist = cv.take<uint16_t>(matrix_cells ? matrix_cells * kAlphas : 1);
    w.bytes = cv.off;
    return w;
}

// alpha_a in float64; the quotient is correctly rounded on the device and on the host alike
__device__ __forceinline__ double alpha_of(int a) { return (double)(a + 1) / 20.0; }

// wave = (problem p, level): the level is the fastest index; level 0 = LEVEL_1, 1 = LEVEL_2
__device__ __forceinline__ void decode_wave(size_t b, size_t* p, int* lv) {
    *p = b >> 1;
    *lv = (int)(b & 1);
}

struct FrameRows {           // the frame's rows of the wave's class and level, as offsets from the frame's first row, in file order
    int ng, nh;
    const int *g, *h;
};

__global__ __launch_bounds__(kWave) void mot_hota_kernel(
    Boxes G, const int32_t* __restrict__ g_cat, const int32_t* __restrict__ g_level, const int32_t* __restrict__ g_traj,
    const int64_t* __restrict__ frame_gt_offsets, const int64_t* __restrict__ stream_frame_offsets, long long n_frames,
    int n_streams, int C, const int64_t* __restrict__ set_row_offsets, const int64_t* __restrict__ frame_hyp_offsets,
    Boxes H, const int32_t* __restrict__ h_cat, const int32_t* __restrict__ h_traj,
    const int32_t* __restrict__ g_ntraj, const int32_t* __restrict__ h_ntraj, const int64_t* __restrict__ mat_offsets,
    long long matrix_cells, Thresholds thr_all, Caps caps, Workspace ws,
    int64_t* __restrict__ hota_counts, double* __restrict__ hota_sums, int64_t* __restrict__ hyp_match, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const size_t wv = blockIdx.x;
    size_t p;
    int lv, k, s, c;
    decode_wave(wv, &p, &lv);
    decode_problem(p, n_streams, C, &k, &s, &c);
    const int capN = caps.capN;
    const double thr = thr_all.v[c - 1];
    const int nG = g_ntraj[(size_t)s * C + (c - 1)], nH = h_ntraj[p];
    const long long cells = (long long)nG * nH;
    const long long mo0 = mat_offsets[p], mo1 = mat_offsets[p + 1];
    const long long f0 = stream_frame_offsets[s], f1 = stream_frame_offsets[s + 1];
    int err = 0;
    if (nG < 0 || nH < 0 || nG > caps.capG || nH > caps.capH || mo0 < 0 || mo1 > matrix_cells || mo1 - mo0 < 2 * cells ||
        f1 - f0 > kMaxStreamFrames) err = kErrCapacity;
    if (err) { if (lane == 0) atomicMax(status, err); return; }

    float* lds_cost = reinterpret_cast<float*>(smem);
    char* mk = smem + (((size_t)caps.lds_cost * sizeof(float) + 15) / 16) * 16;
    MunkresMem L;
    L.row_star = reinterpret_cast<int*>(mk);
    L.row_prime = L.row_star + capN;
    L.col_star = L.row_star + 2 * capN;
    const size_t Wcap = (size_t)(capN + 63) / 64;
    L.zmask = caps.zmask_g ? ws.zmask_g + wv * (size_t)capN * Wcap
                           : reinterpret_cast<unsigned long long*>(mk + (((size_t)3 * capN * sizeof(int) + 15) / 16) * 16);
    L.help = nullptr;
    L.cost_in_lds = 0;
    // the frame's boxes and trajectory indices, staged once per frame: behind the bitmaps' share in LDS, or in the workspace
    char* st = mk + (((size_t)3 * capN * sizeof(int) + 15) / 16) * 16 + (caps.zmask_g ? 0 : (size_t)capN * Wcap * 8);
    double* sgb = caps.stage_g ? ws.stage_box + wv * (size_t)capN * 8 : reinterpret_cast<double*>(st);
    double* shb = sgb + (size_t)capN * 4;
    int* sgt = caps.stage_g ? ws.stage_traj + wv * (size_t)capN * 2 : reinterpret_cast<int*>(st + (size_t)capN * 8 * sizeof(double));
    int* sht = sgt + capN;

    int* gidx = ws.gidx + wv * capN;
    int* hidx = ws.hidx + wv * capN;
    int* gsel = ws.gsel + wv * capN;
    int* hsel = ws.hsel + wv * capN;
    int* hkeep = ws.hkeep + wv * capN;
    double* rowsum = ws.rowsum + wv * capN;
    int* cg = ws.cg + wv * (size_t)caps.capG;
    int* ch = ws.ch + wv * (size_t)caps.capH;
    float* cost_g = caps.cost_g ? ws.cost_g + wv * (size_t)capN * (capN | 1) : nullptr;
    double* part = ws.part + wv * (size_t)kPartDoubles;
    double* Pm = ws.P + mo0 + (long long)lv * cells;                  // n_g x n_h, row = trajectory of the object
    uint16_t* hist = ws.hist + (mo0 + (long long)lv * cells) * kAlphas;
    for (long long i = lane; i < cells; i += kWave) Pm[i] = 0.;
    for (int i = lane; i < nG; i += kWave) cg[i] = 0;
    for (int i = lane; i < nH; i += kWave) ch[i] = 0;
    wsync();

    const long long hbase = set_row_offsets[k];
    const int64_t* fho = frame_hyp_offsets + (size_t)k * (size_t)(n_frames + 1);

    // The frame's rows at the wave's level.  LEVEL_2: the class's rows.  LEVEL_1: ground truth without the level-2 rows, hypotheses
    // without those that reach thr with a removed box of the frame and with no counted one.  ng < 0: more rows than the caller said.
    auto frame_rows = [&](long long g0, long long g1, long long h0, long long h1) {
        FrameRows r;
        r.g = gidx;
        r.h = hidx;
        const int ng = compact_rows(g_cat, g0, g1, c, gidx, capN);
        const int nh = compact_rows(h_cat, h0, h1, c, hidx, capN);
        r.ng = ng;
        r.nh = nh;
        if (ng > capN || nh > capN) { r.ng = -1; return r; }
        if (lv == 1 || ng == 0) return r;
        wsync();
        bool any_dc = false;
        for (int base = 0; base < ng; base += kWave) {
            const int i = base + lane;
            any_dc = any_dc || (i < ng && g_level[g0 + gidx[i]] == 2);
        }
        if (__ballot(any_dc) == 0ull) return r;                        // nothing is removed in this frame
        for (int cbase = 0; cbase < nh; cbase += kWave) {                // lane = hypothesis, ground-truth rows one after the other
            const int jj = cbase + lane;
            const bool act = jj < nh;
            double hb[4] = {0., 0., 0., 0.};
            if (act) H.get(h0 + hidx[jj], hb);
            bool hit_counted = false, hit_dc = false;
            for (int ii = 0; ii < ng; ++ii) {
                const long long grow = g0 + uni(gidx[ii]);
                double gb[4];
                G.get(grow, gb);
                const bool easy = g_level[grow] != 2;
                if (act && iou_dd(gb, hb) >= thr) {
                    hit_counted = hit_counted || easy;
                    hit_dc = hit_dc || !easy;
                }
            }
            if (act) hkeep[jj] = (hit_dc && !hit_counted) ? 0 : 1;
        }
        wsync();
        r.ng = compact_wave(0, ng, [=](int i) { return g_level[g0 + gidx[i]] != 2; }, gsel, capN);
        r.nh = compact_wave(0, nh, [=](int j) { return hkeep[j] != 0; }, hsel, capN);
        wsync();
        for (int i = lane; i < r.ng; i += kWave) gsel[i] = gidx[gsel[i]];     // positions -> row offsets; every lane its own entries
        for (int j = lane; j < r.nh; j += kWave) hsel[j] = hidx[hsel[j]];
        r.g = gsel;
        r.h = hsel;
        return r;
    };

    // boxes and trajectory indices of the frame's rows, position by position (the arithmetic of Boxes::get, done once per row)
    auto stage = [&](const FrameRows& R, long long g0, long long h0) {
        wsync();
        for (int i = lane; i < R.ng; i += kWave) {
            const long long row = g0 + R.g[i];
            double b[4];
            G.get(row, b);
            sgb[4 * i] = b[0]; sgb[4 * i + 1] = b[1]; sgb[4 * i + 2] = b[2]; sgb[4 * i + 3] = b[3];
            sgt[i] = g_traj[row];
        }
        for (int j = lane; j < R.nh; j += kWave) {
            const long long row = h0 + R.h[j];
            double b[4];
            H.get(row, b);
            shb[4 * j] = b[0]; shb[4 * j + 1] = b[1]; shb[4 * j + 2] = b[2]; shb[4 * j + 3] = b[3];
            sht[j] = h_traj[row];
        }
        wsync();
    };
    auto staged = [](const double* boxes, int i, double o[4]) { o[0] = boxes[4 * i]; o[1] = boxes[4 * i + 1]; o[2] = boxes[4 * i + 2]; o[3] = boxes[4 * i + 3]; };

    long long n_gt = 0, n_hyp = 0;                                       // wave-uniform
    // ---- alignment pass ----
    for (long long f = f0; f < f1 && !err; ++f) {
        const long long g0 = frame_gt_offsets[f], g1 = frame_gt_offsets[f + 1];
        const long long h0 = hbase + fho[f], h1 = hbase + fho[f + 1];
        const FrameRows R = frame_rows(g0, g1, h0, h1);
        if (R.ng < 0) { err = kErrCapacity; break; }
        const int ng = R.ng, nh = R.nh;
        if (ng > nG || nh > nH) { err = kErrCapacity; break; }          // more boxes in a frame than trajectories: the caller's counts are wrong
        if (ng == 0 && nh == 0) continue;
        stage(R, g0, h0);
        n_gt += ng;
        n_hyp += nh;
        bool bad = false;
        for (int base = 0; base < ng; base += kWave) {                   // lane = ground-truth row: count its trajectory, row[i] in j order
            const int i = base + lane;
            const bool act = i < ng;
            double gb[4] = {0., 0., 0., 0.};
            if (act) {
                staged(sgb, i, gb);
                const int ot = sgt[i];
                if (ot < 0 || ot >= nG) bad = true;
                else cg[ot] = cg[ot] + 1;
            }
            double sum = 0.;
            for (int jj = 0; jj < nh; ++jj) {
                double hb[4];
                staged(shb, jj, hb);                                     // the same row in every lane
                sum = sum + iou_dd(gb, hb);
            }
            if (act) rowsum[i] = sum;
        }
        if (__ballot(bad) != 0ull) { err = kErrCapacity; break; }
        wsync();
        for (int cbase = 0; cbase < nh; cbase += kWave) {                // lane = hypothesis: col[j] in i order, then the cells
            const int jj = cbase + lane;
            const bool act = jj < nh;
            double hb[4] = {0., 0., 0., 0.};
            int ht = 0;
            if (act) {
                staged(shb, jj, hb);
                ht = sht[jj];
                if (ht < 0 || ht >= nH) bad = true;
                else ch[ht] = ch[ht] + 1;
            }
            if (__ballot(bad) != 0ull) break;
            double col = 0.;
            for (int ii = 0; ii < ng; ++ii) {
                double gb[4];
                staged(sgb, ii, gb);
                col = col + iou_dd(gb, hb);
            }
            for (int ii = 0; ii < ng; ++ii) {
                double gb[4];
                staged(sgb, ii, gb);
                const int ot = sgt[ii];                                  // checked in the sweep above
                const double S = iou_dd(gb, hb);
                if (act && S > 0.) {
                    const long long cell = (long long)ot * nH + ht;
                    Pm[cell] = Pm[cell] + S / ((rowsum[ii] + col) - S);
                }
            }
        }
        if (__ballot(bad) != 0ull) { err = kErrCapacity; break; }
        wsync();
    }
    if (err) { if (lane == 0) atomicMax(status, err); return; }
    wsync();
    for (long long cell = lane; cell < cells; cell += kWave) {            // P -> A in place; a cell nothing was added to stays 0
        const double pv = Pm[cell];
        if (pv > 0.) {                                                   // only such a cell can be matched: its histogram starts here
            const int o = (int)(cell / nH), t = (int)(cell % nH);
            Pm[cell] = pv / ((double)(cg[o] + ch[t]) - pv);
#pragma unroll
            for (int a = 0; a < kAlphas; ++a) hist[cell * kAlphas + a] = 0;
        }
    }
    wsync();

    // ---- matching pass: lane a < 19 keeps tp[a] and loc[a] ----
    const double my_alpha = alpha_of(lane < kAlphas ? lane : kAlphas - 1);
    long long my_tp = 0;
    double my_loc = 0.;
    for (long long f = f0; f < f1 && !err; ++f) {
        const long long g0 = frame_gt_offsets[f], g1 = frame_gt_offsets[f + 1];
        const long long h0 = hbase + fho[f], h1 = hbase + fho[f + 1];
        if (h0 == h1) continue;
        const FrameRows R = frame_rows(g0, g1, h0, h1);
        const int ng = R.ng, nh = R.nh;
        if (ng < 0) { err = kErrCapacity; break; }
        if (nh == 0) continue;
        stage(R, g0, h0);
        if (hyp_match)
            for (int j = lane; j < nh; j += kWave) hyp_match[(h0 + R.h[j]) * 2 + lv] = -1;
        if (ng == 0) { wsync(); continue; }
        const bool transposed = nh < ng;                   // linear_assignment transposes when there are fewer columns than rows
        const int n = transposed ? nh : ng, m = transposed ? ng : nh;
        const int ld = munkres_ld(m);
        const bool in_lds = (long)n * ld <= (long)caps.lds_cost;
        if (!in_lds && !cost_g) { err = kErrCapacity; break; }
        float* Cm = in_lds ? lds_cost : cost_g;
        bool some = false;
        for (int cbase = 0; cbase < nh; cbase += kWave) {                // lane = hypothesis, ground-truth rows one after the other
            const int jj = cbase + lane;
            const bool act = jj < nh;
            double hb[4] = {0., 0., 0., 0.};
            int ht = 0;
            if (act) {
                staged(shb, jj, hb);
                ht = sht[jj];
            }
            for (int ii = 0; ii < ng; ++ii) {
                double gb[4];
                staged(sgb, ii, gb);
                const int ot = sgt[ii];
                if (act) {
                    const float g = (float)(Pm[(long long)ot * nH + ht] * iou_dd(gb, hb));
                    const int r = transposed ? jj : ii, cc = transposed ? ii : jj;
                    Cm[r * ld + cc] = -g;
                    some = some || (g > 0.f);
                }
            }
        }
        wsync();
        if (__ballot(some) == 0ull) continue;                            // the matrix is all zero: no pair would be kept
        const int rc = in_lds ? munkres_wave(lds_cost, n, m, ld, L) : munkres_wave(cost_g, n, m, ld, L);
        if (rc) { err = rc; break; }
        for (int base = 0; base < ng; base += kWave) {                   // lane = ground-truth row
            const int i = base + lane;
            bool matched = false;
            double v = 0.;
            if (i < ng) {
                const int jj = transposed ? L.col_star[i] : L.row_star[i];
                if (jj >= 0 && jj < nh) {
                    const long long grow = g0 + R.g[i], hrow = h0 + R.h[jj];
                    double gb[4], hb[4];
                    staged(sgb, i, gb);
                    staged(shb, jj, hb);
                    v = iou_dd(gb, hb);
                    const long long cell = (long long)sgt[i] * nH + sht[jj];
                    if ((float)(Pm[cell] * v) > 0.f) {
                        matched = true;
                        int b = 0;
#pragma unroll
                        for (int a = 0; a < kAlphas; ++a) b += (v >= alpha_of(a)) ? 1 : 0;
                        if (b > 0) hist[cell * kAlphas + (b - 1)] = (uint16_t)(hist[cell * kAlphas + (b - 1)] + 1);
                        if (hyp_match) hyp_match[hrow * 2 + lv] = grow;
                    }
                }
            }
            for (unsigned long long todo = __ballot(matched); todo; todo &= todo - 1ull) {      // one match after the other, in row order
                const double vb = bcast_d(v, __builtin_ctzll(todo));
                if (lane < kAlphas && vb >= my_alpha) { my_tp += 1; my_loc = my_loc + vb; }
            }
        }
        wsync();
    }
    if (err) { if (lane == 0) atomicMax(status, err); return; }
    wsync();

    // ---- association sums: per lane over its cells, then the 64 partial sums in lane order ----
    double a_ass[kAlphas], a_re[kAlphas], a_pr[kAlphas];
#pragma unroll
    for (int a = 0; a < kAlphas; ++a) { a_ass[a] = 0.; a_re[a] = 0.; a_pr[a] = 0.; }
    for (long long cell = lane; cell < cells; cell += kWave) {
        if (!(Pm[cell] > 0.)) continue;                                  // nothing aligned, nothing matched
        const int o = (int)(cell / nH), t = (int)(cell % nH);
        const double dg = (double)cg[o], dh = (double)ch[t], dgh = (double)(cg[o] + ch[t]);
        int cnt = 0;
#pragma unroll
        for (int a = kAlphas - 1; a >= 0; --a) {
            cnt += hist[cell * kAlphas + a];
            if (cnt > 0) {
                const double dc = (double)cnt;
                a_ass[a] = a_ass[a] + dc * (dc / (dgh - dc));
                a_re[a] = a_re[a] + dc * (dc / dg);
                a_pr[a] = a_pr[a] + dc * (dc / dh);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < kAlphas; ++a) {
        part[(a * 3 + 0) * kWave + lane] = a_ass[a];
        part[(a * 3 + 1) * kWave + lane] = a_re[a];
        part[(a * 3 + 2) * kWave + lane] = a_pr[a];
    }
    wsync();
    if (lane < kAlphas) {                                                // lane = threshold
        double* o = hota_sums + (wv * kAlphas + lane) * 4;
        for (int q = 0; q < 3; ++q) {
            double tot = 0.;
            for (int l = 0; l < kWave; ++l) tot = tot + part[(lane * 3 + q) * kWave + l];
            o[q] = tot;
        }
        o[3] = my_loc;
        hota_counts[wv * 21 + 2 + lane] = my_tp;
    }
    if (lane == 0) {
        hota_counts[wv * 21] = n_gt;
        hota_counts[wv * 21 + 1] = n_hyp;
    }
}

__global__ void hota_fill_kernel(long long n, int64_t* __restrict__ hyp_match) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hyp_match[i] = -2;
}

// wt_mot_hota_dev on an input whose pointers are device pointers
int launch(const wt::TrackInput& in, int64_t n_hyp, const int32_t* g_ntraj, const int32_t* h_ntraj, const int64_t* mat_offsets,
           int64_t matrix_cells, const double* thr, int64_t max_frame_boxes, int64_t max_gt_traj, int64_t max_hyp_traj,
           int64_t* hota_counts, double* hota_sums, int64_t* hyp_match, int32_t* status_dev, void* workspace, size_t workspace_bytes,
           hipStream_t stream) {
    WT_TRY(wt::ensure_device());
    if (in.k_sets < 1 || in.n_streams < 0 || in.n_frames < 0 || in.n_gt < 0 || n_hyp < 0 || matrix_cells < 0 || !thr || !hota_counts || !hota_sums ||
        !status_dev || !g_ntraj || !h_ntraj || !mat_offsets) {
        wt::set_error("wt_mot_hota: bad argument");
        return WT_ERR_INVALID;
    }
    if (in.n_classes < 1 || in.n_classes > kMaxClasses) { wt::set_error("wt_mot_hota: n_classes must be 1..%d", kMaxClasses); return WT_ERR_INVALID; }
    Caps caps;
    WT_TRY(pick_caps(max_frame_boxes, max_gt_traj, max_hyp_traj, &caps));
    const size_t n_waves = 2 * (size_t)in.k_sets * (size_t)in.n_streams * (size_t)in.n_classes;
    if (n_waves > 0x7fffffffull) { wt::set_error("wt_mot_hota: %zu wavefronts in one call", n_waves); return WT_ERR_CAPACITY; }
    Workspace ws = carve(wt::align_ptr(workspace), n_waves, caps, (size_t)matrix_cells);
    if (n_waves && (!workspace || workspace_bytes < ws.bytes + 256)) {
        wt::set_error("HOTA evaluation workspace too small: need %zu bytes, have %zu", ws.bytes + 256, workspace_bytes);
        return WT_ERR_INVALID;
    }
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    if (n_hyp > 0 && hyp_match)
        hipLaunchKernelGGL(hota_fill_kernel, dim3((unsigned)((2 * n_hyp + 255) / 256)), dim3(256), 0, stream, (long long)(2 * n_hyp), hyp_match);
    if (n_waves == 0) { WT_HIP(hipGetLastError()); return WT_OK; }
    WT_HIP(hipMemsetAsync(hota_counts, 0, n_waves * 21 * sizeof(int64_t), stream));
    WT_HIP(hipMemsetAsync(hota_sums, 0, n_waves * kAlphas * 4 * sizeof(double), stream));
    if (caps.lds_bytes > 48 * 1024)
        WT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mot_hota_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)caps.lds_bytes));
    const Boxes G = {in.gx, in.gy, in.gw, in.gh}, H = {in.hx, in.hy, in.hw, in.hh};
    hipLaunchKernelGGL(mot_hota_kernel, dim3((unsigned)n_waves), dim3(kWave), caps.lds_bytes, stream, G, in.g_category, in.g_level, in.g_id,
                       in.frame_gt_offsets, in.stream_frame_offsets, (long long)in.n_frames, (int)in.n_streams, (int)in.n_classes,
                       in.set_row_offsets, in.frame_hyp_offsets, H, in.h_category, in.h_id, g_ntraj, h_ntraj, mat_offsets, (long long)matrix_cells,
                       make_thresholds(thr, in.n_classes), caps, ws, hota_counts, hota_sums, hyp_match, (int*)status_dev);
    WT_HIP(hipGetLastError());
    return WT_OK;
}

}  // namespace

extern "C" {

void wt_mot_hota_limits(int32_t* max_frame_boxes, int32_t* max_trajectories, int32_t* max_stream_frames, int64_t* lds_cost_floats,
                        int64_t* lds_zmask_bytes) {
    if (max_frame_boxes) *max_frame_boxes = kMaxBoxes;
    if (max_trajectories) *max_trajectories = kMaxTraj;
    if (max_stream_frames) *max_stream_frames = kMaxStreamFrames;
    if (lds_cost_floats) *lds_cost_floats = kLdsCostFloats;
    if (lds_zmask_bytes) *lds_zmask_bytes = (int64_t)kLdsZmaskMax;
}

size_t wt_mot_hota_workspace(int32_t k_sets, int32_t n_streams, int32_t n_classes, int64_t max_frame_boxes, int64_t max_gt_traj,
                             int64_t max_hyp_traj, int64_t matrix_cells) {
    Caps c;
    if (k_sets < 1 || n_streams < 0 || n_classes < 1 || matrix_cells < 0 || pick_caps(max_frame_boxes, max_gt_traj, max_hyp_traj, &c) != WT_OK) return 0;
    return carve(nullptr, 2 * (size_t)k_sets * (size_t)n_streams * (size_t)n_classes, c, (size_t)matrix_cells).bytes + 256;
}

int wt_mot_hota_dev(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                    const int32_t* g_category, const int32_t* g_level, const int32_t* g_traj,
                    int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                    int32_t k_sets, int64_t n_hyp, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                    const double* hx, const double* hy, const double* hw, const double* hh,
                    const int32_t* h_category, const int32_t* h_traj,
                    const int32_t* g_ntraj, const int32_t* h_ntraj, const int64_t* mat_offsets, int64_t matrix_cells,
                    int32_t n_classes, const double* thr, int64_t max_frame_boxes, int64_t max_gt_traj, int64_t max_hyp_traj,
                    int64_t* hota_counts, double* hota_sums, int64_t* hyp_match, int32_t* status_dev,
                    void* workspace, size_t workspace_bytes, void* stream_) {
    const wt::TrackInput in = {n_gt, gx, gy, gw, gh, g_category, g_level, g_traj, n_frames, frame_gt_offsets, n_streams, stream_frame_offsets,
                               k_sets, set_row_offsets, frame_hyp_offsets, hx, hy, hw, hh, h_category, h_traj, n_classes};
    return launch(in, n_hyp, g_ntraj, h_ntraj, mat_offsets, matrix_cells, thr, max_frame_boxes, max_gt_traj, max_hyp_traj, hota_counts, hota_sums,
                  hyp_match, status_dev, workspace, workspace_bytes, (hipStream_t)stream_);
}

int wt_mot_hota_host(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                     const int32_t* g_category, const int32_t* g_level, const int32_t* g_traj,
                     int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                     int32_t k_sets, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                     const double* hx, const double* hy, const double* hw, const double* hh,
                     const int32_t* h_category, const int32_t* h_traj,
                     const int32_t* g_ntraj, const int32_t* h_ntraj,
                     int32_t n_classes, const double* thr, size_t workspace_limit_bytes,
                     int64_t* hota_counts, double* hota_sums, int64_t* hyp_match) {
    const wt::TrackInput in = {n_gt, gx, gy, gw, gh, g_category, g_level, g_traj, n_frames, frame_gt_offsets, n_streams, stream_frame_offsets,
                               k_sets, set_row_offsets, frame_hyp_offsets, hx, hy, hw, hh, h_category, h_traj, n_classes};
    WT_TRY(wt::check_track_layout(in, "wt_mot_hota_host", thr && hota_counts && hota_sums && g_ntraj && h_ntraj, kMaxClasses));
    const size_t n_problems = (size_t)k_sets * (size_t)n_streams * (size_t)n_classes;
    int64_t max_g = 0, max_h = 0, max_boxes = 0;
    for (size_t i = 0; i < (size_t)n_streams * (size_t)n_classes; ++i) {
        if (g_ntraj[i] < 0) { wt::set_error("g_ntraj[%zu] is negative", i); return WT_ERR_INVALID; }
        max_g = std::max<int64_t>(max_g, g_ntraj[i]);
    }
    for (size_t i = 0; i < n_problems; ++i) {
        if (h_ntraj[i] < 0) { wt::set_error("h_ntraj[%zu] is negative", i); return WT_ERR_INVALID; }
        max_h = std::max<int64_t>(max_h, h_ntraj[i]);
    }
    for (int32_t s = 0; s < n_streams; ++s)
        if (stream_frame_offsets[s + 1] - stream_frame_offsets[s] > kMaxStreamFrames) {
            wt::set_error("%lld frames in one stream: the HOTA kernel takes at most %d", (long long)(stream_frame_offsets[s + 1] - stream_frame_offsets[s]),
                          kMaxStreamFrames);
            return WT_ERR_CAPACITY;
        }
    // a trajectory index inside its problem's count, and at most once per frame and class; on the way, the most boxes of one class in one frame
    std::vector<int64_t> per_class((size_t)n_classes);
    auto ids_unique = [&](const int32_t* cat, const int32_t* traj, const int32_t* counts, int64_t r0, int64_t r1) {
        std::fill(per_class.begin(), per_class.end(), 0);
        return wt::frame_ids_unique(cat, traj, r0, r1, n_classes, [&](int64_t r) {
            max_boxes = std::max(max_boxes, ++per_class[(size_t)cat[r] - 1]);
            return traj[r] >= 0 && traj[r] < counts[cat[r] - 1];
        });
    };
    WT_TRY(wt::walk_track_frames(in,
        [&](int32_t s, int64_t f, int64_t r0, int64_t r1) {
            if (ids_unique(g_category, g_traj, g_ntraj + (size_t)s * n_classes, r0, r1)) return WT_OK;
            wt::set_error("ground truth: a trajectory index is out of range or occurs twice in frame %lld", (long long)f);
            return WT_ERR_INVALID;
        },
        [&](int32_t k, int32_t s, int64_t f, int64_t r0, int64_t r1) {
            if (ids_unique(h_category, h_traj, h_ntraj + ((size_t)k * n_streams + s) * n_classes, r0, r1)) return WT_OK;
            wt::set_error("result set %d: a trajectory index is out of range or occurs twice in frame %lld", (int)k, (long long)f);
            return WT_ERR_INVALID;
        }));
    if (max_boxes > kMaxBoxes) {
        wt::set_error("%lld boxes of one class in one frame: the assignment kernel takes at most %d a side", (long long)max_boxes, kMaxBoxes);
        return WT_ERR_CAPACITY;
    }
    if (max_g > kMaxTraj || max_h > kMaxTraj) {
        wt::set_error("%lld trajectories of one class in one stream: the HOTA kernel takes at most %d a side", (long long)std::max(max_g, max_h), kMaxTraj);
        return WT_ERR_CAPACITY;
    }
    // per-problem matrix offsets: two matrices (LEVEL_1, LEVEL_2) of g x h cells each
    std::vector<int64_t> mat_offsets(n_problems + 1, 0);
    for (size_t p = 0; p < n_problems; ++p) {
        const int64_t a = g_ntraj[(p / n_classes % n_streams) * n_classes + p % n_classes], b = h_ntraj[p];
        mat_offsets[p + 1] = mat_offsets[p] + 2 * a * b;
    }
    const int64_t matrix_cells = mat_offsets[n_problems];
    const size_t wsb = wt_mot_hota_workspace(k_sets, n_streams, n_classes, max_boxes, max_g, max_h, matrix_cells);
    if (!wsb) return WT_ERR_CAPACITY;
    if (workspace_limit_bytes && wsb > workspace_limit_bytes) {
        wt::set_error("HOTA evaluation workspace too small: need %zu bytes, the limit is %zu (score fewer results per call)", wsb, workspace_limit_bytes);
        return WT_ERR_INVALID;
    }
    WT_TRY(wt::ensure_device());
    wt::StagedTrackInput staged;
    WT_TRY(staged.upload(in));
    const size_t nh = (size_t)staged.n_hyp;
    wt::DevBuf dgn, dhn, dmo, dcnt, dsum, dmatch, dws;
    WT_TRY(dgn.upload(g_ntraj, 4 * (size_t)n_streams * n_classes)); WT_TRY(dhn.upload(h_ntraj, 4 * n_problems));
    WT_TRY(dmo.upload(mat_offsets.data(), 8 * (n_problems + 1)));
    WT_TRY(dcnt.alloc(8 * n_problems * 2 * 21)); WT_TRY(dsum.alloc(8 * n_problems * 2 * kAlphas * 4));
    if (hyp_match) WT_TRY(dmatch.alloc(16 * nh));
    WT_TRY(dws.alloc(wsb));
    WT_TRY(launch(staged.dev, staged.n_hyp, dgn.as<int32_t>(), dhn.as<int32_t>(), dmo.as<int64_t>(), matrix_cells, thr, max_boxes, max_g, max_h,
                  dcnt.as<int64_t>(), dsum.as<double>(), hyp_match ? dmatch.as<int64_t>() : nullptr, staged.status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(staged.finish("HOTA evaluation"));
    if (n_problems) {
        WT_HIP(hipMemcpy(hota_counts, dcnt.p, 8 * n_problems * 2 * 21, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(hota_sums, dsum.p, 8 * n_problems * 2 * kAlphas * 4, hipMemcpyDeviceToHost));
    }
    if (nh && hyp_match) WT_HIP(hipMemcpy(hyp_match, dmatch.p, 16 * nh, hipMemcpyDeviceToHost));
    return WT_OK;
}

}  // extern "C"
