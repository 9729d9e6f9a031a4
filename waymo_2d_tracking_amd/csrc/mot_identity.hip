// Identity preservation (IDF1 / IDP / IDR, Ristani et al. 2016) of tracking results on gfx950 (include/waymotrack.h,
// "MOT identity evaluation"; DESIGN.md section 18 has the definition).
//
// Same shape as mot_eval.hip: one 64-lane wavefront owns one independent problem = (result set k, stream s, class c).
//   count pass   walk the stream's frames in order, compact the class's rows (ballot + popcount), lane = hypothesis box,
//                ground-truth rows one after the other; where IoU >= thr, decrement the float32 cell (trajectory of the
//                object, trajectory of the hypothesis) of the problem's matrix, one matrix per difficulty level.  A pair
//                occurs at most once per frame and one wave walks the frames in order: plain load / add / store by one
//                lane, no atomics.  The matrices live in the workspace with the smaller side as rows.
//   assignment   munkres_wave of sort_device.h in place on each level's matrix (-n: small integers, exact in float32).
//   re-walk      the solve destroys the matrix, so the frames are walked once more: a pair with IoU >= thr whose
//                trajectories are assigned to each other is an identity true positive.
// Compile with -ffp-contract=off (IoU in the operation order of tracking/sort/sort.py:34-47; eval_device.h has it).
#include "eval_device.h"
#include "eval_host.h"

using namespace wtdev;

namespace {

constexpr int kMaxTraj = 4096;                // trajectories per side of one problem: the limit of munkres_wave
constexpr size_t kLdsStarsMax = 8 * 1024;     // star / prime arrays stay in LDS up to here (2 n + m <= 2048), in the workspace beyond
constexpr size_t kLdsZmaskMax = 32 * 1024;    // zero bitmaps stay in LDS up to here (about 500 x 500), in the workspace beyond

struct Caps {
    int capG, capH;          // trajectories (= boxes of one frame at most) per side of one problem
    int capS, capB;          // the smaller / larger side of any problem is at most this
    bool stars_g, zmask_g;
    size_t lds_bytes;
};

struct Workspace {                       // device pointers carved from one block; everything but `mats` is [problem][cap]
    int *gidx, *hidx;                    // [capG], [capH] rows of this class in the frame, relative to the frame's first row
    int* assign;                         // [2][capG] hypothesis trajectory assigned to the object's trajectory, per level (-1 none)
    int* stars_g;                        // [2 capS + capB] when the star arrays can outgrow their LDS share
    unsigned long long* zmask_g;         // [capS * ceil(capB / 64)] when the bitmaps can
    float* mats;                         // every problem's two matrices, at mat_offsets[p]
    size_t bytes;
};

int pick_caps(int64_t max_gt_traj, int64_t max_hyp_traj, Caps* c) {
    if (max_gt_traj > kMaxTraj || max_hyp_traj > kMaxTraj) {
        wt::set_error("%lld trajectories of one class in one stream: the assignment kernel takes at most %d a side",
                      (long long)std::max(max_gt_traj, max_hyp_traj), kMaxTraj);
        return WT_ERR_CAPACITY;
    }
    if (max_gt_traj < 0 || max_hyp_traj < 0) { wt::set_error("wt_mot_identity: a trajectory count is negative"); return WT_ERR_INVALID; }
    c->capG = (int)(max_gt_traj > 0 ? max_gt_traj : 1);
    c->capH = (int)(max_hyp_traj > 0 ? max_hyp_traj : 1);
    c->capS = std::min(c->capG, c->capH);
    c->capB = std::max(c->capG, c->capH);
    const size_t stars = wt::align_up((size_t)(2 * c->capS + c->capB) * sizeof(int), 16);
    const size_t zmask = (size_t)c->capS * ((size_t)(c->capB + 63) / 64) * 8;
    c->stars_g = stars > kLdsStarsMax;
    c->zmask_g = zmask > kLdsZmaskMax;
    c->lds_bytes = (c->stars_g ? 0 : stars) + (c->zmask_g ? 0 : zmask) + 16;
    return WT_OK;
}

Workspace carve(void* base, size_t n_problems, const Caps& c, size_t matrix_floats) {
    wt::Carver cv(base);
    Workspace w;
    w.gidx = cv.take<int>(n_problems * c.capG);
    w.hidx = cv.take<int>(n_problems * c.capH);
    w.assign = cv.take<int>(n_problems * 2 * c.capG);
    w.stars_g = cv.take<int>(c.stars_g ? n_problems * (size_t)(2 * c.capS + c.capB) : 1);
    w.zmask_g = cv.take<unsigned long long>(c.zmask_g ? n_problems * (size_t)c.capS * ((size_t)(c.capB + 63) / 64) : 1);
    w.mats = cv.take<float>(matrix_floats ? matrix_floats : 1);
    w.bytes = cv.off;
    return w;
}

__global__ __launch_bounds__(kWave) void mot_identity_kernel(
    Boxes G, const int32_t* __restrict__ g_cat, const int32_t* __restrict__ g_level, const int32_t* __restrict__ g_traj,
    const int64_t* __restrict__ frame_gt_offsets, const int64_t* __restrict__ stream_frame_offsets, long long n_frames,
    int n_streams, int C, const int64_t* __restrict__ set_row_offsets, const int64_t* __restrict__ frame_hyp_offsets,
    Boxes H, const int32_t* __restrict__ h_cat, const int32_t* __restrict__ h_traj,
    const int32_t* __restrict__ g_ntraj, const int32_t* __restrict__ h_ntraj, const int64_t* __restrict__ mat_offsets,
    long long matrix_floats, Thresholds thr_all, Caps caps, Workspace ws,
    int64_t* __restrict__ id_counts, int64_t* __restrict__ hyp_idmatch, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const size_t p = blockIdx.x;
    int k, s, c;
    decode_problem(p, n_streams, C, &k, &s, &c);
    const double thr = thr_all.v[c - 1];
    const int nG = g_ntraj[(size_t)s * C + (c - 1)], nH = h_ntraj[p];
    const bool transposed = nH < nG;                       // the smaller side is the rows
    const int n = transposed ? nH : nG, m = transposed ? nG : nH;
    const int ld = munkres_ld(m);
    const long long mo0 = mat_offsets[p], mo1 = mat_offsets[p + 1];
    const long long cells = (long long)n * ld;
    int err = 0;
    if (nG < 0 || nH < 0 || nG > caps.capG || nH > caps.capH || mo0 < 0 || mo1 > matrix_floats || mo1 - mo0 < 2 * cells) err = kErrCapacity;
    if (err) { if (lane == 0) atomicMax(status, err); return; }

    const size_t Wcap = (size_t)(caps.capB + 63) / 64;
    const size_t stars_bytes = (((size_t)(2 * caps.capS + caps.capB) * sizeof(int) + 15) / 16) * 16;
    MunkresMem L;
    L.row_star = caps.stars_g ? ws.stars_g + p * (size_t)(2 * caps.capS + caps.capB) : reinterpret_cast<int*>(smem);
    L.row_prime = L.row_star + caps.capS;
    L.col_star = L.row_star + 2 * caps.capS;
    L.zmask = caps.zmask_g ? ws.zmask_g + p * (size_t)caps.capS * Wcap
                           : reinterpret_cast<unsigned long long*>(smem + (caps.stars_g ? 0 : stars_bytes));
    L.help = nullptr;
    L.cost_in_lds = 0;

    int* gidx = ws.gidx + p * caps.capG;
    int* hidx = ws.hidx + p * caps.capH;
    int* assign = ws.assign + p * 2 * (size_t)caps.capG;
    float* M1 = ws.mats + mo0;                                     // LEVEL_1, then LEVEL_2
    float* M2 = M1 + cells;
    for (long long i = lane; i < 2 * cells; i += kWave) M1[i] = 0.f;
    for (int i = lane; i < 2 * nG; i += kWave) assign[(i / nG) * caps.capG + (i % nG)] = -1;
    wsync();

    const long long f0 = stream_frame_offsets[s], f1 = stream_frame_offsets[s + 1];
    const long long hbase = set_row_offsets[k];
    const int64_t* fho = frame_hyp_offsets + (size_t)k * (size_t)(n_frames + 1);
    long long n_gt[2] = {0, 0}, n_hyp[2] = {0, 0}, n_tp[2] = {0, 0};       // wave-uniform
    bool any1 = false, any2 = false;

    // ---- count pass ----
    for (long long f = f0; f < f1 && !err; ++f) {
        const long long g0 = frame_gt_offsets[f], g1 = frame_gt_offsets[f + 1];
        const long long h0 = hbase + fho[f], h1 = hbase + fho[f + 1];
        const int ng = compact_rows(g_cat, g0, g1, c, gidx, caps.capG);
        const int nh = compact_rows(h_cat, h0, h1, c, hidx, caps.capH);
        if (ng > nG || nh > nH) { err = kErrCapacity; break; }          // more boxes in a frame than trajectories: the caller's counts are wrong
        if (ng == 0 && nh == 0) continue;
        wsync();
        bool bad = false;
        for (int base = 0; base < ng; base += kWave) {
            const int i = base + lane;
            const bool act = i < ng;
            bool easy = false;
            if (act) {
                const long long grow = g0 + gidx[i];
                easy = g_level[grow] != 2;
                const int ot = g_traj[grow];
                bad = bad || ot < 0 || ot >= nG;
            }
            n_gt[1] += __popcll(__ballot(act));
            n_gt[0] += __popcll(__ballot(easy));
        }
        if (__ballot(bad) != 0ull) { err = kErrCapacity; break; }
        for (int cbase = 0; cbase < nh; cbase += kWave) {                // lane = hypothesis, ground-truth rows one after the other
            const int jj = cbase + lane;
            const bool act = jj < nh;
            double hb[4] = {0., 0., 0., 0.};
            int ht = 0;
            if (act) {
                const long long hrow = h0 + hidx[jj];
                H.get(hrow, hb);
                ht = h_traj[hrow];
                bad = ht < 0 || ht >= nH;
            }
            bool hit_counted = false, hit_dc = false;
            for (int ii = 0; ii < ng; ++ii) {
                const long long grow = g0 + uni(gidx[ii]);               // the same row in every lane: scalar loads
                double gb[4];
                G.get(grow, gb);
                const bool easy = g_level[grow] != 2;
                const int ot = g_traj[grow];
                if (act && !bad && iou_dd(gb, hb) >= thr) {
                    hit_counted = hit_counted || easy;
                    hit_dc = hit_dc || !easy;
                    const long long cell = transposed ? (long long)ht * ld + ot : (long long)ot * ld + ht;
                    M2[cell] = M2[cell] - 1.f;
                    any2 = true;
                    if (easy) { M1[cell] = M1[cell] - 1.f; any1 = true; }
                }
            }
            n_hyp[1] += __popcll(__ballot(act));
            n_hyp[0] += __popcll(__ballot(act && !(hit_dc && !hit_counted)));
            if (__ballot(bad) != 0ull) { err = kErrCapacity; break; }
        }
        wsync();
    }
    // ---- assignment, level by level ----
    const unsigned long long anyb[2] = {__ballot(any1), __ballot(any2)};
#pragma unroll 1
    for (int lv = 0; lv < 2 && !err; ++lv) {
        if (anyb[lv] == 0ull || n == 0) continue;                        // no pair reaches the threshold: idtp is 0
        const int rc = munkres_wave(lv ? M2 : M1, n, m, ld, L);
        if (rc) { err = rc; break; }
        int* a = assign + lv * caps.capG;
        for (int r = lane; r < n; r += kWave) {
            const int col = L.row_star[r];
            if (col >= 0 && col < m) {
                if (transposed) a[col] = r; else a[r] = col;
            }
        }
        wsync();
    }
    if (err) { if (lane == 0) atomicMax(status, err); return; }
    // ---- re-walk: pairs whose trajectories are assigned to each other ----
    for (long long f = f0; f < f1; ++f) {
        const long long g0 = frame_gt_offsets[f], g1 = frame_gt_offsets[f + 1];
        const long long h0 = hbase + fho[f], h1 = hbase + fho[f + 1];
        if (h0 == h1) continue;
        const int ng = compact_rows(g_cat, g0, g1, c, gidx, caps.capG);
        const int nh = compact_rows(h_cat, h0, h1, c, hidx, caps.capH);
        if (nh == 0) continue;
        wsync();
        for (int cbase = 0; cbase < nh; cbase += kWave) {
            const int jj = cbase + lane;
            const bool act = jj < nh;
            double hb[4] = {0., 0., 0., 0.};
            int ht = -2;
            long long hrow = 0;
            if (act) {
                hrow = h0 + hidx[jj];
                H.get(hrow, hb);
                ht = h_traj[hrow];
            }
            bool hit_counted = false, hit_dc = false;
            long long m1 = -1, m2 = -1;
            for (int ii = 0; ii < ng; ++ii) {
                const long long grow = g0 + uni(gidx[ii]);
                double gb[4];
                G.get(grow, gb);
                const bool easy = g_level[grow] != 2;
                const int ot = g_traj[grow];
                const int a1 = assign[ot], a2 = assign[caps.capG + ot];
                if (act && iou_dd(gb, hb) >= thr) {
                    hit_counted = hit_counted || easy;
                    hit_dc = hit_dc || !easy;
                    if (a2 == ht) m2 = grow;
                    if (easy && a1 == ht) m1 = grow;
                }
            }
            n_tp[1] += __popcll(__ballot(m2 >= 0));
            n_tp[0] += __popcll(__ballot(m1 >= 0));
            if (act && hyp_idmatch) {
                if (m1 < 0 && hit_dc && !hit_counted) m1 = -2;           // left out of LEVEL_1
                hyp_idmatch[hrow * 2] = m1;
                hyp_idmatch[hrow * 2 + 1] = m2;
            }
        }
        wsync();
    }
    if (lane < 2) {                                  // lane = level
        int64_t* o = id_counts + (p * 2 + lane) * 3;
        o[0] = lane ? n_tp[1] : n_tp[0];
        o[1] = lane ? n_gt[1] : n_gt[0];
        o[2] = lane ? n_hyp[1] : n_hyp[0];
    }
}

__global__ void identity_fill_kernel(long long n, int64_t* __restrict__ hyp_idmatch) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hyp_idmatch[i] = -2;
}

// wt_mot_identity_dev on an input whose pointers are device pointers
int launch(const wt::TrackInput& in, int64_t n_hyp, const int32_t* g_ntraj, const int32_t* h_ntraj, const int64_t* mat_offsets,
           int64_t matrix_floats, const double* thr, int64_t max_gt_traj, int64_t max_hyp_traj, int64_t* id_counts, int64_t* hyp_idmatch,
           int32_t* status_dev, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    WT_TRY(wt::ensure_device());
    if (in.k_sets < 1 || in.n_streams < 0 || in.n_frames < 0 || in.n_gt < 0 || n_hyp < 0 || matrix_floats < 0 || !thr || !id_counts || !status_dev ||
        !g_ntraj || !h_ntraj || !mat_offsets) {
        wt::set_error("wt_mot_identity: bad argument");
        return WT_ERR_INVALID;
    }
    if (in.n_classes < 1 || in.n_classes > kMaxClasses) { wt::set_error("wt_mot_identity: n_classes must be 1..%d", kMaxClasses); return WT_ERR_INVALID; }
    Caps caps;
    WT_TRY(pick_caps(max_gt_traj, max_hyp_traj, &caps));
    const size_t n_problems = (size_t)in.k_sets * (size_t)in.n_streams * (size_t)in.n_classes;
    if (n_problems > 0x7fffffffull) { wt::set_error("wt_mot_identity: %zu problems in one call", n_problems); return WT_ERR_CAPACITY; }
    Workspace ws = carve(wt::align_ptr(workspace), n_problems, caps, (size_t)matrix_floats);
    if (n_problems && (!workspace || workspace_bytes < ws.bytes + 256)) {
        wt::set_error("identity evaluation workspace too small: need %zu bytes, have %zu", ws.bytes + 256, workspace_bytes);
        return WT_ERR_INVALID;
    }
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    if (n_hyp > 0 && hyp_idmatch)
        hipLaunchKernelGGL(identity_fill_kernel, dim3((unsigned)((2 * n_hyp + 255) / 256)), dim3(256), 0, stream, (long long)(2 * n_hyp), hyp_idmatch);
    if (n_problems == 0) { WT_HIP(hipGetLastError()); return WT_OK; }
    WT_HIP(hipMemsetAsync(id_counts, 0, n_problems * 6 * sizeof(int64_t), stream));
    if (caps.lds_bytes > 48 * 1024)
        WT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mot_identity_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)caps.lds_bytes));
    const Boxes G = {in.gx, in.gy, in.gw, in.gh}, H = {in.hx, in.hy, in.hw, in.hh};
    hipLaunchKernelGGL(mot_identity_kernel, dim3((unsigned)n_problems), dim3(kWave), caps.lds_bytes, stream, G, in.g_category, in.g_level, in.g_id,
                       in.frame_gt_offsets, in.stream_frame_offsets, (long long)in.n_frames, (int)in.n_streams, (int)in.n_classes,
                       in.set_row_offsets, in.frame_hyp_offsets, H, in.h_category, in.h_id, g_ntraj, h_ntraj, mat_offsets, (long long)matrix_floats,
                       make_thresholds(thr, in.n_classes), caps, ws, id_counts, hyp_idmatch, (int*)status_dev);
    WT_HIP(hipGetLastError());
    return WT_OK;
}

}  // namespace

extern "C" {

void wt_mot_identity_limits(int32_t* max_trajectories, int64_t* lds_stars_bytes, int64_t* lds_zmask_bytes) {
    if (max_trajectories) *max_trajectories = kMaxTraj;
    if (lds_stars_bytes) *lds_stars_bytes = (int64_t)kLdsStarsMax;
    if (lds_zmask_bytes) *lds_zmask_bytes = (int64_t)kLdsZmaskMax;
}

size_t wt_mot_identity_workspace(int32_t k_sets, int32_t n_streams, int32_t n_classes, int64_t max_gt_traj, int64_t max_hyp_traj,
                                 int64_t matrix_floats) {
    Caps c;
    if (k_sets < 1 || n_streams < 0 || n_classes < 1 || matrix_floats < 0 || pick_caps(max_gt_traj, max_hyp_traj, &c) != WT_OK) return 0;
    return carve(nullptr, (size_t)k_sets * (size_t)n_streams * (size_t)n_classes, c, (size_t)matrix_floats).bytes + 256;
}

int wt_mot_identity_dev(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                        const int32_t* g_category, const int32_t* g_level, const int32_t* g_traj,
                        int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                        int32_t k_sets, int64_t n_hyp, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                        const double* hx, const double* hy, const double* hw, const double* hh,
                        const int32_t* h_category, const int32_t* h_traj,
                        const int32_t* g_ntraj, const int32_t* h_ntraj, const int64_t* mat_offsets, int64_t matrix_floats,
                        int32_t n_classes, const double* thr, int64_t max_gt_traj, int64_t max_hyp_traj,
                        int64_t* id_counts, int64_t* hyp_idmatch, int32_t* status_dev,
                        void* workspace, size_t workspace_bytes, void* stream_) {
    const wt::TrackInput in = {n_gt, gx, gy, gw, gh, g_category, g_level, g_traj, n_frames, frame_gt_offsets, n_streams, stream_frame_offsets,
                               k_sets, set_row_offsets, frame_hyp_offsets, hx, hy, hw, hh, h_category, h_traj, n_classes};
    return launch(in, n_hyp, g_ntraj, h_ntraj, mat_offsets, matrix_floats, thr, max_gt_traj, max_hyp_traj, id_counts, hyp_idmatch, status_dev,
                  workspace, workspace_bytes, (hipStream_t)stream_);
}

int wt_mot_identity_host(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                         const int32_t* g_category, const int32_t* g_level, const int32_t* g_traj,
                         int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t k_sets, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                         const double* hx, const double* hy, const double* hw, const double* hh,
                         const int32_t* h_category, const int32_t* h_traj,
                         const int32_t* g_ntraj, const int32_t* h_ntraj,
                         int32_t n_classes, const double* thr, size_t workspace_limit_bytes,
                         int64_t* id_counts, int64_t* hyp_idmatch) {
    const wt::TrackInput in = {n_gt, gx, gy, gw, gh, g_category, g_level, g_traj, n_frames, frame_gt_offsets, n_streams, stream_frame_offsets,
                               k_sets, set_row_offsets, frame_hyp_offsets, hx, hy, hw, hh, h_category, h_traj, n_classes};
    WT_TRY(wt::check_track_layout(in, "wt_mot_identity_host", thr && id_counts && g_ntraj && h_ntraj, kMaxClasses));
    const size_t n_problems = (size_t)k_sets * (size_t)n_streams * (size_t)n_classes;
    int64_t max_g = 0, max_h = 0;
    for (size_t i = 0; i < (size_t)n_streams * (size_t)n_classes; ++i) {
        if (g_ntraj[i] < 0) { wt::set_error("g_ntraj[%zu] is negative", i); return WT_ERR_INVALID; }
        max_g = std::max<int64_t>(max_g, g_ntraj[i]);
    }
    for (size_t i = 0; i < n_problems; ++i) {
        if (h_ntraj[i] < 0) { wt::set_error("h_ntraj[%zu] is negative", i); return WT_ERR_INVALID; }
        max_h = std::max<int64_t>(max_h, h_ntraj[i]);
    }
    // a trajectory index inside its problem's count, and at most once per frame and class
    auto ids_unique = [&](const int32_t* cat, const int32_t* traj, const int32_t* counts, int64_t r0, int64_t r1) {
        return wt::frame_ids_unique(cat, traj, r0, r1, n_classes, [&](int64_t r) { return traj[r] >= 0 && traj[r] < counts[cat[r] - 1]; });
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
    if (max_g > kMaxTraj || max_h > kMaxTraj) {
        wt::set_error("%lld trajectories of one class in one stream: the assignment kernel takes at most %d a side", (long long)std::max(max_g, max_h), kMaxTraj);
        return WT_ERR_CAPACITY;
    }
    // per-problem matrix offsets: two matrices of min x munkres_ld(max) floats each
    std::vector<int64_t> mat_offsets(n_problems + 1, 0);
    for (size_t p = 0; p < n_problems; ++p) {
        const int64_t a = g_ntraj[(p / n_classes % n_streams) * n_classes + p % n_classes], b = h_ntraj[p];
        mat_offsets[p + 1] = mat_offsets[p] + 2 * std::min(a, b) * (int64_t)munkres_ld((int)std::max(a, b));
    }
    const int64_t matrix_floats = mat_offsets[n_problems];
    const size_t wsb = wt_mot_identity_workspace(k_sets, n_streams, n_classes, max_g, max_h, matrix_floats);
    if (!wsb) return WT_ERR_CAPACITY;
    if (workspace_limit_bytes && wsb > workspace_limit_bytes) {
        wt::set_error("identity evaluation workspace too small: need %zu bytes, the limit is %zu (score fewer results per call)", wsb, workspace_limit_bytes);
        return WT_ERR_INVALID;
    }
    WT_TRY(wt::ensure_device());
    wt::StagedTrackInput staged;
    WT_TRY(staged.upload(in));
    const size_t nh = (size_t)staged.n_hyp;
    wt::DevBuf dgn, dhn, dmo, dcnt, dmatch, dws;
    WT_TRY(dgn.upload(g_ntraj, 4 * (size_t)n_streams * n_classes)); WT_TRY(dhn.upload(h_ntraj, 4 * n_problems));
    WT_TRY(dmo.upload(mat_offsets.data(), 8 * (n_problems + 1)));
    WT_TRY(dcnt.alloc(8 * n_problems * 6));
    if (hyp_idmatch) WT_TRY(dmatch.alloc(16 * nh));
    WT_TRY(dws.alloc(wsb));
    WT_TRY(launch(staged.dev, staged.n_hyp, dgn.as<int32_t>(), dhn.as<int32_t>(), dmo.as<int64_t>(), matrix_floats, thr, max_g, max_h,
                  dcnt.as<int64_t>(), hyp_idmatch ? dmatch.as<int64_t>() : nullptr, staged.status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(staged.finish("identity evaluation"));
    if (n_problems) WT_HIP(hipMemcpy(id_counts, dcnt.p, 8 * n_problems * 6, hipMemcpyDeviceToHost));
    if (nh && hyp_idmatch) WT_HIP(hipMemcpy(hyp_idmatch, dmatch.p, 16 * nh, hipMemcpyDeviceToHost));
    return WT_OK;
}

}  // extern "C"
