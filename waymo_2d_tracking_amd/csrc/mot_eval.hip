// CLEAR-MOT evaluation of tracking results on gfx950 (include/waymotrack.h, "MOT evaluation"; DESIGN.md has the definition).
//
// Same shape as the SORT engine: one 64-lane wavefront owns one independent problem = (result set k, stream s, class c)
// and walks the stream's frames in order; a sweep of K settings is K times as many wavefronts in the same launch.
// Per frame: compact the class's ground-truth rows and hypotheses (ballot + popcount), carry over last frame's pairs
// that still clear the threshold, assign the rest with the Munkres of sort_device.h on the gated float32 IoU matrix
// (LDS when it fits, workspace otherwise), then count for both difficulty levels.  The IoU sum is accumulated one
// match after the other in ground-truth row order, so that it is the same float64 number on every run and on the CPU.
// Compile with -ffp-contract=off (IoU in the operation order of tracking/sort/sort.py:34-47; eval_device.h has it).
#include "eval_device.h"
#include "eval_host.h"

using namespace wtdev;

namespace {

constexpr int kMaxBoxes = 4096;               // per side and (frame, class): the limit of munkres_wave
constexpr int kLdsCostFloats = 8192;          // 32 KiB of cost matrix in LDS per wave
constexpr size_t kLdsZmaskMax = 32 * 1024;    // zero bitmaps stay in LDS up to here (about 500 x 500), in the workspace beyond

struct Caps {
    int capN;                // boxes per side of one (frame, class)
    int max_ids;             // ground-truth ids per stream
    int lds_cost;            // floats of cost matrix in LDS
    bool cost_g, zmask_g;
    size_t lds_bytes;
};

struct Workspace {                       // device pointers carved from one block; everything is per problem
    int *gidx, *hidx;                    // [capN] rows of this class in the frame, relative to the frame's first row
    int *gmatch, *hmatch;                // [capN] matched position on the other side or -1
    int *rlist, *clist;                  // [capN] positions still unmatched after the carry-over
    int *last, *last_f;                  // [max_ids] hypothesis id the object was last matched to, and in which frame (-1 never)
    float* cost_g;                       // [capN * (capN | 1)] when the matrix can outgrow the LDS share
    unsigned long long* zmask_g;         // [capN * ceil(capN / 64)] when the bitmaps can
    size_t bytes;
};

int pick_caps(int64_t max_frame_boxes, int32_t max_gt_ids, Caps* c) {
    if (max_frame_boxes > kMaxBoxes) {
        wt::set_error("%lld boxes of one class in one frame: the assignment kernel takes at most %d a side", (long long)max_frame_boxes, kMaxBoxes);
        return WT_ERR_CAPACITY;
    }
    if (max_gt_ids < 0) { wt::set_error("max_gt_ids is negative"); return WT_ERR_INVALID; }
    c->capN = (int)(max_frame_boxes > 0 ? max_frame_boxes : 1);
    c->max_ids = max_gt_ids > 0 ? max_gt_ids : 1;
    const int64_t full = (int64_t)c->capN * (c->capN | 1);
    c->lds_cost = (int)(full < kLdsCostFloats ? full : kLdsCostFloats);
    c->cost_g = full > kLdsCostFloats;
    const size_t W = (size_t)(c->capN + 63) / 64;
    c->zmask_g = (size_t)c->capN * W * 8 > kLdsZmaskMax;
    const size_t stars = wt::align_up((size_t)3 * c->capN * sizeof(int), 16);
    c->lds_bytes = wt::align_up((size_t)c->lds_cost * sizeof(float), 16) + stars + (c->zmask_g ? 0 : (size_t)c->capN * W * 8) + 16;
    return WT_OK;
}

Workspace carve(void* base, size_t n_problems, const Caps& c) {
    wt::Carver cv(base);
    Workspace w;
    const size_t W = (size_t)(c.capN + 63) / 64;
    w.gidx = cv.take<int>(n_problems * c.capN);
    w.hidx = cv.take<int>(n_problems * c.capN);
    w.gmatch = cv.take<int>(n_problems * c.capN);
    w.hmatch = cv.take<int>(n_problems * c.capN);
    w.rlist = cv.take<int>(n_problems * c.capN);
    w.clist = cv.take<int>(n_problems * c.capN);
    w.last = cv.take<int>(n_problems * c.max_ids);
    w.last_f = cv.take<int>(n_problems * c.max_ids);
    w.cost_g = cv.take<float>(c.cost_g ? n_problems * (size_t)c.capN * (c.capN | 1) : 1);
    w.zmask_g = cv.take<unsigned long long>(c.zmask_g ? n_problems * (size_t)c.capN * W : 1);
    w.bytes = cv.off;
    return w;
}

__global__ __launch_bounds__(kWave) void mot_eval_kernel(
    Boxes G, const int32_t* __restrict__ g_cat, const int32_t* __restrict__ g_level, const int32_t* __restrict__ g_id,
    const int64_t* __restrict__ frame_gt_offsets, const int64_t* __restrict__ stream_frame_offsets, long long n_frames,
    int n_streams, int C, const int64_t* __restrict__ set_row_offsets, const int64_t* __restrict__ frame_hyp_offsets,
    Boxes H, const int32_t* __restrict__ h_cat, const int32_t* __restrict__ h_id, Thresholds thr_all, Caps caps, Workspace ws,
    int64_t* __restrict__ counts, double* __restrict__ iou_sum, int64_t* __restrict__ hyp_match, uint8_t* __restrict__ hyp_switch,
    int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const size_t p = blockIdx.x;
    int k, s, c;
    decode_problem(p, n_streams, C, &k, &s, &c);
    const int capN = caps.capN;
    const double thr = thr_all.v[c - 1];

    float* lds_cost = reinterpret_cast<float*>(smem);
    char* mk = smem + (((size_t)caps.lds_cost * sizeof(float) + 15) / 16) * 16;
    MunkresMem L;
    L.row_star = reinterpret_cast<int*>(mk);
    L.row_prime = L.row_star + capN;
    L.col_star = L.row_star + 2 * capN;
    const size_t Wcap = (size_t)(capN + 63) / 64;
    L.zmask = caps.zmask_g ? ws.zmask_g + p * (size_t)capN * Wcap
                           : reinterpret_cast<unsigned long long*>(mk + (((size_t)3 * capN * sizeof(int) + 15) / 16) * 16);
    L.help = nullptr;
    L.cost_in_lds = 0;

    int* gidx = ws.gidx + p * capN;
    int* hidx = ws.hidx + p * capN;
    int* gmatch = ws.gmatch + p * capN;
    int* hmatch = ws.hmatch + p * capN;
    int* rlist = ws.rlist + p * capN;
    int* clist = ws.clist + p * capN;
    int* last = ws.last + p * caps.max_ids;
    int* last_f = ws.last_f + p * caps.max_ids;
    float* cost_g = caps.cost_g ? ws.cost_g + p * (size_t)capN * (capN | 1) : nullptr;
    for (int i = lane; i < caps.max_ids; i += kWave) { last[i] = -1; last_f[i] = -1; }
    wsync();

    long long n_gt[2] = {0, 0}, n_tp[2] = {0, 0}, n_sw[2] = {0, 0}, n_fp = 0;      // [0] LEVEL_1, [1] LEVEL_2; wave-uniform
    double sum[2] = {0., 0.};
    int err = 0;
    const long long f0 = stream_frame_offsets[s], f1 = stream_frame_offsets[s + 1];
    const long long hbase = set_row_offsets[k];
    const int64_t* fho = frame_hyp_offsets + (size_t)k * (size_t)(n_frames + 1);
    for (long long f = f0; f < f1 && !err; ++f) {
        const int fo = (int)(f - f0);
        const long long g0 = frame_gt_offsets[f], g1 = frame_gt_offsets[f + 1];
        const long long h0 = hbase + fho[f], h1 = hbase + fho[f + 1];
        // ---- this class's rows of the frame, in file order ----
        const int ng = compact_rows(g_cat, g0, g1, c, gidx, capN);
        const int nh = compact_rows(h_cat, h0, h1, c, hidx, capN);
        if (ng > capN || nh > capN) { err = kErrCapacity; break; }
        if (ng == 0 && nh == 0) continue;
        for (int i = lane; i < ng; i += kWave) gmatch[i] = -1;
        for (int j = lane; j < nh; j += kWave) hmatch[j] = -1;
        wsync();
        // ---- 1. carry over: (o, h) of the previous frame stays when both are here and still overlap enough ----
        if (ng > 0 && nh > 0 && fo > 0) {
            for (int base = 0; base < ng; base += kWave) {
                const int i = base + lane;
                int want = -1;
                long long grow = 0;
                if (i < ng) {
                    grow = g0 + gidx[i];
                    const int o = g_id[grow];
                    if (last_f[o] == fo - 1) want = last[o];
                }
                if (__ballot(want >= 0) == 0ull) continue;
                int found = -1;
                for (int j = 0; j < nh; ++j) {
                    const int id = h_id[h0 + hidx[j]];                 // the same address in every lane
                    if (id == want) found = j;
                }
                if (want >= 0 && found >= 0) {
                    double gb[4], hb[4];
                    G.get(grow, gb);
                    H.get(h0 + hidx[found], hb);
                    if (iou_dd(gb, hb) >= thr) { gmatch[i] = found; hmatch[found] = i; }
                }
            }
            wsync();
        }
        // ---- 2. the rest: Munkres on the gated IoU matrix ----
        const int nr = compact_wave(0, ng, [=](int i) { return gmatch[i] < 0; }, rlist, capN);
        const int nc = compact_wave(0, nh, [=](int j) { return hmatch[j] < 0; }, clist, capN);
        wsync();
        if (nr > 0 && nc > 0) {
            const bool transposed = nc < nr;               // linear_assignment transposes when there are fewer columns than rows
            const int n = transposed ? nc : nr, m = transposed ? nr : nc;
            const int ld = munkres_ld(m);
            const bool in_lds = (long)n * ld <= (long)caps.lds_cost;
            if (!in_lds && !cost_g) { err = kErrCapacity; break; }
            float* Cm = in_lds ? lds_cost : cost_g;
            bool gate = false;
            for (int cbase = 0; cbase < nc; cbase += kWave) {        // lane = hypothesis, ground-truth rows one after the other
                const int jj = cbase + lane;
                double hb[4] = {0., 0., 0., 0.};
                if (jj < nc) H.get(h0 + hidx[clist[jj]], hb);
                for (int ii = 0; ii < nr; ++ii) {
                    double gb[4];
                    G.get(g0 + gidx[rlist[ii]], gb);
                    const double v = iou_dd(gb, hb);
                    const float g = (v >= thr) ? (float)v : 0.f;
                    if (jj < nc) {
                        const int r = transposed ? jj : ii, cc = transposed ? ii : jj;
                        Cm[r * ld + cc] = -g;
                        gate = gate || (g > 0.f);
                    }
                }
            }
            wsync();
            if (__ballot(gate) != 0ull) {                             // nothing passes the gate: no pair would be kept
                const int rc = in_lds ? munkres_wave(lds_cost, n, m, ld, L) : munkres_wave(cost_g, n, m, ld, L);
                if (rc) { err = rc; break; }
                for (int ii = lane; ii < nr; ii += kWave) {
                    const int jj = transposed ? L.col_star[ii] : L.row_star[ii];
                    if (jj >= 0) {
                        const int i = rlist[ii], j = clist[jj];
                        double gb[4], hb[4];
                        G.get(g0 + gidx[i], gb);
                        H.get(h0 + hidx[j], hb);
                        const double v = iou_dd(gb, hb);
                        if (v >= thr && (float)v > 0.f) { gmatch[i] = j; hmatch[j] = i; }
                    }
                }
            }
            wsync();
        }
        // ---- 3. count ----
        for (int base = 0; base < ng; base += kWave) {
            const int i = base + lane;
            const bool act = i < ng;
            bool matched = false, easy = false, sw = false;
            double v = 0.;
            if (act) {
                const long long grow = g0 + gidx[i];
                easy = g_level[grow] != 2;
                const int j = gmatch[i];
                if (j >= 0) {
                    matched = true;
                    const long long hrow = h0 + hidx[j];
                    const int o = g_id[grow], hid = h_id[hrow];
                    double gb[4], hb[4];
                    G.get(grow, gb);
                    H.get(hrow, hb);
                    v = iou_dd(gb, hb);
                    sw = last_f[o] >= 0 && last[o] != hid;
                    last[o] = hid;
                    last_f[o] = fo;
                    if (hyp_match) hyp_match[hrow] = grow;
                    if (hyp_switch && sw) hyp_switch[hrow] = 1;
                }
            }
            const unsigned long long m2 = __ballot(matched), m1 = __ballot(matched && easy);
            n_gt[1] += __popcll(__ballot(act));
            n_gt[0] += __popcll(__ballot(act && easy));
            n_tp[1] += __popcll(m2);
            n_tp[0] += __popcll(m1);
            n_sw[1] += __popcll(__ballot(sw));
            n_sw[0] += __popcll(__ballot(sw && easy));
            for (unsigned long long todo = m2; todo; todo &= todo - 1ull) {      // one match after the other, in row order
                const int b = __builtin_ctzll(todo);
                const double vb = bcast_d(v, b);
                sum[1] = sum[1] + vb;
                if ((m1 >> b) & 1ull) sum[0] = sum[0] + vb;
            }
        }
        for (int base = 0; base < nh; base += kWave) {
            const int j = base + lane;
            const bool um = (j < nh) && hmatch[j] < 0;
            n_fp += __popcll(__ballot(um));
            if (um && hyp_match) hyp_match[h0 + hidx[j]] = -1;
        }
        wsync();
    }
    if (err && lane == 0) atomicMax(status, err);
    if (lane < 2) {                                  // lane = level
        int64_t* o = counts + (p * 2 + lane) * 5;
        const long long gt = lane ? n_gt[1] : n_gt[0], tp = lane ? n_tp[1] : n_tp[0], isw = lane ? n_sw[1] : n_sw[0];
        o[0] = gt; o[1] = tp; o[2] = gt - tp; o[3] = n_fp; o[4] = isw;
        iou_sum[p * 2 + lane] = lane ? sum[1] : sum[0];
    }
}

__global__ void mot_fill_kernel(long long n, int64_t* __restrict__ hyp_match, uint8_t* __restrict__ hyp_switch) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (hyp_match) hyp_match[i] = -2;
    if (hyp_switch) hyp_switch[i] = 0;
}

// wt_mot_eval_dev on an input whose pointers are device pointers
int launch(const wt::TrackInput& in, int64_t n_hyp, const double* thr, int64_t max_frame_boxes, int32_t max_gt_ids,
           int64_t* counts, double* iou_sum, int64_t* hyp_match, uint8_t* hyp_switch, int32_t* status_dev,
           void* workspace, size_t workspace_bytes, hipStream_t stream) {
    WT_TRY(wt::ensure_device());
    if (in.k_sets < 1 || in.n_streams < 0 || in.n_frames < 0 || in.n_gt < 0 || n_hyp < 0 || !thr || !counts || !iou_sum || !status_dev) {
        wt::set_error("wt_mot_eval: bad argument");
        return WT_ERR_INVALID;
    }
    if (in.n_classes < 1 || in.n_classes > kMaxClasses) { wt::set_error("wt_mot_eval: n_classes must be 1..%d", kMaxClasses); return WT_ERR_INVALID; }
    Caps caps;
    WT_TRY(pick_caps(max_frame_boxes, max_gt_ids, &caps));
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    if (n_hyp > 0 && (hyp_match || hyp_switch))
        hipLaunchKernelGGL(mot_fill_kernel, dim3((unsigned)((n_hyp + 255) / 256)), dim3(256), 0, stream, (long long)n_hyp, hyp_match, hyp_switch);
    const size_t n_problems = (size_t)in.k_sets * (size_t)in.n_streams * (size_t)in.n_classes;
    if (n_problems == 0) { WT_HIP(hipGetLastError()); return WT_OK; }
    if (n_problems > 0x7fffffffull) { wt::set_error("wt_mot_eval: %zu problems in one call", n_problems); return WT_ERR_CAPACITY; }
    Workspace ws = carve(wt::align_ptr(workspace), n_problems, caps);
    if (!workspace || workspace_bytes < ws.bytes + 256) {
        wt::set_error("evaluation workspace too small: need %zu bytes, have %zu", ws.bytes + 256, workspace_bytes);
        return WT_ERR_CAPACITY;
    }
    if (caps.lds_bytes > 48 * 1024)
        WT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mot_eval_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)caps.lds_bytes));
    const Boxes G = {in.gx, in.gy, in.gw, in.gh}, H = {in.hx, in.hy, in.hw, in.hh};
    hipLaunchKernelGGL(mot_eval_kernel, dim3((unsigned)n_problems), dim3(kWave), caps.lds_bytes, stream, G, in.g_category, in.g_level, in.g_id,
                       in.frame_gt_offsets, in.stream_frame_offsets, (long long)in.n_frames, (int)in.n_streams, (int)in.n_classes,
                       in.set_row_offsets, in.frame_hyp_offsets, H, in.h_category, in.h_id, make_thresholds(thr, in.n_classes), caps, ws,
                       counts, iou_sum, hyp_match, hyp_switch, (int*)status_dev);
    WT_HIP(hipGetLastError());
    return WT_OK;
}

}  // namespace

extern "C" {

size_t wt_mot_eval_workspace(int32_t k_sets, int32_t n_streams, int32_t n_classes, int64_t max_frame_boxes, int32_t max_gt_ids) {
    Caps c;
    if (k_sets < 1 || n_streams < 0 || n_classes < 1 || pick_caps(max_frame_boxes, max_gt_ids, &c) != WT_OK) return 0;
    return carve(nullptr, (size_t)k_sets * (size_t)n_streams * (size_t)n_classes, c).bytes + 256;
}

int wt_mot_eval_dev(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                    const int32_t* g_category, const int32_t* g_level, const int32_t* g_id,
                    int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                    int32_t k_sets, int64_t n_hyp, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                    const double* hx, const double* hy, const double* hw, const double* hh,
                    const int32_t* h_category, const int32_t* h_id,
                    int32_t n_classes, const double* thr, int64_t max_frame_boxes, int32_t max_gt_ids,
                    int64_t* counts, double* iou_sum, int64_t* hyp_match, uint8_t* hyp_switch, int32_t* status_dev,
                    void* workspace, size_t workspace_bytes, void* stream_) {
    const wt::TrackInput in = {n_gt, gx, gy, gw, gh, g_category, g_level, g_id, n_frames, frame_gt_offsets, n_streams, stream_frame_offsets,
                               k_sets, set_row_offsets, frame_hyp_offsets, hx, hy, hw, hh, h_category, h_id, n_classes};
    return launch(in, n_hyp, thr, max_frame_boxes, max_gt_ids, counts, iou_sum, hyp_match, hyp_switch, status_dev, workspace, workspace_bytes,
                  (hipStream_t)stream_);
}

int wt_mot_eval_host(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                     const int32_t* g_category, const int32_t* g_level, const int32_t* g_id,
                     int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                     int32_t k_sets, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                     const double* hx, const double* hy, const double* hw, const double* hh,
                     const int32_t* h_category, const int32_t* h_id,
                     int32_t n_classes, const double* thr,
                     int64_t* counts, double* iou_sum, int64_t* hyp_match, uint8_t* hyp_switch) {
    const wt::TrackInput in = {n_gt, gx, gy, gw, gh, g_category, g_level, g_id, n_frames, frame_gt_offsets, n_streams, stream_frame_offsets,
                               k_sets, set_row_offsets, frame_hyp_offsets, hx, hy, hw, hh, h_category, h_id, n_classes};
    WT_TRY(wt::check_track_layout(in, "wt_mot_eval_host", thr && counts && iou_sum, kMaxClasses));
    // an id is valid when it is not negative; on the way, the most boxes of one class in one frame and the largest ground-truth id
    std::vector<int64_t> per_class((size_t)n_classes);
    int64_t max_boxes = 0;
    int32_t max_id = -1;
    auto ids_unique = [&](const int32_t* cat, const int32_t* id, int64_t r0, int64_t r1) {
        std::fill(per_class.begin(), per_class.end(), 0);
        return wt::frame_ids_unique(cat, id, r0, r1, n_classes, [&](int64_t r) {
            if (id[r] < 0) return false;
            max_boxes = std::max(max_boxes, ++per_class[(size_t)cat[r] - 1]);
            return true;
        });
    };
    WT_TRY(wt::walk_track_frames(in,
        [&](int32_t, int64_t f, int64_t r0, int64_t r1) {
            for (int64_t r = r0; r < r1; ++r) {              // every row, whatever its class: the kernel indexes by the id
                if (g_id[r] < 0) { wt::set_error("ground-truth row %lld: negative object id", (long long)r); return WT_ERR_INVALID; }
                if (g_id[r] > max_id) max_id = g_id[r];
            }
            if (ids_unique(g_category, g_id, r0, r1)) return WT_OK;
            wt::set_error("ground truth: an object id occurs twice in frame %lld", (long long)f);
            return WT_ERR_INVALID;
        },
        [&](int32_t k, int32_t, int64_t f, int64_t r0, int64_t r1) {
            if (ids_unique(h_category, h_id, r0, r1)) return WT_OK;
            wt::set_error("result set %d: an object id is negative or occurs twice in frame %lld", (int)k, (long long)f);
            return WT_ERR_INVALID;
        }));
    if (max_boxes > kMaxBoxes) {
        wt::set_error("%lld boxes of one class in one frame: the assignment kernel takes at most %d a side", (long long)max_boxes, kMaxBoxes);
        return WT_ERR_CAPACITY;
    }
    WT_TRY(wt::ensure_device());
    wt::StagedTrackInput staged;
    WT_TRY(staged.upload(in));
    const size_t nh = (size_t)staged.n_hyp, n_problems = (size_t)k_sets * (size_t)n_streams * (size_t)n_classes;
    wt::DevBuf dcnt, dsum, dmatch, dswitch, dws;
    WT_TRY(dcnt.alloc(8 * n_problems * 10)); WT_TRY(dsum.alloc(8 * n_problems * 2));
    if (hyp_match) WT_TRY(dmatch.alloc(8 * nh));
    if (hyp_switch) WT_TRY(dswitch.alloc(nh));
    const size_t wsb = wt_mot_eval_workspace(k_sets, n_streams, n_classes, max_boxes, max_id + 1);
    if (!wsb) return WT_ERR_CAPACITY;
    WT_TRY(dws.alloc(wsb));
    WT_TRY(launch(staged.dev, staged.n_hyp, thr, max_boxes, max_id + 1, dcnt.as<int64_t>(), dsum.as<double>(),
                  hyp_match ? dmatch.as<int64_t>() : nullptr, hyp_switch ? dswitch.as<uint8_t>() : nullptr, staged.status.as<int32_t>(),
                  dws.p, wsb, nullptr));
    WT_TRY(staged.finish("evaluation"));
    if (n_problems) {
        WT_HIP(hipMemcpy(counts, dcnt.p, 8 * n_problems * 10, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(iou_sum, dsum.p, 8 * n_problems * 2, hipMemcpyDeviceToHost));
    }
    if (nh && hyp_match) WT_HIP(hipMemcpy(hyp_match, dmatch.p, 8 * nh, hipMemcpyDeviceToHost));
    if (nh && hyp_switch) WT_HIP(hipMemcpy(hyp_switch, dswitch.p, nh, hipMemcpyDeviceToHost));
    return WT_OK;
}

}  // extern "C"
