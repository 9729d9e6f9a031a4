// Weighted boxes fusion (WBF) and non-maximum weighted (NMW) on gfx950: the merge rules of detnet/ensemble_b.py, one 64-lane
// wavefront per (image, category) group.  The definition is the project's own (tests/wbf_ref.py restates
// it in plain Python): the published algorithm on pixel corner boxes with a defined tie order, not pinned against the
// ensemble_boxes package.  float64, compiled with -ffp-contract=off: every product, sum and quotient is rounded on its own and in
// the order of the restatement, so the results are compared with ==.
//
// Per group (n rows): one coalesced read of 40*n B (AoS rows -> SoA), a stable rank by counting, then the serial walk in score
// order.  A row's step: the lanes stride over the clusters made so far and take the IoU with each cluster's match box (the fused
// box for WBF, the first member for NMW), each lane keeps its best under strict >, a 6-step butterfly takes the maximum with ties
// to the lowest cluster index, and lanes 0..3 update the chosen cluster's sums (one coordinate each).  Clusters only ever change
// between two barriers of the one wave, so LDS ordering is all the walk needs.  Rows, ranks and cluster state live in LDS
// (136 B/row) while the group fits 64 KiB; larger groups run the same code on a global-memory slice (template<bool kLds>).
#include "common.h"

namespace {

constexpr int kWave = 64;
constexpr size_t kLdsBudget = 64 * 1024;          // the budget of ensemble.hip
constexpr size_t kScratchRowBytes = 144;          // group_mem_bytes(1) rounded up to 16: every group's slice stays 16-B aligned
constexpr int64_t kMaxGroupRows = 1 << 24;        // the in-group indices are int

struct FuseMem {
    double* s;      // rows: score and corners
    double* x1;
    double* y1;
    double* x2;
    double* y2;
    double* mb;     // clusters, 4 x cap: the box rows are matched against (WBF: fused box, NMW: first member)
    double* S;      // clusters: WBF sum of scores, NMW sum of score * IoU
    double* B;      // clusters, 4 x cap: weighted corner sums
    double* conf;   // clusters: NMW first member's score; WBF filled in after the walk
    int* pos;       // pos[rank] = row
    int* cnt;       // clusters: members
    int* rowcl;     // rows: cluster (creation index)
    int* opos;      // clusters: position in the group's output
};

__host__ __device__ inline size_t group_mem_bytes(size_t cap) { return cap * (15 * sizeof(double) + 4 * sizeof(int)); }

__host__ __device__ inline size_t lds_capacity_rows() { return kLdsBudget / group_mem_bytes(1); }

__device__ __forceinline__ FuseMem carve(char* base, size_t cap) {
    FuseMem m;
    double* d = reinterpret_cast<double*>(base);
    m.s = d; m.x1 = d + cap; m.y1 = d + 2 * cap; m.x2 = d + 3 * cap; m.y2 = d + 4 * cap;
    m.mb = d + 5 * cap; m.S = d + 9 * cap; m.B = d + 10 * cap; m.conf = d + 14 * cap;
    int* ip = reinterpret_cast<int*>(d + 15 * cap);
    m.pos = ip; m.cnt = ip + cap; m.rowcl = ip + 2 * cap; m.opos = ip + 3 * cap;
    return m;
}

// "a comes before b": descending value, ties to the lower index.  NaN (never in validated input) sorts first so that the ranks
// stay a permutation whatever the data.
__device__ __forceinline__ bool before(double a, int ia, double b, int ib) {
    const bool an = a != a, bn = b != b;
    if (an != bn) return an;
    if (!an && a != b) return a > b;
    return ia < ib;
}

// IoU of corner boxes, area = (x2 - x1) * (y2 - y1); exactly 0 when the boxes do not overlap
__device__ __forceinline__ double iou_corners(double ax1, double ay1, double ax2, double ay2, double bx1, double by1, double bx2,
                                              double by2) {
    double iw = (ax2 < bx2 ? ax2 : bx2) - (ax1 > bx1 ? ax1 : bx1); if (!(iw > 0.)) iw = 0.;
    double ih = (ay2 < by2 ? ay2 : by2) - (ay1 > by1 ? ay1 : by1); if (!(ih > 0.)) ih = 0.;
    const double inter = iw * ih;
    if (inter == 0.) return 0.;
    const double area_a = (ax2 - ax1) * (ay2 - ay1), area_b = (bx2 - bx1) * (by2 - by1);
    return inter / ((area_a + area_b) - inter);
}

// One group.  in: n rows [score, x, y, w, h]; out: the clusters as rows [conf, x1, y1, w, h] by descending conf.
__device__ void fuse_group(const double* __restrict__ in, int n, double wsum, bool nmw, double thr, const FuseMem& m, size_t cap,
                           double* __restrict__ out, int32_t* __restrict__ out_members, int32_t* __restrict__ row_cluster,
                           int64_t* out_count) {
    const int lane = threadIdx.x;
    for (int j = lane; j < 5 * n; j += kWave) {           // s, x1, y1, x2, y2 are consecutive arrays of cap
        const int r = j / 5, c = j - 5 * r;
        m.s[c * cap + r] = in[j];
    }
    __syncthreads();
    for (int i = lane; i < n; i += kWave) {               // [x, y, w, h] -> corners (own row only)
        m.x2[i] = m.x1[i] + m.x2[i];
        m.y2[i] = m.y1[i] + m.y2[i];
    }
    for (int i = lane; i < n; i += kWave) {               // scores are final after the load: rank by counting
        const double si = m.s[i];
        int c = 0;
        for (int j = 0; j < n; ++j) c += before(m.s[j], j, si, i) ? 1 : 0;
        m.pos[c] = i;
    }
    __syncthreads();
    int nc = 0;                                            // wave-uniform
    for (int r = 0; r < n; ++r) {
        const int i = m.pos[r];
        const double s = m.s[i], bx1 = m.x1[i], by1 = m.y1[i], bx2 = m.x2[i], by2 = m.y2[i];
        double best = thr;
        int bi = 0x7fffffff;
        for (int c = lane; c < nc; c += kWave) {
            const double v = iou_corners(m.mb[c], m.mb[cap + c], m.mb[2 * cap + c], m.mb[3 * cap + c], bx1, by1, bx2, by2);
            if (v > best) { best = v; bi = c; }           // ascending c: the first of equal IoUs stays
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(best, o, kWave);
            const int oi = __shfl_xor(bi, o, kWave);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        const bool join = bi != 0x7fffffff;                // every lane holds the same (best, bi)
        const int k = join ? bi : nc;
        const double bl = lane == 0 ? bx1 : (lane == 1 ? by1 : (lane == 2 ? bx2 : by2));      // lane q < 4 owns corner q
        // the weight of this member: WBF its score, NMW score * IoU with the first member (itself for a new cluster)
        const double wt = nmw ? s * (join ? best : iou_corners(bx1, by1, bx2, by2, bx1, by1, bx2, by2)) : s;
        double S_old = 0., B_old = 0.;
        int cnt_old = 0;
        if (join) {
            S_old = m.S[k];
            cnt_old = m.cnt[k];
            if (lane < 4) B_old = m.B[lane * cap + k];
        }
        __syncthreads();                                   // all reads of cluster k before its update
        if (lane < 4) {
            const double wb = wt * bl;
            if (join) {
                const double S_new = S_old + wt, B_new = B_old + wb;
                m.B[lane * cap + k] = B_new;
                if (!nmw) m.mb[lane * cap + k] = B_new / S_new;
                if (lane == 0) { m.S[k] = S_new; m.cnt[k] = cnt_old + 1; }
            } else {
                m.B[lane * cap + k] = wb;
                m.mb[lane * cap + k] = bl;
                if (lane == 0) { m.S[k] = wt; m.cnt[k] = 1; m.conf[k] = s; }
            }
            if (lane == 0) m.rowcl[i] = k;
        }
        if (!join) ++nc;
        __syncthreads();                                   // the update is visible to the next row's reads
    }
    // confidence and output box per cluster
    for (int c = lane; c < nc; c += kWave) {
        if (nmw) {
            const double W = m.S[c];
            for (int q = 0; q < 4; ++q) m.mb[q * cap + c] = m.B[q * cap + c] / W;
        } else {
            const double cn = (double)m.cnt[c];
            m.conf[c] = ((m.S[c] / cn) * (wsum < cn ? wsum : cn)) / wsum;
        }
    }
    __syncthreads();
    for (int c = lane; c < nc; c += kWave) {               // clusters by conf, descending and stable in creation order
        const double cc = m.conf[c];
        int p = 0;
        for (int j = 0; j < nc; ++j) p += before(m.conf[j], j, cc, c) ? 1 : 0;
        m.opos[c] = p;
        double* o = out + 5 * (size_t)p;
        const double x1 = m.mb[c], y1 = m.mb[cap + c];
        o[0] = cc; o[1] = x1; o[2] = y1; o[3] = m.mb[2 * cap + c] - x1; o[4] = m.mb[3 * cap + c] - y1;
        if (out_members) out_members[p] = m.cnt[c];
    }
    __syncthreads();
    if (row_cluster)
        for (int i = lane; i < n; i += kWave) row_cluster[i] = m.opos[m.rowcl[i]];
    if (lane == 0) *out_count = nc;
}

template <bool kLds>
__global__ __launch_bounds__(kWave) void fuse_groups_kernel(
    const double* __restrict__ dets5, const int64_t* __restrict__ group_offsets, const double* __restrict__ group_wsum,
    int64_t n_groups, int method, double thr, double* __restrict__ out5, int32_t* __restrict__ out_members,
    int32_t* __restrict__ row_cluster, int64_t* __restrict__ out_counts, char* scratch, size_t lds_cap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t o0 = group_offsets[g];
        const int64_t rows = group_offsets[g + 1] - o0;
        if (rows <= 0) {
            if (threadIdx.x == 0) out_counts[g] = 0;
            continue;
        }
        // a group larger than the caller's max_group_rows has no memory to run in: reported, never run
        if (rows > kMaxGroupRows || (kLds && (size_t)rows > lds_cap)) {
            if (threadIdx.x == 0) out_counts[g] = -1;
            continue;
        }
        const int n = (int)rows;
        // LDS: arrays sized lds_cap.  Global scratch: this group's slice holds exactly n rows of every array.
        const size_t cap = kLds ? lds_cap : (size_t)n;
        const FuseMem m = carve(kLds ? smem : scratch + (size_t)o0 * kScratchRowBytes + (size_t)g * 64, cap);
        fuse_group(dets5 + 5 * o0, n, group_wsum[g], method == 1, thr, m, cap, out5 + 5 * o0,
                   out_members ? out_members + o0 : nullptr, row_cluster ? row_cluster + o0 : nullptr, out_counts + g);
        __syncthreads();
    }
}

size_t workspace_bytes_for(int64_t n_rows, int64_t n_groups, int64_t max_group_rows) {
    if (n_rows < 0 || n_groups < 0 || max_group_rows < 0) return 0;
    if ((size_t)max_group_rows <= lds_capacity_rows()) return 0;
    return (size_t)n_rows * kScratchRowBytes + (size_t)n_groups * 64 + 256;
}

int launch_fuse(const double* dets5, const int64_t* group_offsets, const double* group_wsum, int64_t n_rows, int64_t n_groups,
                int64_t max_group_rows, int method, double thr, double* out5, int32_t* out_members, int32_t* row_cluster,
                int64_t* out_counts, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (method != 0 && method != 1) { wt::set_error("method must be 0 (weighted_fusion) or 1 (nmw), got %d", method); return WT_ERR_INVALID; }
    if (n_rows < 0 || n_groups < 0 || max_group_rows < 0) {
        wt::set_error("negative size: n_rows %lld, n_groups %lld, max_group_rows %lld", (long long)n_rows, (long long)n_groups,
                      (long long)max_group_rows);
        return WT_ERR_INVALID;
    }
    if (max_group_rows > kMaxGroupRows) {
        wt::set_error("max_group_rows %lld: a group holds at most %lld rows", (long long)max_group_rows, (long long)kMaxGroupRows);
        return WT_ERR_INVALID;
    }
    if (n_groups == 0) return WT_OK;
    if (!dets5 || !group_offsets || !group_wsum || !out5 || !out_counts) { wt::set_error("null pointer argument"); return WT_ERR_INVALID; }
    const size_t cap = (size_t)(max_group_rows > 0 ? max_group_rows : 1);
    const unsigned grid = (unsigned)(n_groups < (1 << 20) ? n_groups : (1 << 20));
    if (cap <= lds_capacity_rows()) {
        hipLaunchKernelGGL(fuse_groups_kernel<true>, dim3(grid), dim3(kWave), group_mem_bytes(cap), stream, dets5, group_offsets,
                           group_wsum, n_groups, method, thr, out5, out_members, row_cluster, out_counts, (char*)nullptr, cap);
    } else {
        const size_t need = workspace_bytes_for(n_rows, n_groups, max_group_rows);
        if (!workspace || workspace_bytes < need) {
            wt::set_error("fusion workspace too small: need %zu bytes, have %zu", need, workspace ? workspace_bytes : (size_t)0);
            return WT_ERR_INVALID;
        }
        hipLaunchKernelGGL(fuse_groups_kernel<false>, dim3(grid), dim3(kWave), 0, stream, dets5, group_offsets, group_wsum,
                           n_groups, method, thr, out5, out_members, row_cluster, out_counts, (char*)workspace, (size_t)0);
    }
    WT_HIP(hipGetLastError());
    return WT_OK;
}

// ---- fusion of K views' wire slots (the device form of: --export per view -> detnet.ensemble_b -> JSON, between the pipeline's
// two score filters) ----------------------------------------------------------------------------------------------------------
// The slot layout and the two passes are those of wt_ensemble_slots_dev (ensemble.hip).  Pass 1, one wavefront per (frame,
// category) group: scan all K * S slots of the frame view by view in slot order; a row is kept when its category is in 1..C,
// w > 0, h > 0 and score * weight >= min_score; the kept rows of the group's own category are gathered, and every view with a kept
// row of ANY category adds its weight to wsum, in view order (ensemble_b.merge_inputs) - so each group's wave derives the frame's
// wsum on its own.  fuse_group merges; clusters with conf > min_score leave as [x, y, w, h, round5(conf)], boxes not truncated.
// Pass 2, one wavefront per frame: the frame's groups in ascending category order into its K * S output slots.
constexpr int kMaxViews = 16;
constexpr int64_t kMaxSlots = 1 << 20;            // K * S <= kMaxGroupRows

// round(np.float64(s), 5) = numpy around: multiply, rint (half to even), divide (not CPython's correctly rounded round)
__device__ __forceinline__ double round5_numpy(double s) { return rint(s * 1e5) / 1e5; }

struct FuseSlotsWs {
    double* rows;      // per group K*S rows of 5: gathered input [score, x, y, w, h], later the final wire rows [x, y, w, h, score]
    double* merged;    // per group K*S rows of 5: fuse_group's output [conf, x, y, w, h]
    int32_t* count;    // per group: final row count
    char* scratch;     // per group `scratch_stride` bytes of group state (global path only)
    size_t scratch_stride;
};

bool fuse_slots_use_lds(int64_t ks) { return (size_t)ks <= lds_capacity_rows(); }

FuseSlotsWs fuse_slots_ws_layout(char* base, int64_t n_groups, size_t ks, bool lds, size_t* total) {
    FuseSlotsWs w;
    size_t off = 0;
    const size_t rows_b = wt::align_up((size_t)n_groups * ks * 5 * sizeof(double));
    w.rows = reinterpret_cast<double*>(base + off); off += rows_b;
    w.merged = reinterpret_cast<double*>(base + off); off += rows_b;
    w.count = reinterpret_cast<int32_t*>(base + off); off += wt::align_up((size_t)n_groups * sizeof(int32_t));
    w.scratch_stride = lds ? 0 : wt::align_up(group_mem_bytes(ks));
    w.scratch = base + off; off += (size_t)n_groups * w.scratch_stride;
    *total = off > 0 ? off : 256;
    return w;
}

template <bool kLds>
__global__ __launch_bounds__(kWave) void fuse_slots_kernel(
    const double* __restrict__ xywhs, const int32_t* __restrict__ category, int64_t n_frames, int S, int K,
    const double* __restrict__ weights, int C, int method, double thr, double min_score, FuseSlotsWs ws) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int64_t n_merged;
    const int lane = threadIdx.x;
    const int64_t N = n_frames * S;
    const size_t ks = (size_t)K * S;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t g = blockIdx.x; g < n_frames * C; g += gridDim.x) {
        const int64_t f = g / C;
        const int c = (int)(g - f * C) + 1;
        double* rows = ws.rows + (size_t)g * ks * 5;
        double* merged = ws.merged + (size_t)g * ks * 5;
        // 1. scan the frame: gather this category's kept rows, add up the weights of the views that kept any row
        int n = 0;
        double wsum = 0.;
        for (int k = 0; k < K; ++k) {
            const double wk = weights[k];
            bool any = false;
            for (int base = 0; base < S; base += kWave) {
                const int s = base + lane;
                bool kept = false, own = false;
                double x = 0., y = 0., w = 0., h = 0., sc = 0.;
                if (s < S) {
                    const int cat = category[(int64_t)k * N + f * S + s];
                    if (cat >= 1 && cat <= C) {
                        const double* p = xywhs + (int64_t)k * 5 * N + f * S + s;
                        w = p[2 * N]; h = p[3 * N];
                        sc = p[4 * N] * wk;
                        kept = (w > 0.) && (h > 0.) && (sc >= min_score);
                        own = kept && cat == c;
                        if (own) { x = p[0]; y = p[N]; }
                    }
                }
                any = any || __ballot(kept) != 0ull;
                const unsigned long long mask = __ballot(own);
                if (own) {
                    double* r = rows + 5 * (size_t)(n + __popcll(mask & below));
                    r[0] = sc; r[1] = x; r[2] = y; r[3] = w; r[4] = h;
                }
                n += __popcll(mask);
            }
            wsum = wsum + (any ? wk : 0.);
        }
        __syncthreads();
        // 2. merge (fuse_group, rows [score, x_left, y_top, w, h])
        if (n > 0) {
            const FuseMem m = carve(kLds ? smem : ws.scratch + (size_t)g * ws.scratch_stride, ks);
            fuse_group(rows, n, wsum, method == 1, thr, m, ks, merged, nullptr, nullptr, &n_merged);
        } else if (lane == 0) {
            n_merged = 0;
        }
        __syncthreads();
        // 3. conf > min_score, float boxes, numpy's round(conf, 5); wire order [x, y, w, h, score]
        const int nm = (int)n_merged;
        int nk = 0;
        for (int base = 0; base < nm; base += kWave) {
            const int r = base + lane;
            bool keep = false;
            double v[5] = {0., 0., 0., 0., 0.};
            if (r < nm) {
                for (int q = 0; q < 5; ++q) v[q] = merged[5 * (size_t)r + q];
                keep = v[0] > min_score;
            }
            const unsigned long long mask = __ballot(keep);
            if (keep) {
                double* o = rows + 5 * (size_t)(nk + __popcll(mask & below));
                o[0] = v[1]; o[1] = v[2]; o[2] = v[3]; o[3] = v[4];
                o[4] = round5_numpy(v[0]);
            }
            nk += __popcll(mask);
        }
        if (lane == 0) ws.count[g] = nk;
        __syncthreads();
    }
}

// pass 2: frame f's groups in ascending category order -> output slots [f * K * S, (f + 1) * K * S); the rest empty
__global__ __launch_bounds__(kWave) void fuse_slots_compact_kernel(int64_t n_frames, int S, int K, int C, FuseSlotsWs ws,
                                                                  double* __restrict__ out_xywhs,
                                                                  int32_t* __restrict__ out_category,
                                                                  int64_t* __restrict__ out_counts) {
    const int lane = threadIdx.x;
    const int64_t ks = (int64_t)K * S;
    const int64_t NO = n_frames * ks;
    for (int64_t f = blockIdx.x; f < n_frames; f += gridDim.x) {
        int64_t o = f * ks;
        for (int c = 0; c < C; ++c) {
            const int64_t g = f * C + c;
            const int cnt = ws.count[g];
            const double* rows = ws.rows + (size_t)g * ks * 5;
            for (int j = lane; j < cnt; j += kWave) {
                for (int q = 0; q < 5; ++q) out_xywhs[q * NO + o + j] = rows[5 * (size_t)j + q];
                out_category[o + j] = c + 1;
            }
            o += cnt;
        }
        for (int64_t j = o + lane; j < (f + 1) * ks; j += kWave) {
            for (int q = 0; q < 5; ++q) out_xywhs[q * NO + j] = 0.;
            out_category[j] = 0;
        }
        if (lane == 0) out_counts[f] = o - f * ks;
    }
}

bool fuse_slots_shape_ok(int64_t n_frames, int64_t slots, int k_views, int n_categories, int method) {
    return n_frames >= 0 && slots >= 0 && slots <= kMaxSlots && k_views >= 1 && k_views <= kMaxViews && n_categories >= 1 &&
           (method == 0 || method == 1) && n_frames <= ((int64_t)1 << 40) / n_categories;
}

}  // namespace

extern "C" {

size_t wt_fuse_slots_workspace(int64_t n_frames, int64_t slots, int k_views, int n_categories, int method) {
    if (!fuse_slots_shape_ok(n_frames, slots, k_views, n_categories, method)) return 0;
    const int64_t ks = (int64_t)k_views * slots;
    size_t total = 0;
    fuse_slots_ws_layout(nullptr, n_frames * n_categories, (size_t)(ks > 0 ? ks : 1), fuse_slots_use_lds(ks), &total);
    return total;
}

int wt_fuse_slots_dev(const double* xywhs, const int32_t* category, int64_t n_frames, int64_t slots, int k_views,
                      const double* weights, int n_categories, int method, double iou_thresh, double min_score,
                      double* out_xywhs, int32_t* out_category, int64_t* out_counts, void* workspace, size_t workspace_bytes,
                      void* stream) {
    WT_TRY(wt::ensure_device());
    if (method != 0 && method != 1) { wt::set_error("method must be 0 (weighted_fusion) or 1 (nmw), got %d", method); return WT_ERR_INVALID; }
    if (k_views < 1 || k_views > kMaxViews) { wt::set_error("k_views must be in 1..%d", kMaxViews); return WT_ERR_INVALID; }
    if (!fuse_slots_shape_ok(n_frames, slots, k_views, n_categories, method)) {
        wt::set_error("bad slot shape: n_frames %lld, slots %lld, n_categories %d", (long long)n_frames, (long long)slots, n_categories);
        return WT_ERR_INVALID;
    }
    if (n_frames == 0 || slots == 0) return WT_OK;
    if (!xywhs || !category || !weights || !out_xywhs || !out_category || !out_counts || !workspace) {
        wt::set_error("null pointer argument"); return WT_ERR_INVALID;
    }
    const int64_t ks = (int64_t)k_views * slots;
    const bool lds = fuse_slots_use_lds(ks);
    const int64_t n_groups = n_frames * n_categories;
    size_t need = 0;
    const FuseSlotsWs ws = fuse_slots_ws_layout((char*)workspace, n_groups, (size_t)ks, lds, &need);
    if (workspace_bytes < need) {
        wt::set_error("slot fusion workspace too small: need %zu bytes, have %zu", need, workspace_bytes);
        return WT_ERR_CAPACITY;
    }
    const hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(n_groups < (1 << 20) ? n_groups : (1 << 20));
    if (lds)
        hipLaunchKernelGGL(fuse_slots_kernel<true>, dim3(grid), dim3(kWave), group_mem_bytes((size_t)ks), st, xywhs, category,
                           n_frames, (int)slots, k_views, weights, n_categories, method, iou_thresh, min_score, ws);
    else
        hipLaunchKernelGGL(fuse_slots_kernel<false>, dim3(grid), dim3(kWave), 0, st, xywhs, category, n_frames, (int)slots,
                           k_views, weights, n_categories, method, iou_thresh, min_score, ws);
    WT_HIP(hipGetLastError());
    const unsigned fgrid = (unsigned)(n_frames < (1 << 20) ? n_frames : (1 << 20));
    hipLaunchKernelGGL(fuse_slots_compact_kernel, dim3(fgrid), dim3(kWave), 0, st, n_frames, (int)slots, k_views, n_categories, ws,
                       out_xywhs, out_category, out_counts);
    WT_HIP(hipGetLastError());
    return WT_OK;
}

int64_t wt_fuse_groups_lds_rows(void) { return (int64_t)lds_capacity_rows(); }

size_t wt_fuse_groups_workspace(int64_t n_rows, int64_t n_groups, int64_t max_group_rows) {
    return workspace_bytes_for(n_rows, n_groups, max_group_rows);
}

int wt_fuse_groups_dev(const double* dets5, const int64_t* group_offsets, const double* group_wsum, int64_t n_rows,
                       int64_t n_groups, int64_t max_group_rows, int method, double iou_thresh, double* out5,
                       int32_t* out_members, int32_t* row_cluster, int64_t* out_counts, void* workspace, size_t workspace_bytes,
                       void* stream) {
    WT_TRY(wt::ensure_device());
    return launch_fuse(dets5, group_offsets, group_wsum, n_rows, n_groups, max_group_rows, method, iou_thresh, out5, out_members,
                       row_cluster, out_counts, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_fuse_groups_host(const double* dets5, const int64_t* group_offsets, const double* group_wsum, int64_t n_groups, int method,
                        double iou_thresh, double* out5, int32_t* out_members, int32_t* row_cluster, int64_t* out_counts) {
    WT_TRY(wt::ensure_device());
    if (method != 0 && method != 1) { wt::set_error("method must be 0 (weighted_fusion) or 1 (nmw), got %d", method); return WT_ERR_INVALID; }
    if (n_groups < 0) { wt::set_error("negative size: n_groups %lld", (long long)n_groups); return WT_ERR_INVALID; }
    if (n_groups == 0) return WT_OK;
    if (!dets5 || !group_offsets || !group_wsum || !out5 || !out_counts) { wt::set_error("null pointer argument"); return WT_ERR_INVALID; }
    if (group_offsets[0] != 0) { wt::set_error("group_offsets must start at 0"); return WT_ERR_INVALID; }
    const int64_t n_rows = group_offsets[n_groups];
    int64_t max_rows = 0;
    for (int64_t g = 0; g < n_groups; ++g) {
        const int64_t c = group_offsets[g + 1] - group_offsets[g];
        if (c < 0) { wt::set_error("group_offsets must be non-decreasing"); return WT_ERR_INVALID; }
        if (c > max_rows) max_rows = c;
    }
    wt::DevBuf d_in, d_off, d_ws_sum, d_out, d_mem, d_rc, d_cnt, d_ws;
    WT_TRY(d_in.alloc(sizeof(double) * 5 * (size_t)n_rows));
    WT_TRY(d_off.alloc(sizeof(int64_t) * (size_t)(n_groups + 1)));
    WT_TRY(d_ws_sum.alloc(sizeof(double) * (size_t)n_groups));
    WT_TRY(d_out.alloc(sizeof(double) * 5 * (size_t)n_rows));
    WT_TRY(d_mem.alloc(sizeof(int32_t) * (size_t)n_rows));
    WT_TRY(d_rc.alloc(sizeof(int32_t) * (size_t)n_rows));
    WT_TRY(d_cnt.alloc(sizeof(int64_t) * (size_t)n_groups));
    WT_HIP(hipMemcpy(d_in.p, dets5, sizeof(double) * 5 * (size_t)n_rows, hipMemcpyHostToDevice));
    WT_HIP(hipMemcpy(d_off.p, group_offsets, sizeof(int64_t) * (size_t)(n_groups + 1), hipMemcpyHostToDevice));
    WT_HIP(hipMemcpy(d_ws_sum.p, group_wsum, sizeof(double) * (size_t)n_groups, hipMemcpyHostToDevice));
    const size_t ws = workspace_bytes_for(n_rows, n_groups, max_rows);
    if (ws) WT_TRY(d_ws.alloc(ws));
    WT_TRY(launch_fuse(d_in.as<double>(), d_off.as<int64_t>(), d_ws_sum.as<double>(), n_rows, n_groups, max_rows, method,
                       iou_thresh, d_out.as<double>(), d_mem.as<int32_t>(), d_rc.as<int32_t>(), d_cnt.as<int64_t>(), d_ws.p, ws,
                       nullptr));
    WT_HIP(hipDeviceSynchronize());
    WT_HIP(hipMemcpy(out5, d_out.p, sizeof(double) * 5 * (size_t)n_rows, hipMemcpyDeviceToHost));
    WT_HIP(hipMemcpy(out_counts, d_cnt.p, sizeof(int64_t) * (size_t)n_groups, hipMemcpyDeviceToHost));
    if (out_members) WT_HIP(hipMemcpy(out_members, d_mem.p, sizeof(int32_t) * (size_t)n_rows, hipMemcpyDeviceToHost));
    if (row_cluster) WT_HIP(hipMemcpy(row_cluster, d_rc.p, sizeof(int32_t) * (size_t)n_rows, hipMemcpyDeviceToHost));
    return WT_OK;
}

}  // extern "C"
