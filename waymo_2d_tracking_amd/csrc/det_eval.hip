// Detection AP / AR on gfx950 (include/waymotrack.h, "Detection evaluation"; DESIGN.md section 16 has the definition).
//
// K results are scored against one ground truth in one call.  Five steps, all on the caller's stream:
//   prep    one thread per result row: does the row take part (category in range, conf > min_conf of its set), its sort key
//           (descending confidence as an ascending uint64) and its segment (set, class);
//   npos    one thread per ground-truth row: positives per class and size bucket;
//   match   one wavefront per problem (set, image, class): float64 IoU of every participating row against the class's
//           ground-truth rows in LDS tiles of 64, running first-argmax, then "the most confident row that claims a box" per
//           threshold with two atomics per claim on the box's slot (max of the confidence key, then min of the row index);
//   order   a stable sort of the rows by (set, class, confidence descending), equal confidences in input order (det_order.h);
//   curve   one workgroup per (set, class, threshold, size bucket): totals forward, then the tiles backwards with a prefix sum of
//           TP / FP, the reverse running maximum of the precision and the AP terms.
// No kernel waits for another workgroup, every loop bound is an input size, and there is no per-problem capacity.
// Compile with -ffp-contract=off: IoU, precision, recall and the AP terms are rounded operation by operation like numpy's.
#include "det_metric_device.h"
#include "det_metric_host.h"
#include "det_order.h"

using namespace wtdev;

namespace {

constexpr int kMaxClasses = 16;
constexpr int kMaxThr = 8;
constexpr int kBuckets = 4;                   // '', S, M, L
constexpr int kCurveThreads = 512;
constexpr int kCurveItems = 4;
constexpr int kCurveTile = kCurveThreads * kCurveItems;
constexpr int kCurveWaves = kCurveThreads / kWave;
constexpr double kSmall = 32.0 * 32.0, kLarge = 96.0 * 96.0;      // metric.SIZE_BUCKETS, pixels^2
constexpr double kEps = 2.220446049250313e-16;                   // np.finfo(np.float64).eps

struct Thresholds { double v[kMaxClasses * kMaxThr]; };

struct Workspace {
    wt::OrderBufs o;                          // keys = confidence keys, segments = (set, class)
    uint8_t *flag, *bucket;                   // [n_det * n_thr], [n_det]
    long long* match;                         // [n_det]
    unsigned int* hits;                       // [n_det] bit t: IoU of the row's box exceeds threshold t
    unsigned long long* best_key;             // [K * n_gt * n_thr] slot of a ground-truth box: best confidence key that claims it
    long long* best_row;                      // [K * n_gt * n_thr] and the first row with that key
    long long* npos;                          // [n_classes * 4]
    double* min_conf;                         // [K]
    size_t bytes;
};

int carve(void* base, size_t K, size_t C, size_t T, size_t n_gt, size_t n_det, Workspace* ws) {
    wt::Carver cv(base);
    Workspace& w = *ws;
    const size_t nd = n_det ? n_det : 1, slots = K * n_gt * T ? K * n_gt * T : 1;
    WT_TRY(wt::carve_order(cv, n_det, K, C, &w.o));
    w.flag = cv.take<uint8_t>(nd * T);
    w.bucket = cv.take<uint8_t>(nd);
    w.match = cv.take<long long>(nd);
    w.hits = cv.take<unsigned int>(nd);
    w.best_key = cv.take<unsigned long long>(slots);
    w.best_row = cv.take<long long>(slots);
    w.npos = cv.take<long long>(C * kBuckets);
    w.min_conf = cv.take<double>(K);
    w.bytes = cv.off;
    return WT_OK;
}

// ---- device helpers ----------------------------------------------------------------------------------------------------
// desc_key of a confidence: larger key = more confident; 0 marks "no claim" in a slot
// np.minimum / np.maximum: a NaN operand is the result
__device__ __forceinline__ double np_min(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a < b ? a : b)); }
__device__ __forceinline__ double np_max(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }
__device__ __forceinline__ int size_bucket(double px) { return px < kSmall ? 1 : ((px >= kSmall && px < kLarge) ? 2 : (px >= kLarge ? 3 : 0)); }

// ---- prep ----------------------------------------------------------------------------------------------------------------
__global__ void det_prep_kernel(long long n_det, int K, int C, int T, const int64_t* __restrict__ set_row_offsets,
                                const double* __restrict__ conf, const int32_t* __restrict__ category,
                                const double* __restrict__ min_conf, Workspace ws, uint8_t* __restrict__ flag, int64_t* __restrict__ match) {
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_det) return;
    const int lo = set_of_row(set_row_offsets, K, d);
    const int c = category[d];
    const double v = conf[d];
    const bool part = c >= 1 && c <= C && v > min_conf[lo];
    ws.o.key_in[d] = part ? ~desc_key(v) : ~0ull;
    ws.o.row_in[d] = d;
    ws.o.seg[d] = part ? (unsigned)(lo * C + (c - 1)) : (unsigned)(K * C);
    ws.hits[d] = 0u;
    match[d] = -1;
    for (int t = 0; t < T; ++t) flag[d * T + t] = 2;
}

// ---- positives per (class, bucket) -----------------------------------------------------------------------------------------
__global__ void det_npos_kernel(long long n_gt, long long n_images, int C, const double* __restrict__ x1, const double* __restrict__ y1,
                                const double* __restrict__ x2, const double* __restrict__ y2, const int32_t* __restrict__ label,
                                const int64_t* __restrict__ image_gt_offsets, const double* __restrict__ image_area, long long* __restrict__ npos) {
    __shared__ unsigned int cnt[kMaxClasses * kBuckets];
    for (int i = threadIdx.x; i < C * kBuckets; i += blockDim.x) cnt[i] = 0u;
    __syncthreads();
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_gt) {
        const int c = label[r];
        if (c >= 1 && c <= C) {
            const long long img = image_of_row(image_gt_offsets, n_images, r);
            const double g_size = (x2[r] - x1[r]) * (y2[r] - y1[r]);
            const int b = size_bucket(g_size * image_area[img]);
            atomicAdd(&cnt[(c - 1) * kBuckets], 1u);
            if (b) atomicAdd(&cnt[(c - 1) * kBuckets + b], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * kBuckets; i += blockDim.x)
        if (cnt[i]) atomicAdd((unsigned long long*)&npos[i], (unsigned long long)cnt[i]);
}

// ---- match -----------------------------------------------------------------------------------------------------------------
struct GtCols { const double *x1, *y1, *x2, *y2; };
struct DetCols { const double *conf, *cx, *cy, *w, *h; };

__global__ __launch_bounds__(kWave) void det_match_kernel(
    GtCols G, const int32_t* __restrict__ g_label, const int64_t* __restrict__ image_gt_offsets, const double* __restrict__ image_area,
    long long n_images, long long n_gt, int C, int T, const int64_t* __restrict__ set_row_offsets, const int64_t* __restrict__ image_det_offsets,
    DetCols D, const int32_t* __restrict__ d_cat, const double* __restrict__ min_conf, Thresholds thr_all, Workspace ws,
    uint8_t* __restrict__ flag, int64_t* __restrict__ match) {
    __shared__ double tx1[kWave], ty1[kWave], tx2[kWave], ty2[kWave], tsz[kWave];
    __shared__ long long trow[kWave];
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = lanemask_lt();
    const DetProblem prob(blockIdx.x, n_images, C);
    const int c = prob.c + 1;
    const long long img = prob.img, k = prob.k;
    long long d0, d1;
    prob.rows(set_row_offsets, image_det_offsets, n_images, &d0, &d1);
    if (d0 >= d1) return;
    const double minc = min_conf[k];
    bool any = false;
    for (long long base = d0; base < d1; base += kWave) {
        const long long d = base + lane;
        any = any || ((d < d1) && d_cat[d] == c && D.conf[d] > minc);
    }
    if (__ballot(any) == 0ull) return;
    const long long g0 = image_gt_offsets[img], g1 = image_gt_offsets[img + 1];
    const double img_area = image_area[img];
    const double* thr = thr_all.v + (c - 1) * kMaxThr;      // wave-uniform reads of the kernel argument
    unsigned long long* best_key = ws.best_key + (size_t)k * (size_t)n_gt * (size_t)T;
    long long* best_row = ws.best_row + (size_t)k * (size_t)n_gt * (size_t)T;

    // ---- 0. empty slots for the boxes of this class ----
    for (long long base = g0; base < g1; base += kWave) {
        const long long r = base + lane;
        if (r < g1 && g_label[r] == c)
            for (int t = 0; t < T; ++t) {
                slot_store(&best_key[r * T + t], 0ull);
                slot_store(&best_row[r * T + t], 0x7fffffffffffffffll);
            }
    }
    gsync();
    // ---- 1. IoU, first argmax, and the best confidence that claims each box ----
    // The class's boxes are re-read and re-compacted for every chunk of 64 rows: chunks x tiles global reads, which is one pass for
    // all but crowded images (a running argmax per row would otherwise have to be kept across tiles for every chunk at once).
    for (long long base = d0; base < d1; base += kWave) {
        const long long d = base + lane;
        const bool mine = (d < d1) && d_cat[d] == c && D.conf[d] > minc;
        if (__ballot(mine) == 0ull) continue;
        double cf = 0., area = 0., x1 = 0., y1 = 0., x2 = 0., y2 = 0.;
        if (mine) {
            cf = D.conf[d];
            const double cx = D.cx[d], cy = D.cy[d], w = D.w[d], h = D.h[d];
            area = w * h;
            x1 = cx - w / 2; y1 = cy - h / 2;
            x2 = cx + w / 2; y2 = cy + h / 2;
        }
        double best = 0.;
        long long jmax = -1;
        for (long long gb = g0; gb < g1; gb += kWave) {
            const long long r = gb + lane;
            const bool isg = (r < g1) && g_label[r] == c;
            const unsigned long long mm = __ballot(isg);
            if (mm == 0ull) continue;
            if (isg) {
                const int q = __popcll(mm & lt);
                const double a = G.x1[r], b = G.y1[r], cc = G.x2[r], dd = G.y2[r];
                tx1[q] = a; ty1[q] = b; tx2[q] = cc; ty2[q] = dd;
                tsz[q] = (cc - a) * (dd - b);
                trow[q] = r;
            }
            const int nt = __popcll(mm);
            wsync();
            if (mine) {
                for (int j = 0; j < nt; ++j) {
                    const double iw = np_max(np_min(tx2[j], x2) - np_max(tx1[j], x1), 0.);
                    const double ih = np_max(np_min(ty2[j], y2) - np_max(ty1[j], y1), 0.);
                    const double inter = iw * ih;
                    const double v = inter / ((area + tsz[j]) - inter);
                    // numpy argmax: the first NaN wins, otherwise the first maximum
                    if (jmax < 0 || (best == best && (v != v || v > best))) { best = v; jmax = trow[j]; }
                }
            }
            wsync();
        }
        if (mine) {
            const unsigned long long key = desc_key(cf);
            unsigned int hm = 0u;
            if (jmax >= 0)
                for (int t = 0; t < T; ++t)
                    if (best > thr[t]) {
                        hm |= 1u << t;
                        atomicMax(&best_key[jmax * T + t], key);
                    }
            ws.hits[d] = hm;
            match[d] = jmax;
            ws.bucket[d] = (uint8_t)size_bucket(area * img_area);
        }
    }
    gsync();
    // ---- 2. among the rows with that confidence, the first in input order ----
    for (long long base = d0; base < d1; base += kWave) {
        const long long d = base + lane;
        const bool mine = (d < d1) && d_cat[d] == c && D.conf[d] > minc;
        if (!mine) continue;
        const unsigned int hm = ws.hits[d];
        if (!hm) continue;
        const unsigned long long key = desc_key(D.conf[d]);
        const long long j = match[d];
        for (int t = 0; t < T; ++t)
            if (((hm >> t) & 1u) && slot_load(&best_key[j * T + t]) == key) atomicMin(&best_row[j * T + t], d);
    }
    gsync();
    // ---- 3. flags ----
    for (long long base = d0; base < d1; base += kWave) {
        const long long d = base + lane;
        const bool mine = (d < d1) && d_cat[d] == c && D.conf[d] > minc;
        if (!mine) continue;
        const unsigned int hm = ws.hits[d];
        const long long j = match[d];
        for (int t = 0; t < T; ++t) {
            const bool tp = ((hm >> t) & 1u) && slot_load(&best_row[j * T + t]) == d;
            flag[d * T + t] = tp ? 1 : 0;
        }
    }
}

// ---- curve -----------------------------------------------------------------------------------------------------------------
// maximum over the threads AFTER this one (0 when there is none; the values are >= 0); *total = the maximum over all.
__device__ __forceinline__ double block_excl_max_after(double v, double* total, double* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const double u = __shfl_down(inc, o, kWave);
        if (lane + o < kWave) inc = (u > inc) ? u : inc;
    }
    double after = __shfl_down(inc, 1, kWave);           // suffix maximum of the lanes after this one
    if (lane == kWave - 1) after = 0.;
    __syncthreads();
    if (lane == 0) lds[wave] = inc;
    __syncthreads();
    double all = 0.;
#pragma unroll
    for (int w = 0; w < kCurveWaves; ++w) {
        const double s = lds[w];
        if (w > wave) after = (s > after) ? s : after;
        all = (s > all) ? s : all;
    }
    *total = all;
    return after;
}

__global__ __launch_bounds__(kCurveThreads) void det_curve_kernel(
    int C, int T, const long long* __restrict__ order, const long long* __restrict__ class_offsets, const uint8_t* __restrict__ flag,
    const uint8_t* __restrict__ bucket, const long long* __restrict__ npos_cb, double* __restrict__ ap, double* __restrict__ ar,
    int64_t* __restrict__ npos_out, int64_t* __restrict__ tp_out, int64_t* __restrict__ fp_out, int64_t* __restrict__ ctp_out,
    int64_t* __restrict__ cfp_out) {
    __shared__ int lds_i[kCurveWaves + 1];
    __shared__ double lds_d[kCurveWaves + 1];
    __shared__ long long lds_l[2 * kCurveWaves];
    const size_t q = blockIdx.x;                         // ((k * C + c) * T + t) * 4 + b
    const int b = (int)(q % kBuckets);
    const int t = (int)((q / kBuckets) % (size_t)T);
    const int c = (int)((q / ((size_t)kBuckets * T)) % (size_t)C);
    const size_t k = q / ((size_t)kBuckets * T * C);
    const long long o0 = class_offsets[k * (C + 1) + c], o1 = class_offsets[k * (C + 1) + c + 1];
    const long long npos = npos_cb[c * kBuckets + b];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- totals ----
    long long n_tp = 0, n_fp = 0;
    for (long long i = o0 + tid; i < o1; i += kCurveThreads) {
        const long long row = order[i];
        if (b == 0 || bucket[row] == b) {
            const int f = flag[row * T + t];
            n_tp += f == 1;
            n_fp += f == 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { n_tp += __shfl_xor(n_tp, o, kWave); n_fp += __shfl_xor(n_fp, o, kWave); }
    if (lane == 0) { lds_l[wave] = n_tp; lds_l[kCurveWaves + wave] = n_fp; }
    __syncthreads();
    long long tot_tp = 0, tot_fp = 0;
#pragma unroll
    for (int w = 0; w < kCurveWaves; ++w) { tot_tp += lds_l[w]; tot_fp += lds_l[kCurveWaves + w]; }

    // ---- the tiles backwards: counts before a tile = counts up to its end - its own ----
    const double npos_d = (double)npos;
    const double den = npos_d > kEps ? npos_d : kEps;
    long long rem_tp = tot_tp, rem_fp = tot_fp;
    double carry_max = 0.;                               // mpre's closing 0
    double acc = 0.;
    const long long n = o1 - o0;
    const long long n_tiles = (n + kCurveTile - 1) / kCurveTile;
    for (long long tile = n_tiles - 1; tile >= 0; --tile) {
        const long long first = o0 + tile * kCurveTile + (long long)tid * kCurveItems;
        int tpv[kCurveItems], fpv[kCurveItems];
        int packed = 0;
#pragma unroll
        for (int u = 0; u < kCurveItems; ++u) {
            tpv[u] = 0; fpv[u] = 0;
            const long long i = first + u;
            if (i < o1) {
                const long long row = order[i];
                if (b == 0 || bucket[row] == b) {
                    const int f = flag[row * T + t];
                    tpv[u] = f == 1;
                    fpv[u] = f == 0;
                }
            }
            packed += (tpv[u] << 16) + fpv[u];
        }
        int tile_total;
        const int before = block_excl_sum<kCurveWaves>(packed, &tile_total, lds_i);
        const long long base_tp = rem_tp - (tile_total >> 16), base_fp = rem_fp - (tile_total & 0xffff);
        long long ctp = base_tp + (before >> 16), cfp = base_fp + (before & 0xffff);
        double prec[kCurveItems], step[kCurveItems];
        double my_max = 0.;
#pragma unroll
        for (int u = 0; u < kCurveItems; ++u) {
            ctp += tpv[u]; cfp += fpv[u];
            prec[u] = 0.; step[u] = 0.;
            if (tpv[u] | fpv[u]) {
                const double s = (double)(ctp + cfp);
                prec[u] = (double)ctp / (s > kEps ? s : kEps);
                const double rec = (double)ctp / den, rec_prev = (double)(ctp - tpv[u]) / den;
                step[u] = rec - rec_prev;                 // 0 where the recall does not move
                my_max = prec[u] > my_max ? prec[u] : my_max;
            }
            if (b == 0 && ctp_out && first + u < o1) {
                ctp_out[(first + u) * T + t] = ctp;
                cfp_out[(first + u) * T + t] = cfp;
            }
        }
        double tile_max;
        double m = block_excl_max_after(my_max, &tile_max, lds_d);
        m = carry_max > m ? carry_max : m;
#pragma unroll
        for (int u = kCurveItems - 1; u >= 0; --u) {
            m = prec[u] > m ? prec[u] : m;
            if (step[u] != 0.) acc = acc + step[u] * m;
        }
        carry_max = tile_max > carry_max ? tile_max : carry_max;
        rem_tp = base_tp; rem_fp = base_fp;
    }
    // ---- the AP sum ----
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, kWave);
    __syncthreads();
    if (lane == 0) lds_d[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.;
        for (int w = 0; w < kCurveWaves; ++w) sum = sum + lds_d[w];
        ap[q] = sum;
        ar[q] = (tot_tp + tot_fp) > 0 ? (double)tot_tp / den : __longlong_as_double(0x7ff8000000000000ll);
        npos_out[q] = npos;
        tp_out[q] = tot_tp;
        fp_out[q] = tot_fp;
    }
}

int check_sizes(int32_t k_sets, int64_t n_images, int32_t n_classes, int32_t n_thr, int64_t n_gt, int64_t n_det) {
    if (k_sets < 1 || n_images < 0 || n_gt < 0 || n_det < 0) { wt::set_error("wt_det_eval: bad argument"); return WT_ERR_INVALID; }
    if (n_classes < 1 || n_classes > kMaxClasses) { wt::set_error("wt_det_eval: n_classes must be 1..%d", kMaxClasses); return WT_ERR_INVALID; }
    if (n_thr < 1 || n_thr > kMaxThr) { wt::set_error("wt_det_eval: n_thr must be 1..%d", kMaxThr); return WT_ERR_INVALID; }
    if (n_det > 0x7fffffffll || n_gt > 0x7fffffffll) { wt::set_error("wt_det_eval: more than 2^31 - 1 rows in one call"); return WT_ERR_CAPACITY; }
    // one workgroup per problem / per curve: a launch takes fewer than 2^32 threads in all
    const unsigned long long problems = (unsigned long long)k_sets * (unsigned long long)n_images * (unsigned long long)n_classes;
    const unsigned long long curves = (unsigned long long)k_sets * n_classes * n_thr * kBuckets;
    if (problems * kWave > 0xffffffffull || curves * kCurveThreads > 0xffffffffull) {
        wt::set_error("wt_det_eval: %llu problems and %llu curves in one call: at most %llu and %llu", problems, curves,
                      0xffffffffull / kWave, 0xffffffffull / kCurveThreads);
        return WT_ERR_CAPACITY;
    }
    return WT_OK;
}

}  // namespace

extern "C" {

size_t wt_det_eval_workspace(int32_t k_sets, int64_t n_images, int32_t n_classes, int32_t n_thr, int64_t n_gt, int64_t n_det) {
    if (check_sizes(k_sets, n_images, n_classes, n_thr, n_gt, n_det) != WT_OK) return 0;
    Workspace ws;
    if (carve(nullptr, (size_t)k_sets, (size_t)n_classes, (size_t)n_thr, (size_t)n_gt, (size_t)n_det, &ws) != WT_OK) return 0;
    return ws.bytes + 256;
}

int wt_det_eval_dev(int64_t n_gt, const double* gx1, const double* gy1, const double* gx2, const double* gy2, const int32_t* g_label,
                    int64_t n_images, const int64_t* image_gt_offsets, const double* image_area,
                    int32_t k_sets, int64_t n_det, const int64_t* set_row_offsets, const int64_t* image_det_offsets,
                    const double* conf, const double* cx, const double* cy, const double* w, const double* h, const int32_t* category,
                    const double* min_conf, int32_t n_classes, int32_t n_thr, const double* thr,
                    double* ap, double* ar, int64_t* npos, int64_t* tp, int64_t* fp,
                    uint8_t* tp_flag, int64_t* match_gt, int64_t* order, int64_t* class_offsets, int64_t* ctp, int64_t* cfp,
                    int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream_) {
    WT_TRY(wt::ensure_device());
    hipStream_t stream = (hipStream_t)stream_;
    WT_TRY(check_sizes(k_sets, n_images, n_classes, n_thr, n_gt, n_det));
    if (!min_conf || !thr || !ap || !ar || !npos || !tp || !fp || !status_dev || (ctp == nullptr) != (cfp == nullptr)) {
        wt::set_error("wt_det_eval: bad argument");
        return WT_ERR_INVALID;
    }
    const int K = k_sets, C = n_classes, T = n_thr;
    Workspace ws;
    WT_TRY(carve(wt::align_ptr(workspace), (size_t)K, (size_t)C, (size_t)T, (size_t)n_gt, (size_t)n_det, &ws));
    if (!workspace || workspace_bytes < ws.bytes + 256) {
        wt::set_error("evaluation workspace too small: need %zu bytes, have %zu", ws.bytes + 256, workspace_bytes);
        return WT_ERR_CAPACITY;
    }
    uint8_t* flag = tp_flag ? tp_flag : ws.flag;
    int64_t* match = match_gt ? match_gt : (int64_t*)ws.match;
    long long* ord = order ? (long long*)order : ws.o.order;
    Thresholds th;
    for (int c = 0; c < kMaxClasses; ++c)
        for (int t = 0; t < kMaxThr; ++t) th.v[c * kMaxThr + t] = (c < C && t < T) ? thr[c * T + t] : 2.0;
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    // K values from pageable host memory: the runtime stages them before it returns; this one copy keeps the call out of a graph capture
    WT_HIP(hipMemcpyAsync(ws.min_conf, min_conf, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, stream));
    WT_HIP(hipMemsetAsync(ws.npos, 0, sizeof(long long) * (size_t)C * kBuckets, stream));
    if (ctp && n_det > 0) {                              // positions after the last participating row stay 0
        WT_HIP(hipMemsetAsync(ctp, 0, sizeof(int64_t) * (size_t)n_det * T, stream));
        WT_HIP(hipMemsetAsync(cfp, 0, sizeof(int64_t) * (size_t)n_det * T, stream));
    }
    if (n_det > 0)
        hipLaunchKernelGGL(det_prep_kernel, dim3((unsigned)((n_det + 255) / 256)), dim3(256), 0, stream, (long long)n_det, K, C, T, set_row_offsets,
                           conf, category, ws.min_conf, ws, flag, match);
    if (n_gt > 0)
        hipLaunchKernelGGL(det_npos_kernel, dim3((unsigned)((n_gt + 255) / 256)), dim3(256), 0, stream, (long long)n_gt, (long long)n_images, C,
                           gx1, gy1, gx2, gy2, g_label, image_gt_offsets, image_area, ws.npos);
    const size_t n_problems = (size_t)K * (size_t)n_images * (size_t)C;
    if (n_det > 0 && n_problems > 0) {
        const GtCols G = {gx1, gy1, gx2, gy2};
        const DetCols D = {conf, cx, cy, w, h};
        hipLaunchKernelGGL(det_match_kernel, dim3((unsigned)n_problems), dim3(kWave), 0, stream, G, g_label, image_gt_offsets, image_area,
                           (long long)n_images, (long long)n_gt, C, T, set_row_offsets, image_det_offsets, D, category, ws.min_conf, th, ws, flag, match);
    }
    WT_TRY(wt::enqueue_order(ws.o, n_det, K, C, ord, class_offsets, stream));
    hipLaunchKernelGGL(det_curve_kernel, dim3((unsigned)((size_t)K * C * T * kBuckets)), dim3(kCurveThreads), 0, stream, C, T, ord, ws.o.class_offsets, flag,
                       ws.bucket, ws.npos, ap, ar, npos, tp, fp, ctp, cfp);
    WT_HIP(hipGetLastError());
    return WT_OK;
}

int wt_det_eval_host(int64_t n_gt, const double* gx1, const double* gy1, const double* gx2, const double* gy2, const int32_t* g_label,
                     int64_t n_images, const int64_t* image_gt_offsets, const double* image_area,
                     int32_t k_sets, const int64_t* set_row_offsets, const int64_t* image_det_offsets,
                     const double* conf, const double* cx, const double* cy, const double* w, const double* h, const int32_t* category,
                     const double* min_conf, int32_t n_classes, int32_t n_thr, const double* thr,
                     double* ap, double* ar, int64_t* npos, int64_t* tp, int64_t* fp,
                     uint8_t* tp_flag, int64_t* match_gt, int64_t* order, int64_t* class_offsets, int64_t* ctp, int64_t* cfp) {
    if (k_sets < 1 || !set_row_offsets || !image_det_offsets || !image_gt_offsets || !min_conf || !thr || !ap || !ar || !npos || !tp || !fp) {
        wt::set_error("wt_det_eval_host: bad argument");
        return WT_ERR_INVALID;
    }
    const int64_t n_det = set_row_offsets[k_sets];
    WT_TRY(check_sizes(k_sets, n_images, n_classes, n_thr, n_gt, n_det));
    if ((ctp == nullptr) != (cfp == nullptr)) { wt::set_error("wt_det_eval_host: ctp and cfp come together"); return WT_ERR_INVALID; }
    // ---- the layout must be what the kernels walk: checked here, the device form trusts its caller ----
    const wt::DetLayout layout = {n_gt, n_images, k_sets, image_gt_offsets, set_row_offsets, image_det_offsets};
    WT_TRY(wt::check_det_layout(layout, "wt_det_eval_host"));
    WT_TRY(wt::check_det_eval_rows(layout, g_label, category, n_classes));
    WT_TRY(wt::ensure_device());
    const size_t ng = (size_t)n_gt, nd = (size_t)n_det, K = (size_t)k_sets, C = (size_t)n_classes, T = (size_t)n_thr, ni = (size_t)n_images;
    const size_t n_out = K * C * T * kBuckets;
    wt::DevBuf dg[4], dgl, dio, dia, dsr, dido, dd[5], dcat, dap, dar, dnp, dtp, dfp, dflag, dmatch, dorder, dco, dctp, dcfp, dstat, dws;
    const double* gsrc[4] = {gx1, gy1, gx2, gy2};
    const double* dsrc[5] = {conf, cx, cy, w, h};
    for (int i = 0; i < 4; ++i) WT_TRY(dg[i].upload(gsrc[i], 8 * ng));
    for (int i = 0; i < 5; ++i) WT_TRY(dd[i].upload(dsrc[i], 8 * nd));
    WT_TRY(dgl.upload(g_label, 4 * ng));
    WT_TRY(dcat.upload(category, 4 * nd));
    WT_TRY(dio.upload(image_gt_offsets, 8 * (ni + 1)));
    WT_TRY(dia.upload(image_area, 8 * ni));
    WT_TRY(dsr.upload(set_row_offsets, 8 * (K + 1)));
    WT_TRY(dido.upload(image_det_offsets, 8 * K * (ni + 1)));
    WT_TRY(dap.alloc(8 * n_out)); WT_TRY(dar.alloc(8 * n_out)); WT_TRY(dnp.alloc(8 * n_out)); WT_TRY(dtp.alloc(8 * n_out)); WT_TRY(dfp.alloc(8 * n_out));
    WT_TRY(dstat.alloc(16));
    if (tp_flag) WT_TRY(dflag.alloc(nd * T));
    if (match_gt) WT_TRY(dmatch.alloc(8 * nd));
    if (order) WT_TRY(dorder.alloc(8 * nd));
    if (class_offsets) WT_TRY(dco.alloc(8 * K * (C + 1)));
    if (ctp) { WT_TRY(dctp.alloc(8 * nd * T)); WT_TRY(dcfp.alloc(8 * nd * T)); }
    const size_t wsb = wt_det_eval_workspace(k_sets, n_images, n_classes, n_thr, n_gt, n_det);
    if (!wsb) return WT_ERR_CAPACITY;
    WT_TRY(dws.alloc(wsb));
    WT_TRY(wt_det_eval_dev(n_gt, dg[0].as<double>(), dg[1].as<double>(), dg[2].as<double>(), dg[3].as<double>(), dgl.as<int32_t>(), n_images,
                           dio.as<int64_t>(), dia.as<double>(), k_sets, n_det, dsr.as<int64_t>(), dido.as<int64_t>(), dd[0].as<double>(),
                           dd[1].as<double>(), dd[2].as<double>(), dd[3].as<double>(), dd[4].as<double>(), dcat.as<int32_t>(), min_conf, n_classes,
                           n_thr, thr, dap.as<double>(), dar.as<double>(), dnp.as<int64_t>(), dtp.as<int64_t>(), dfp.as<int64_t>(),
                           tp_flag ? dflag.as<uint8_t>() : nullptr, match_gt ? dmatch.as<int64_t>() : nullptr, order ? dorder.as<int64_t>() : nullptr,
                           class_offsets ? dco.as<int64_t>() : nullptr, ctp ? dctp.as<int64_t>() : nullptr, ctp ? dcfp.as<int64_t>() : nullptr,
                           dstat.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(wt::finish_det_call(dstat, "evaluation", " (4 = capacity)"));
    WT_TRY(dap.download(ap)); WT_TRY(dar.download(ar)); WT_TRY(dnp.download(npos)); WT_TRY(dtp.download(tp)); WT_TRY(dfp.download(fp));
    if (class_offsets) WT_TRY(dco.download(class_offsets));
    if (tp_flag) WT_TRY(dflag.download(tp_flag));
    if (match_gt) WT_TRY(dmatch.download(match_gt));
    if (order) WT_TRY(dorder.download(order));
    if (ctp) { WT_TRY(dctp.download(ctp)); WT_TRY(dcfp.download(cfp)); }
    return WT_OK;
}

}  // extern "C"
