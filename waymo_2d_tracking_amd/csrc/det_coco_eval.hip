// COCO detection metric (AP@[.5:.95], AP50, AP75, by area, AR@1/10/100) on gfx950 (include/waymotrack.h, "COCO detection
// evaluation"; DESIGN.md section 28 has the definition).
//
// K results are scored against one ground truth in one call.  All steps run on the caller's stream:
//   prep    one thread per result row: sort key (descending score as an ascending uint64), segment (set, category), rank = -1;
//   npig    one thread per (ground-truth row, set): not-ignored boxes per (set, category, area range) on the participating images;
//   match   one wavefront per problem (set, image, category).  select: every row of the category counts the rows that go before
//           it by (score key, input index); the first max_dets[last] of them form the list D in LDS.  match: for each d of D in
//           order the lanes compute the float64 IoU against 64 ground-truth rows at a time into LDS, then lane a * T + t walks the
//           tile for ITS (area range, threshold) chain: best free not-ignored box (ties to the last), else best ignored one.  The
//           "taken" sets are one 64-bit word per ground-truth row (bit = chain) in LDS, in the workspace for images with more
//           than kTakenLds rows;
//   order   a stable sort of the rows by (set, category, score descending), equal scores in input order (det_order.h);
//   gather  rank and the matched / ignored bit words of every row, in sorted order;
//   curve   one workgroup per (set, category, area range, max_dets, threshold): prefix sums of TP / FP, precision and recall per
//           TP row, the best precision per recall bucket with LDS atomics, a suffix maximum over the buckets = the 101 samples.
// No kernel waits for another workgroup, every loop bound is an input size, and there is no per-problem capacity.
// Compile with -ffp-contract=off: IoU, precision and recall are rounded operation by operation like numpy's.
#include "det_metric_device.h"
#include "det_metric_host.h"
#include "det_order.h"

using namespace wtdev;

namespace {

constexpr int kMaxThr = 16;
constexpr int kMaxRec = 128;
constexpr int kMaxArea = 4;
constexpr int kMaxMd = 4;
constexpr int kCap = 128;                      // largest max_dets value: ranks fit the LDS list and a uint8
constexpr int kTakenLds = 256;                 // ground-truth rows of one image whose taken words live in LDS
constexpr int kNpigLds = 1024;                 // (category, area range) counters a block of the npig kernel keeps in LDS
constexpr int kCurveThreads = 256;
constexpr int kCurveItems = 4;
constexpr int kCurveTile = kCurveThreads * kCurveItems;
constexpr int kCurveWaves = kCurveThreads / kWave;
constexpr double kEps = 2.220446049250313e-16;                   // 2^-52
constexpr double kBoundCap = 1.0 - 1e-10;

struct Params {
    double thr[kMaxThr];
    double rec[kMaxRec];
    double area[kMaxArea * 2];
    int32_t max_dets[kMaxMd];
};

struct Workspace {
    wt::OrderBufs o;                          // keys = score keys, segments = (set, category)
    int32_t* rank;                            // [n_det] rank in the problem, -1 = takes no part
    unsigned long long *mbits, *ibits;        // [n_det] bit a * T + t: matched / ignored
    uint8_t* srank;                           // [n_det] rank by sorted position, 255 = takes no part
    unsigned long long *smbits, *sibits;      // [n_det] the bit words by sorted position
    unsigned long long* taken;                // [K * n_gt] taken words of the images with more than kTakenLds rows
    long long* npig;                          // [K * C * A]
    size_t bytes;
};

int carve(void* base, size_t K, size_t C, size_t A, size_t n_gt, size_t n_det, Workspace* ws) {
    wt::Carver cv(base);
    Workspace& w = *ws;
    const size_t nd = n_det ? n_det : 1, slots = K * n_gt ? K * n_gt : 1;
    WT_TRY(wt::carve_order(cv, n_det, K, C, &w.o));
    w.rank = cv.take<int32_t>(nd);
    w.mbits = cv.take<unsigned long long>(nd);
    w.ibits = cv.take<unsigned long long>(nd);
    w.srank = cv.take<uint8_t>(nd);
    w.smbits = cv.take<unsigned long long>(nd);
    w.sibits = cv.take<unsigned long long>(nd);
    w.taken = cv.take<unsigned long long>(slots);
    w.npig = cv.take<long long>(K * C * A);
    w.bytes = cv.off;
    return WT_OK;
}

// desc_key of a score: larger key = higher score; 0 marks "not a row of this category" in a tile

// ---- prep ----------------------------------------------------------------------------------------------------------------
__global__ void coco_prep_kernel(long long n_det, int K, int C, int AT, const int64_t* __restrict__ set_row_offsets, const double* __restrict__ score,
                                 const int32_t* __restrict__ category, Workspace ws, int32_t* __restrict__ rank, int64_t* __restrict__ match_out,
                                 uint8_t* __restrict__ ign_out) {
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_det) return;
    const int lo = set_of_row(set_row_offsets, K, d);
    const int c = category[d];
    const bool part = c >= 0 && c < C;
    ws.o.key_in[d] = ~desc_key(score[d]);
    ws.o.row_in[d] = d;
    ws.o.seg[d] = part ? (unsigned)(lo * C + c) : (unsigned)(K * C);
    rank[d] = -1;
    if (match_out)
        for (int q = 0; q < AT; ++q) { match_out[(size_t)d * AT + q] = -1; ign_out[(size_t)d * AT + q] = 0; }
}

// ---- not-ignored ground truth per (set, category, area range) -------------------------------------------------------------
__global__ void coco_npig_kernel(long long n_gt, long long n_images, int C, int A, Params P, const double* __restrict__ g_area,
                                 const int32_t* __restrict__ g_cat, const uint8_t* __restrict__ g_crowd, const int64_t* __restrict__ image_gt_offsets,
                                 const uint8_t* __restrict__ image_mask, long long* __restrict__ npig) {
    // the rows of a block meet in LDS counters first (a handful of addresses for the whole data set); more than kNpigLds counters go straight to memory
    __shared__ unsigned int cnt[kNpigLds];
    const int CA = C * A;
    const bool in_lds = CA <= kNpigLds;
    if (in_lds) {
        for (int i = threadIdx.x; i < CA; i += blockDim.x) cnt[i] = 0u;
        __syncthreads();
    }
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long k = blockIdx.y;
    const int c = r < n_gt ? g_cat[r] : -1;
    bool counts = c >= 0 && c < C && !g_crowd[r];
    if (counts && image_mask) counts = image_mask[k * n_images + image_of_row(image_gt_offsets, n_images, r)] != 0;
    if (counts) {
        const double area = g_area[r];
        for (int a = 0; a < A; ++a)
            if (!(area < P.area[2 * a] || area > P.area[2 * a + 1])) {
                if (in_lds) atomicAdd(&cnt[c * A + a], 1u);
                else atomicAdd((unsigned long long*)&npig[(k * C + c) * A + a], 1ull);
            }
    }
    if (in_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < CA; i += blockDim.x)
            if (cnt[i]) atomicAdd((unsigned long long*)&npig[k * CA + i], (unsigned long long)cnt[i]);
    }
}

// without a mask every set has the counts of set 0
__global__ void coco_npig_fill_kernel(long long n, long long per_set, long long* __restrict__ npig) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per_set && i < n) npig[i] = npig[i % per_set];
}

// ---- select + match --------------------------------------------------------------------------------------------------------
struct GtCols { const double *x, *y, *w, *h, *area; const int32_t* cat; const uint8_t* crowd; };
struct DetCols { const double *score, *x, *y, *w, *h; const int32_t* cat; };

__global__ __launch_bounds__(kWave) void coco_match_kernel(
    GtCols G, const int64_t* __restrict__ image_gt_offsets, long long n_images, long long n_gt, int C, int T, int A, int cap, Params P,
    const int64_t* __restrict__ set_row_offsets, const int64_t* __restrict__ image_det_offsets, DetCols D, const uint8_t* __restrict__ image_mask,
    Workspace ws, int32_t* __restrict__ rank, int64_t* __restrict__ match_out, uint8_t* __restrict__ ign_out) {
    __shared__ unsigned long long tkey[kWave];
    __shared__ double tiou[kWave];
    __shared__ uint8_t tflag[kWave];
    __shared__ int sel[kCap];
    __shared__ unsigned long long taken_lds[kTakenLds];
    const int lane = threadIdx.x & 63;
    const DetProblem prob(blockIdx.x, n_images, C);
    const int c = prob.c;
    const long long img = prob.img, k = prob.k;
    if (image_mask && !image_mask[k * n_images + img]) return;
    long long d0, d1;
    prob.rows(set_row_offsets, image_det_offsets, n_images, &d0, &d1);
    if (d0 >= d1) return;

    // ---- select: rank of every row of the category among them by (score key descending, input index) ----
    int n_c = 0;
    for (long long base = d0; base < d1; base += kWave) {
        const long long d = base + lane;
        const bool mine = (d < d1) && D.cat[d] == c;
        const unsigned long long mm = __ballot(mine);
        if (mm == 0ull) continue;
        n_c += __popcll(mm);
        const unsigned long long key = mine ? desc_key(D.score[d]) : 0ull;
        int before = 0;
        for (long long tb = d0; tb < d1; tb += kWave) {
            const long long e = tb + lane;
            wsync();                                     // the previous tile has been read
            tkey[lane] = ((e < d1) && D.cat[e] == c) ? desc_key(D.score[e]) : 0ull;
            wsync();
            if (mine) {
                const int nt = (int)((d1 - tb) < kWave ? (d1 - tb) : kWave);
                for (int j = 0; j < nt; ++j) {
                    const unsigned long long o = tkey[j];
                    before += (o > key) || (o == key && (tb + j) < d);
                }
            }
        }
        if (mine) {
            if (before < cap) { sel[before] = (int)(d - d0); rank[d] = before; }
        }
    }
    if (n_c == 0) return;
    const int n_sel = n_c < cap ? n_c : cap;

    // ---- the taken words of the image's ground-truth rows ----
    const long long g0 = image_gt_offsets[img], g1 = image_gt_offsets[img + 1];
    const bool in_lds = (g1 - g0) <= kTakenLds;
    unsigned long long* taken_g = ws.taken + (size_t)k * (size_t)n_gt + (size_t)g0;
    for (long long i = lane; i < g1 - g0; i += kWave) {
        if (in_lds) taken_lds[i] = 0ull;
        else if (G.cat[g0 + i] == c) slot_store(&taken_g[i], 0ull);      // the other rows belong to the waves of their categories
    }
    if (in_lds) wsync(); else gsync();

    // ---- chain of this lane ----
    const int AT = A * T;
    const bool act = lane < AT;
    const int ca = act ? lane / T : 0, ct = act ? lane % T : 0;
    const double thr = P.thr[ct];
    const double bound = thr < kBoundCap ? thr : kBoundCap;
    const double a_lo = P.area[2 * ca], a_hi = P.area[2 * ca + 1];
    const unsigned long long my_bit = 1ull << lane;

    // one tile of ground truth (the usual case): its boxes stay in registers over all d
    const bool single = (g1 - g0) <= kWave;
    double gx = 0., gy = 0., gw = 0., gh = 0.;
    bool isg = false;
    uint8_t gflag = 0;
    auto load_gt = [&](long long r) {
        isg = (r < g1) && G.cat[r] == c;
        gflag = 0;
        if (isg) {
            gx = G.x[r]; gy = G.y[r]; gw = G.w[r]; gh = G.h[r];
            const double ar = G.area[r];
            const bool crowd = G.crowd[r] != 0;
            for (int a = 0; a < A; ++a)
                if (crowd || ar < P.area[2 * a] || ar > P.area[2 * a + 1]) gflag |= (uint8_t)(1u << a);
            if (crowd) gflag |= 0x80u;
        }
    };
    if (single) load_gt(g0 + lane);

    for (int ri = 0; ri < n_sel; ++ri) {
        const long long d = d0 + sel[ri];
        const double dx = D.x[d], dy = D.y[d], dw = D.w[d], dh = D.h[d];
        const double darea = dw * dh;
        double best_n = bound, best_i = bound;
        long long m_n = -1, m_i = -1;
        for (long long gb = g0; gb < g1; gb += kWave) {
            if (!single) load_gt(gb + lane);
            unsigned long long mm = __ballot(isg);
            if (mm == 0ull) continue;
            wsync();                                     // the previous tile has been read
            if (isg) {
                const double xa = (dx + dw) < (gx + gw) ? (dx + dw) : (gx + gw);
                const double xb = dx > gx ? dx : gx;
                const double ya = (dy + dh) < (gy + gh) ? (dy + dh) : (gy + gh);
                const double yb = dy > gy ? dy : gy;
                double iw = xa - xb, ih = ya - yb;
                if (iw <= 0.) iw = 0.;
                if (ih <= 0.) ih = 0.;
                const double inter = iw * ih;
                const double uni_ = (gflag & 0x80u) ? darea : ((darea + gw * gh) - inter);
                tiou[lane] = (inter == 0.) ? 0. : inter / uni_;
                tflag[lane] = gflag;
            }
            wsync();
            while (mm) {                                 // wave-uniform walk in annotation order
                const int j = __builtin_ctzll(mm);
                mm &= mm - 1ull;
                const long long r = gb + j;
                const unsigned long long tk = in_lds ? taken_lds[r - g0] : slot_load(&taken_g[r - g0]);
                const double v = tiou[j];
                const unsigned f = tflag[j];
                if (act && !((tk & my_bit) && !(f & 0x80u)) && !(v < bound)) {
                    if ((f >> ca) & 1u) {
                        if (v >= best_i) { best_i = v; m_i = r; }
                    } else {
                        if (v >= best_n) { best_n = v; m_n = r; }
                    }
                }
            }
        }
        const long long m = m_n >= 0 ? m_n : m_i;
        const bool matched = act && m >= 0;
        const bool d_ign = act && (m >= 0 ? m_n < 0 : (darea < a_lo || darea > a_hi));
        if (matched) {
            if (in_lds) atomicOr(&taken_lds[m - g0], my_bit); else atomicOr(&taken_g[m - g0], my_bit);
        }
        const unsigned long long mb = __ballot(matched), ib = __ballot(d_ign);
        if (lane == 0) { ws.mbits[d] = mb; ws.ibits[d] = ib; }
        if (match_out && act) {
            match_out[(size_t)d * AT + lane] = m;
            ign_out[(size_t)d * AT + lane] = d_ign ? 1 : 0;
        }
        if (in_lds) wsync(); else gsync();
    }
}

// ---- rank and bit words in sorted order ------------------------------------------------------------------------------------
__global__ void coco_gather_rows_kernel(long long n, const long long* __restrict__ order, const int32_t* __restrict__ rank, Workspace ws) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long row = order[i];
    const int r = rank[row];
    ws.srank[i] = r < 0 ? (uint8_t)255 : (uint8_t)r;
    ws.smbits[i] = r < 0 ? 0ull : ws.mbits[row];
    ws.sibits[i] = r < 0 ? 0ull : ws.ibits[row];
}

// ---- curve -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCurveThreads) void coco_curve_kernel(int C, int T, int A, int M, int R, Params P, Workspace ws,
                                                                   double* __restrict__ precision, double* __restrict__ recall) {
    __shared__ int lds_i[kCurveWaves];
    __shared__ unsigned long long bucket[kMaxRec];
    __shared__ double rec[kMaxRec];
    const size_t q = blockIdx.x;                         // (((k * C + c) * A + a) * M + m) * T + t
    const int t = (int)(q % (size_t)T);
    const int m = (int)((q / (size_t)T) % (size_t)M);
    const int a = (int)((q / ((size_t)T * M)) % (size_t)A);
    const int c = (int)((q / ((size_t)T * M * A)) % (size_t)C);
    const size_t k = q / ((size_t)T * M * A * C);
    const int tid = threadIdx.x;
    const long long npig = ws.npig[(k * C + c) * A + a];
    const size_t rec_idx = (((k * T + t) * C + c) * A + a) * M + m;
    auto prec_idx = [&](int ri) { return ((((k * T + t) * (size_t)R + ri) * C + c) * A + a) * M + m; };
    if (npig == 0) {                                     // wave-uniform: no not-ignored ground truth
        for (int ri = tid; ri < R; ri += kCurveThreads) precision[prec_idx(ri)] = -1.;
        if (tid == 0) recall[rec_idx] = -1.;
        return;
    }
    for (int ri = tid; ri < kMaxRec; ri += kCurveThreads) { bucket[ri] = 0ull; rec[ri] = ri < R ? P.rec[ri] : 0.; }
    __syncthreads();
    const long long o0 = ws.o.class_offsets[k * (C + 1) + c], o1 = ws.o.class_offsets[k * (C + 1) + c + 1];
    const int md = P.max_dets[m];
    const int chain = a * T + t;
    const double npig_d = (double)npig;
    long long run_tp = 0, run_fp = 0;
    const long long n = o1 - o0;
    const long long n_tiles = (n + kCurveTile - 1) / kCurveTile;
    for (long long tile = 0; tile < n_tiles; ++tile) {
        const long long first = o0 + tile * kCurveTile + (long long)tid * kCurveItems;
        int tpv[kCurveItems], fpv[kCurveItems];
        int packed = 0;
#pragma unroll
        for (int u = 0; u < kCurveItems; ++u) {
            tpv[u] = 0; fpv[u] = 0;
            const long long i = first + u;
            if (i < o1 && (int)ws.srank[i] < md) {
                const int mt = (int)((ws.smbits[i] >> chain) & 1ull), ig = (int)((ws.sibits[i] >> chain) & 1ull);
                tpv[u] = mt & (ig ^ 1);
                fpv[u] = (mt ^ 1) & (ig ^ 1);
            }
            packed += (tpv[u] << 16) + fpv[u];
        }
        int tile_total;
        const int before = block_excl_sum<kCurveWaves>(packed, &tile_total, lds_i);
        long long ctp = run_tp + (before >> 16), cfp = run_fp + (before & 0xffff);
#pragma unroll
        for (int u = 0; u < kCurveItems; ++u) {
            ctp += tpv[u]; cfp += fpv[u];
            if (tpv[u]) {                                // the rows after a TP up to the next one have its recall and no better precision
                const double pr = (double)ctp / (((double)cfp + (double)ctp) + kEps);
                const double rc = (double)ctp / npig_d;
                int lo = 0, hi = R;                      // number of recall thresholds <= rc
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (rec[mid] <= rc) lo = mid + 1; else hi = mid;
                }
                if (lo > 0) atomicMax(&bucket[lo - 1], (unsigned long long)__double_as_longlong(pr));     // pr >= 0: its bits order like its value
            }
        }
        run_tp += tile_total >> 16; run_fp += tile_total & 0xffff;
    }
    __syncthreads();
    for (int ri = tid; ri < R; ri += kCurveThreads) {
        unsigned long long best = 0ull;
        for (int j = ri; j < R; ++j) best = bucket[j] > best ? bucket[j] : best;
        precision[prec_idx(ri)] = __longlong_as_double((long long)best);
    }
    if (tid == 0) recall[rec_idx] = (double)run_tp / npig_d;
}

int check_sizes(int32_t k_sets, int64_t n_images, int32_t n_cats, int32_t n_thr, int32_t n_rec, int32_t n_area, int32_t n_maxdet, int64_t n_gt, int64_t n_det) {
    if (k_sets < 1 || n_images < 0 || n_gt < 0 || n_det < 0 || n_cats < 1) { wt::set_error("wt_det_coco: bad argument"); return WT_ERR_INVALID; }
    if (n_thr < 1 || n_area < 1 || n_thr > kMaxThr || n_area > kMaxArea || n_thr * n_area > kWave) {
        wt::set_error("wt_det_coco: n_thr must be 1..%d and n_area 1..%d", kMaxThr, kMaxArea);
        return WT_ERR_INVALID;
    }
    if (n_rec < 1 || n_rec > kMaxRec) { wt::set_error("wt_det_coco: n_rec must be 1..%d", kMaxRec); return WT_ERR_INVALID; }
    if (n_maxdet < 1 || n_maxdet > kMaxMd) { wt::set_error("wt_det_coco: n_maxdet must be 1..%d", kMaxMd); return WT_ERR_INVALID; }
    if (n_det > 0x7fffffffll || n_gt > 0x7fffffffll) { wt::set_error("wt_det_coco: more than 2^31 - 1 rows in one call"); return WT_ERR_CAPACITY; }
    // one workgroup per problem / per curve: a launch takes fewer than 2^32 threads in all
    const unsigned long long problems = (unsigned long long)k_sets * (unsigned long long)n_images * (unsigned long long)n_cats;
    const unsigned long long curves = (unsigned long long)k_sets * n_cats * n_thr * n_area * n_maxdet;
    if (problems * kWave > 0xffffffffull || curves * kCurveThreads > 0xffffffffull || k_sets > 65535) {
        wt::set_error("wt_det_coco: %llu problems and %llu curves in one call: at most %llu and %llu, and 65535 results", problems, curves,
                      0xffffffffull / kWave, 0xffffffffull / kCurveThreads);
        return WT_ERR_CAPACITY;
    }
    return WT_OK;
}

// thr, rec, area_rng, max_dets are host arrays: checked and packed into the kernel argument
int pack_params(int32_t n_thr, const double* thr, int32_t n_rec, const double* rec, int32_t n_area, const double* area_rng, int32_t n_maxdet,
                const int32_t* max_dets, Params* P) {
    if (!thr || !rec || !area_rng || !max_dets) { wt::set_error("wt_det_coco: bad argument"); return WT_ERR_INVALID; }
    for (int i = 0; i < kMaxThr; ++i) P->thr[i] = i < n_thr ? thr[i] : 2.0;
    for (int i = 0; i < kMaxRec; ++i) P->rec[i] = i < n_rec ? rec[i] : 0.0;
    for (int i = 0; i < kMaxArea * 2; ++i) P->area[i] = i < 2 * n_area ? area_rng[i] : 0.0;
    for (int i = 0; i < kMaxMd; ++i) P->max_dets[i] = i < n_maxdet ? max_dets[i] : 0;
    for (int i = 0; i < n_thr; ++i)
        if (!(thr[i] == thr[i])) { wt::set_error("wt_det_coco: IoU threshold %d is not a number", i); return WT_ERR_INVALID; }
    for (int i = 0; i < n_rec; ++i)
        if (!(rec[i] == rec[i]) || (i > 0 && !(rec[i] > rec[i - 1]))) { wt::set_error("wt_det_coco: recall thresholds must ascend (entry %d)", i); return WT_ERR_INVALID; }
    for (int i = 0; i < n_maxdet; ++i) {
        if (max_dets[i] < 1 || (i > 0 && max_dets[i] <= max_dets[i - 1])) { wt::set_error("wt_det_coco: max_dets must be positive and ascend (entry %d)", i); return WT_ERR_INVALID; }
        if (max_dets[i] > kCap) { wt::set_error("wt_det_coco: max_dets %d above %d", (int)max_dets[i], kCap); return WT_ERR_CAPACITY; }
    }
    return WT_OK;
}

}  // namespace

extern "C" {

size_t wt_det_coco_workspace(int32_t k_sets, int64_t n_images, int32_t n_cats, int32_t n_thr, int32_t n_rec, int32_t n_area, int32_t n_maxdet,
                             int64_t n_gt, int64_t n_det) {
    if (check_sizes(k_sets, n_images, n_cats, n_thr, n_rec, n_area, n_maxdet, n_gt, n_det) != WT_OK) return 0;
    Workspace ws;
    if (carve(nullptr, (size_t)k_sets, (size_t)n_cats, (size_t)n_area, (size_t)n_gt, (size_t)n_det, &ws) != WT_OK) return 0;
    return ws.bytes + 256;
}

int wt_det_coco_dev(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh, const double* g_area,
                    const int32_t* g_cat, const uint8_t* g_crowd, int64_t n_images, const int64_t* image_gt_offsets,
                    int32_t k_sets, int64_t n_det, const int64_t* set_row_offsets, const int64_t* image_det_offsets,
                    const double* score, const double* x, const double* y, const double* w, const double* h, const int32_t* category,
                    const uint8_t* image_mask, int32_t n_cats, int32_t n_thr, const double* thr, int32_t n_rec, const double* rec,
                    int32_t n_area, const double* area_rng, int32_t n_maxdet, const int32_t* max_dets,
                    double* precision, double* recall, int64_t* npig, int32_t* rank, int64_t* match_gt, uint8_t* ignore,
                    int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream_) {
    WT_TRY(wt::ensure_device());
    hipStream_t stream = (hipStream_t)stream_;
    WT_TRY(check_sizes(k_sets, n_images, n_cats, n_thr, n_rec, n_area, n_maxdet, n_gt, n_det));
    Params P;
    WT_TRY(pack_params(n_thr, thr, n_rec, rec, n_area, area_rng, n_maxdet, max_dets, &P));
    if (!precision || !recall || !npig || !status_dev || !set_row_offsets || !image_det_offsets || !image_gt_offsets ||
        (match_gt == nullptr) != (ignore == nullptr)) {
        wt::set_error("wt_det_coco: bad argument");
        return WT_ERR_INVALID;
    }
    if ((n_gt > 0 && (!gx || !gy || !gw || !gh || !g_area || !g_cat || !g_crowd)) || (n_det > 0 && (!score || !x || !y || !w || !h || !category))) {
        wt::set_error("wt_det_coco: bad argument");
        return WT_ERR_INVALID;
    }
    const int K = k_sets, C = n_cats, T = n_thr, A = n_area, M = n_maxdet, R = n_rec;
    Workspace ws;
    WT_TRY(carve(wt::align_ptr(workspace), (size_t)K, (size_t)C, (size_t)A, (size_t)n_gt, (size_t)n_det, &ws));
    if (!workspace || workspace_bytes < ws.bytes + 256) {
        wt::set_error("COCO evaluation workspace too small: need %zu bytes, have %zu", ws.bytes + 256, workspace_bytes);
        return WT_ERR_CAPACITY;
    }
    int32_t* rk = rank ? rank : ws.rank;
    const size_t n_npig = (size_t)K * C * A;
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    WT_HIP(hipMemsetAsync(ws.npig, 0, sizeof(long long) * n_npig, stream));
    if (n_det > 0)
        hipLaunchKernelGGL(coco_prep_kernel, dim3((unsigned)((n_det + 255) / 256)), dim3(256), 0, stream, (long long)n_det, K, C, A * T, set_row_offsets,
                           score, category, ws, rk, match_gt, ignore);
    if (n_gt > 0)
        hipLaunchKernelGGL(coco_npig_kernel, dim3((unsigned)((n_gt + 255) / 256), image_mask ? (unsigned)K : 1u), dim3(256), 0, stream, (long long)n_gt,
                           (long long)n_images, C, A, P, g_area, g_cat, g_crowd, image_gt_offsets, image_mask, ws.npig);
    if (!image_mask && K > 1)
        hipLaunchKernelGGL(coco_npig_fill_kernel, dim3((unsigned)((n_npig + 255) / 256)), dim3(256), 0, stream, (long long)n_npig, (long long)C * A, ws.npig);
    WT_HIP(hipMemcpyAsync(npig, ws.npig, sizeof(long long) * n_npig, hipMemcpyDeviceToDevice, stream));
    const size_t n_problems = (size_t)K * (size_t)n_images * (size_t)C;
    if (n_det > 0 && n_problems > 0) {
        const GtCols G = {gx, gy, gw, gh, g_area, g_cat, g_crowd};
        const DetCols D = {score, x, y, w, h, category};
        hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)n_problems), dim3(kWave), 0, stream, G, image_gt_offsets, (long long)n_images, (long long)n_gt,
                           C, T, A, (int)P.max_dets[M - 1], P, set_row_offsets, image_det_offsets, D, image_mask, ws, rk, match_gt, ignore);
    }
    WT_TRY(wt::enqueue_order(ws.o, n_det, K, C, ws.o.order, nullptr, stream));
    if (n_det > 0)
        hipLaunchKernelGGL(coco_gather_rows_kernel, dim3((unsigned)((n_det + 255) / 256)), dim3(256), 0, stream, (long long)n_det, ws.o.order, rk, ws);
    hipLaunchKernelGGL(coco_curve_kernel, dim3((unsigned)((size_t)K * C * A * M * T)), dim3(kCurveThreads), 0, stream, C, T, A, M, R, P, ws, precision, recall);
    WT_HIP(hipGetLastError());
    return WT_OK;
}

int wt_det_coco_host(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh, const double* g_area,
                     const int32_t* g_cat, const uint8_t* g_crowd, int64_t n_images, const int64_t* image_gt_offsets,
                     int32_t k_sets, const int64_t* set_row_offsets, const int64_t* image_det_offsets,
                     const double* score, const double* x, const double* y, const double* w, const double* h, const int32_t* category,
                     const uint8_t* image_mask, int32_t n_cats, int32_t n_thr, const double* thr, int32_t n_rec, const double* rec,
                     int32_t n_area, const double* area_rng, int32_t n_maxdet, const int32_t* max_dets,
                     double* precision, double* recall, int64_t* npig, int32_t* rank, int64_t* match_gt, uint8_t* ignore) {
    if (k_sets < 1 || !set_row_offsets || !image_det_offsets || !image_gt_offsets || !precision || !recall || !npig) {
        wt::set_error("wt_det_coco_host: bad argument");
        return WT_ERR_INVALID;
    }
    const int64_t n_det = set_row_offsets[k_sets];
    WT_TRY(check_sizes(k_sets, n_images, n_cats, n_thr, n_rec, n_area, n_maxdet, n_gt, n_det));
    Params P;
    WT_TRY(pack_params(n_thr, thr, n_rec, rec, n_area, area_rng, n_maxdet, max_dets, &P));
    if ((match_gt == nullptr) != (ignore == nullptr)) { wt::set_error("wt_det_coco_host: match_gt and ignore come together"); return WT_ERR_INVALID; }
    if ((n_gt > 0 && (!gx || !gy || !gw || !gh || !g_area || !g_cat || !g_crowd)) || (n_det > 0 && (!score || !x || !y || !w || !h || !category))) {
        wt::set_error("wt_det_coco_host: bad argument");
        return WT_ERR_INVALID;
    }
    // ---- the layout must be what the kernels walk, and the numbers finite: checked here, the device form trusts its caller ----
    const wt::DetLayout layout = {n_gt, n_images, k_sets, image_gt_offsets, set_row_offsets, image_det_offsets};
    const double* gsrc[5] = {gx, gy, gw, gh, g_area};
    const double* dsrc[5] = {score, x, y, w, h};
    WT_TRY(wt::check_det_layout(layout, "wt_det_coco_host"));
    WT_TRY(wt::check_det_coco_rows(layout, gsrc, g_cat, dsrc, category, n_cats));
    WT_TRY(wt::ensure_device());
    const size_t ng = (size_t)n_gt, nd = (size_t)n_det, K = (size_t)k_sets, C = (size_t)n_cats, T = (size_t)n_thr, A = (size_t)n_area, M = (size_t)n_maxdet,
                 R = (size_t)n_rec, ni = (size_t)n_images;
    const size_t n_prec = K * T * R * C * A * M, n_rcl = K * T * C * A * M, n_np = K * C * A;
    wt::DevBuf dg[5], dgc, dgw, dio, dsr, dido, dd[5], dcat, dmask, dprec, drcl, dnp, drank, dmatch, dign, dstat, dws;
    for (int i = 0; i < 5; ++i) WT_TRY(dg[i].upload(gsrc[i], 8 * ng));
    for (int i = 0; i < 5; ++i) WT_TRY(dd[i].upload(dsrc[i], 8 * nd));
    WT_TRY(dgc.upload(g_cat, 4 * ng));
    WT_TRY(dgw.upload(g_crowd, ng));
    WT_TRY(dcat.upload(category, 4 * nd));
    WT_TRY(dio.upload(image_gt_offsets, 8 * (ni + 1)));
    WT_TRY(dsr.upload(set_row_offsets, 8 * (K + 1)));
    WT_TRY(dido.upload(image_det_offsets, 8 * K * (ni + 1)));
    if (image_mask) WT_TRY(dmask.upload(image_mask, K * ni));
    WT_TRY(dprec.alloc(8 * n_prec)); WT_TRY(drcl.alloc(8 * n_rcl)); WT_TRY(dnp.alloc(8 * n_np));
    WT_TRY(dstat.alloc(16));
    if (rank) WT_TRY(drank.alloc(4 * nd));
    if (match_gt) { WT_TRY(dmatch.alloc(8 * nd * A * T)); WT_TRY(dign.alloc(nd * A * T)); }
    const size_t wsb = wt_det_coco_workspace(k_sets, n_images, n_cats, n_thr, n_rec, n_area, n_maxdet, n_gt, n_det);
    if (!wsb) return WT_ERR_CAPACITY;
    WT_TRY(dws.alloc(wsb));
    WT_TRY(wt_det_coco_dev(n_gt, dg[0].as<double>(), dg[1].as<double>(), dg[2].as<double>(), dg[3].as<double>(), dg[4].as<double>(), dgc.as<int32_t>(),
                           dgw.as<uint8_t>(), n_images, dio.as<int64_t>(), k_sets, n_det, dsr.as<int64_t>(), dido.as<int64_t>(), dd[0].as<double>(),
                           dd[1].as<double>(), dd[2].as<double>(), dd[3].as<double>(), dd[4].as<double>(), dcat.as<int32_t>(),
                           image_mask ? dmask.as<uint8_t>() : nullptr, n_cats, n_thr, thr, n_rec, rec, n_area, area_rng, n_maxdet, max_dets,
                           dprec.as<double>(), drcl.as<double>(), dnp.as<int64_t>(), rank ? drank.as<int32_t>() : nullptr,
                           match_gt ? dmatch.as<int64_t>() : nullptr, match_gt ? dign.as<uint8_t>() : nullptr, dstat.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(wt::finish_det_call(dstat, "COCO evaluation", ""));
    WT_TRY(dprec.download(precision)); WT_TRY(drcl.download(recall)); WT_TRY(dnp.download(npig));
    if (rank) WT_TRY(drank.download(rank));
    if (match_gt) { WT_TRY(dmatch.download(match_gt)); WT_TRY(dign.download(ignore)); }
    return WT_OK;
}

}  // extern "C"
