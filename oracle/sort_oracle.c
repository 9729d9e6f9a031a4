/* TEST INFRASTRUCTURE ONLY - see wt_oracle.h.  CPU restatement of the reference SORT path.
 * Compile with -ffp-contract=off: every product and sum below is individually rounded, in the order
 * written, and the HIP kernels (waymo_2d_tracking_amd/csrc/sort_engine.hip) use the same order.
 */
#include "wt_oracle.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------------------------------------
 * sort.py:33-47 iou(bb_test = float32 detection row, bb_gt = float64 track row).
 * NumPy-1.x scalar promotion: max/min of (f32,f64) -> f64; the detection area (b2-b0)*(b3-b1) is
 * evaluated entirely in float32; everything else float64.
 */
double wto_iou(const float det[4], const double trk[4])
{
    double xx1 = ((double)det[0] > trk[0]) ? (double)det[0] : trk[0];
    double yy1 = ((double)det[1] > trk[1]) ? (double)det[1] : trk[1];
    double xx2 = ((double)det[2] < trk[2]) ? (double)det[2] : trk[2];
    double yy2 = ((double)det[3] < trk[3]) ? (double)det[3] : trk[3];
    double w = xx2 - xx1; if (!(w > 0.)) w = (w != w) ? w : 0.;   /* np.maximum(0., .) propagates NaN */
    double h = yy2 - yy1; if (!(h > 0.)) h = (h != h) ? h : 0.;
    double wh = w * h;
    float dw = det[2] - det[0];
    float dh = det[3] - det[1];
    float darea = dw * dh;                                        /* float32 product */
    double tarea = (trk[2] - trk[0]) * (trk[3] - trk[1]);
    double o = wh / (((double)darea + tarea) - wh);
    return o;
}

/* ------------------------------------------------------------------------------------------------
 * scikit-learn 0.22.2 sklearn/utils/linear_assignment_.py (call site sort.py:206), restated: classic
 * Munkres on a float32 copy of the cost matrix; rows<=cols enforced by transposing; the first uncovered
 * zero is always taken in row-major order; stars are unique per row/column so they are kept as
 * row_star/col_star index arrays instead of a marks matrix (same information).
 */
typedef struct {
    int n, m;
    float* C;
    unsigned char *row_cov, *col_cov;
    int *row_star, *col_star, *row_prime;
    int64_t* stats;      /* optional work counters (wto_linear_assignment_stats_f32), NULL: none */
} munkres_t;

static void mk_clear_covers(munkres_t* s)
{
    memset(s->row_cov, 0, (size_t)s->n);
    memset(s->col_cov, 0, (size_t)s->m);
}

static int mk_run(munkres_t* s)
{
    const int n = s->n, m = s->m;
    float* C = s->C;
    int r, c;
    /* step 1: subtract the row minimum; star zeros greedily in row-major order */
    for (r = 0; r < n; ++r) {
        float mn = C[(size_t)r * m];
        for (c = 1; c < m; ++c) if (C[(size_t)r * m + c] < mn) mn = C[(size_t)r * m + c];
        for (c = 0; c < m; ++c) C[(size_t)r * m + c] = C[(size_t)r * m + c] - mn;
    }
    for (r = 0; r < n; ++r)
        for (c = 0; c < m; ++c)
            if (C[(size_t)r * m + c] == 0.f && !s->col_cov[c] && !s->row_cov[r]) {
                s->row_star[r] = c; s->col_star[c] = r; s->col_cov[c] = 1; s->row_cov[r] = 1;
            }
    mk_clear_covers(s);
    long guard = 0;
    const long guard_max = 64L + 8L * (long)(n + m) * (long)(n + m) * (long)(n + 1);
    for (;;) {
        /* step 3: cover starred columns; done when every row has a star */
        int stars = 0;
        for (c = 0; c < m; ++c) if (s->col_star[c] >= 0) { s->col_cov[c] = 1; }
        for (r = 0; r < n; ++r) if (s->row_star[r] >= 0) ++stars;
        if (stars >= n) return 0;
        /* step 4 (+6): prime uncovered zeros until one has no star in its row */
        int z0r = -1, z0c = -1;
        for (;;) {
            if (++guard > guard_max) return 5;
            int fr = -1, fc = -1;
            for (r = 0; r < n && fr < 0; ++r) {
                if (s->row_cov[r]) continue;
                for (c = 0; c < m; ++c)
                    if (C[(size_t)r * m + c] == 0.f && !s->col_cov[c]) { fr = r; fc = c; break; }
            }
            if (fr < 0) {
                /* step 6: add the smallest uncovered value to covered rows, subtract from uncovered cols */
                int any_r = 0, any_c = 0, first = 1;
                float mn = 0.f;
                for (r = 0; r < n; ++r) if (!s->row_cov[r]) any_r = 1;
                for (c = 0; c < m; ++c) if (!s->col_cov[c]) any_c = 1;
                if (any_r && any_c) {
                    for (r = 0; r < n; ++r) {
                        if (s->row_cov[r]) continue;
                        for (c = 0; c < m; ++c) {
                            if (s->col_cov[c]) continue;
                            float v = C[(size_t)r * m + c];
                            if (first || v < mn) { mn = v; first = 0; }
                        }
                    }
                    for (r = 0; r < n; ++r)
                        if (s->row_cov[r]) for (c = 0; c < m; ++c) C[(size_t)r * m + c] = C[(size_t)r * m + c] + mn;
                    for (c = 0; c < m; ++c)
                        if (!s->col_cov[c]) for (r = 0; r < n; ++r) C[(size_t)r * m + c] = C[(size_t)r * m + c] - mn;
                    if (s->stats) s->stats[0] += 1;
                }
                continue;
            }
            s->row_prime[fr] = fc;
            if (s->row_star[fr] < 0) { z0r = fr; z0c = fc; break; }
            s->row_cov[fr] = 1;
            s->col_cov[s->row_star[fr]] = 0;
        }
        /* step 5: augmenting path from Z0; stars on the path are removed, primes become stars */
        {
            int pr = z0r, pc = z0c;
            int64_t path_stars = 0;                      /* stars on the path: each one moves to its row's prime */
            for (;;) {
                int r2 = s->col_star[pc];
                s->row_star[pr] = pc; s->col_star[pc] = pr;
                if (r2 < 0) break;
                pr = r2; pc = s->row_prime[r2];
                ++path_stars;
                if (++guard > guard_max) return 5;
            }
            if (s->stats) {
                s->stats[1] += 1;
                if (path_stars > s->stats[2]) s->stats[2] = path_stars;
            }
            mk_clear_covers(s);
            for (r = 0; r < n; ++r) s->row_prime[r] = -1;
        }
    }
}

static int linear_assignment_impl(const float* cost, int n_rows, int n_cols, int* pairs, int* n_pairs, int64_t* stats)
{
    *n_pairs = 0;
    if (n_rows <= 0 || n_cols <= 0) return 0;
    const int transposed = n_cols < n_rows;
    munkres_t s;
    s.stats = stats;
    s.n = transposed ? n_cols : n_rows;
    s.m = transposed ? n_rows : n_cols;
    s.C = (float*)malloc(sizeof(float) * (size_t)s.n * s.m);
    s.row_cov = (unsigned char*)calloc((size_t)s.n, 1);
    s.col_cov = (unsigned char*)calloc((size_t)s.m, 1);
    s.row_star = (int*)malloc(sizeof(int) * (size_t)s.n);
    s.col_star = (int*)malloc(sizeof(int) * (size_t)s.m);
    s.row_prime = (int*)malloc(sizeof(int) * (size_t)s.n);
    int r, c;
    for (r = 0; r < s.n; ++r) { s.row_star[r] = -1; s.row_prime[r] = -1; }
    for (c = 0; c < s.m; ++c) s.col_star[c] = -1;
    for (r = 0; r < s.n; ++r)
        for (c = 0; c < s.m; ++c)
            s.C[(size_t)r * s.m + c] = transposed ? cost[(size_t)c * n_cols + r] : cost[(size_t)r * n_cols + c];
    int rc = mk_run(&s);
    if (rc == 0) {
        int k = 0;
        if (!transposed) {
            for (r = 0; r < s.n; ++r) if (s.row_star[r] >= 0) { pairs[2 * k] = r; pairs[2 * k + 1] = s.row_star[r]; ++k; }
        } else {   /* original rows are the working columns: list them in ascending original-row order */
            for (c = 0; c < s.m; ++c) if (s.col_star[c] >= 0) { pairs[2 * k] = c; pairs[2 * k + 1] = s.col_star[c]; ++k; }
        }
        *n_pairs = k;
    }
    free(s.C); free(s.row_cov); free(s.col_cov); free(s.row_star); free(s.col_star); free(s.row_prime);
    return rc;
}

int wto_linear_assignment_f32(const float* cost, int n_rows, int n_cols, int* pairs, int* n_pairs)
{
    return linear_assignment_impl(cost, n_rows, n_cols, pairs, n_pairs, NULL);
}

/* the same run with work counters: stats[0] step-6 executions that changed the matrix, stats[1] augmenting paths,
 * stats[2] stars on the longest augmenting path */
int wto_linear_assignment_stats_f32(const float* cost, int n_rows, int n_cols, int* pairs, int* n_pairs, int64_t stats[3])
{
    stats[0] = stats[1] = stats[2] = 0;
    return linear_assignment_impl(cost, n_rows, n_cols, pairs, n_pairs, stats);
}

/* test hook: the float32 matrix handed to linear_assignment by wto_associate (sort.py:201-206), -iou, (n, t) row-major */
void wto_iou_cost(const float* dets5, int n, const double* trks4, int t, float* neg)
{
    int d, k;
    for (d = 0; d < n; ++d)
        for (k = 0; k < t; ++k) {
            float v = (float)wto_iou(dets5 + 5 * (size_t)d, trks4 + 4 * (size_t)k);
            neg[(size_t)d * t + k] = -v;
        }
}

/* ------------------------------------------------------------------------------------------------
 * sort.py:193-230 associate_detections_to_trackers
 */
int wto_associate(const float* dets5, int n, const double* trks4, int t, double iou_threshold,
                  int* matches, int* n_matches, int* unmatched_dets, int* n_ud, int* unmatched_trks, int* n_ut)
{
    int d, k;
    *n_matches = 0; *n_ud = 0; *n_ut = 0;
    if (t == 0) {                                  /* sort.py:199-200 */
        for (d = 0; d < n; ++d) unmatched_dets[(*n_ud)++] = d;
        return 0;
    }
    float* iou_matrix = (float*)malloc(sizeof(float) * (size_t)(n > 0 ? n : 1) * t);
    float* neg = (float*)malloc(sizeof(float) * (size_t)(n > 0 ? n : 1) * t);
    for (d = 0; d < n; ++d)
        for (k = 0; k < t; ++k) {
            float v = (float)wto_iou(dets5 + 5 * (size_t)d, trks4 + 4 * (size_t)k);   /* stored float32, sort.py:201,205 */
            iou_matrix[(size_t)d * t + k] = v;
            neg[(size_t)d * t + k] = -v;
        }
    int* pairs = (int*)malloc(sizeof(int) * 2 * (size_t)((n < t ? n : t) + 1));
    int np_ = 0;
    int rc = wto_linear_assignment_f32(neg, n, t, pairs, &np_);
    if (rc == 0) {
        char* dm = (char*)calloc((size_t)n + 1, 1);
        char* tm = (char*)calloc((size_t)t + 1, 1);
        for (k = 0; k < np_; ++k) { dm[pairs[2 * k]] = 1; tm[pairs[2 * k + 1]] = 1; }
        for (d = 0; d < n; ++d) if (!dm[d]) unmatched_dets[(*n_ud)++] = d;      /* sort.py:208-211 */
        for (k = 0; k < t; ++k) if (!tm[k]) unmatched_trks[(*n_ut)++] = k;      /* sort.py:212-215 */
        for (k = 0; k < np_; ++k) {                                             /* sort.py:218-224 */
            int md = pairs[2 * k], mt = pairs[2 * k + 1];
            if ((double)iou_matrix[(size_t)md * t + mt] < iou_threshold) {
                unmatched_dets[(*n_ud)++] = md;
                unmatched_trks[(*n_ut)++] = mt;
            } else {
                matches[2 * (*n_matches)] = md; matches[2 * (*n_matches) + 1] = mt; ++(*n_matches);
            }
        }
        free(dm); free(tm);
    }
    free(iou_matrix); free(neg); free(pairs);
    return rc;
}

/* ------------------------------------------------------------------------------------------------
 * sort.py:78-190 KalmanBoxTracker (+ filterpy KalmanFilter predict/update, restated).
 * F, H are 0/1 matrices, Q, R, P0 diagonal: products with their structural zeros are exact zeros, so the
 * dense numpy.dot sums reduce to the sparse forms below bit-for-bit (up to the sign of zero).
 */
typedef struct {
    double x[7];
    double P[49];
    int64_t id;
    int time_since_update, hit_streak, hits, age;
} track_t;

static const double KQ[7] = {2., 2., 1., 25., 4., 4., 5.};          /* sort.py:111-115 */
static const double KR[4] = {1., 1., 10., 10.};                     /* sort.py:127 */
static const double KP0[7] = {10., 10., 10., 10., 10000., 10000., 10000.};  /* sort.py:133-134 */

/* sort.py:50-62 convert_bbox_to_z on a float32 row */
static void bbox_to_z(const float b[4], double z[4])
{
    float w = b[2] - b[0];
    float h = b[3] - b[1];
    z[0] = (double)b[0] + (double)w / 2.;
    z[1] = (double)b[1] + (double)h / 2.;
    float s = w * h;                       /* float32 product */
    z[2] = (double)s;
    z[3] = (double)w / (double)h;
}

/* sort.py:65-75 convert_x_to_bbox */
static void x_to_bbox(const double x[7], double b[4])
{
    double w = sqrt(x[2] * x[3]);
    double h = x[2] / w;
    b[0] = x[0] - w / 2.;
    b[1] = x[1] - h / 2.;
    b[2] = x[0] + w / 2.;
    b[3] = x[1] + h / 2.;
}

static void track_init(track_t* t, const float bbox[4], int64_t id)
{
    double z[4];
    int i;
    memset(t, 0, sizeof(*t));
    bbox_to_z(bbox, z);
    for (i = 0; i < 4; ++i) t->x[i] = z[i];
    for (i = 0; i < 7; ++i) t->P[i * 7 + i] = KP0[i];
    t->id = id;
}

/* sort.py:166-178 predict(): x = F x ; P = F P F^T + Q */
static void track_predict(track_t* t)
{
    int i, j;
    double FP[49];
    if ((t->x[6] + t->x[2]) <= 0) t->x[6] *= 0.0;
    for (i = 0; i < 3; ++i) t->x[i] = t->x[i] + t->x[i + 4];
    for (i = 0; i < 7; ++i)
        for (j = 0; j < 7; ++j)
            FP[i * 7 + j] = (i < 3) ? (t->P[i * 7 + j] + t->P[(i + 4) * 7 + j]) : t->P[i * 7 + j];
    for (i = 0; i < 7; ++i)
        for (j = 0; j < 7; ++j) {
            double v = (j < 3) ? (FP[i * 7 + j] + FP[i * 7 + j + 4]) : FP[i * 7 + j];
            t->P[i * 7 + j] = (i == j) ? (v + KQ[i]) : v;
        }
    t->age += 1;
    if (t->time_since_update > 0) t->hit_streak = 0;
    t->time_since_update += 1;
}

/* numpy.linalg.inv on 4x4 (LAPACK gesv on the identity): LU with partial pivoting, then forward and
 * back substitution per identity column.  Operation order is fixed here and mirrored on the GPU. */
static void inv4(const double S[16], double SI[16])
{
    double A[16];
    int piv[4];
    int i, j, k;
    memcpy(A, S, sizeof(A));
    for (k = 0; k < 4; ++k) {
        int p = k;
        double best = fabs(A[k * 4 + k]);
        for (i = k + 1; i < 4; ++i) if (fabs(A[i * 4 + k]) > best) { best = fabs(A[i * 4 + k]); p = i; }
        piv[k] = p;
        if (p != k) for (j = 0; j < 4; ++j) { double tmp = A[k * 4 + j]; A[k * 4 + j] = A[p * 4 + j]; A[p * 4 + j] = tmp; }
        for (i = k + 1; i < 4; ++i) {
            A[i * 4 + k] = A[i * 4 + k] / A[k * 4 + k];
            for (j = k + 1; j < 4; ++j) A[i * 4 + j] = A[i * 4 + j] - A[i * 4 + k] * A[k * 4 + j];
        }
    }
    for (j = 0; j < 4; ++j) {
        double b[4] = {0., 0., 0., 0.};
        b[j] = 1.;
        for (k = 0; k < 4; ++k) if (piv[k] != k) { double tmp = b[k]; b[k] = b[piv[k]]; b[piv[k]] = tmp; }
        for (i = 1; i < 4; ++i) for (k = 0; k < i; ++k) b[i] = b[i] - A[i * 4 + k] * b[k];
        for (i = 3; i >= 0; --i) {
            for (k = i + 1; k < 4; ++k) b[i] = b[i] - A[i * 4 + k] * b[k];
            b[i] = b[i] / A[i * 4 + i];
        }
        for (i = 0; i < 4; ++i) SI[i * 4 + j] = b[i];
    }
}

/* sort.py:153-164 update() -> filterpy update: y = z - Hx; S = HPH^T + R; K = PH^T S^-1; x += K y;
 * P = (I-KH) P (I-KH)^T + K R K^T.  Sums run over k ascending, zeros of H/I skipped (exact). */
static void track_update(track_t* t, const float bbox[4])
{
    double z[4], y[4], S[16], SI[16], K[28], A[49], B[49], Pn[49];
    int i, j, k;
    t->time_since_update = 0;
    t->hits += 1;
    t->hit_streak += 1;
    bbox_to_z(bbox, z);
    for (i = 0; i < 4; ++i) y[i] = z[i] - t->x[i];
    for (i = 0; i < 4; ++i) for (j = 0; j < 4; ++j) S[i * 4 + j] = (i == j) ? (t->P[i * 7 + j] + KR[i]) : t->P[i * 7 + j];
    inv4(S, SI);
    for (i = 0; i < 7; ++i)
        for (j = 0; j < 4; ++j) {
            double acc = t->P[i * 7 + 0] * SI[0 * 4 + j];
            for (k = 1; k < 4; ++k) acc = acc + t->P[i * 7 + k] * SI[k * 4 + j];
            K[i * 4 + j] = acc;
        }
    for (i = 0; i < 7; ++i) {
        double acc = K[i * 4 + 0] * y[0];
        for (k = 1; k < 4; ++k) acc = acc + K[i * 4 + k] * y[k];
        t->x[i] = t->x[i] + acc;
    }
    for (i = 0; i < 7; ++i) for (j = 0; j < 7; ++j)
        A[i * 7 + j] = (j < 4) ? (((i == j) ? 1. : 0.) - K[i * 4 + j]) : ((i == j) ? 1. : 0.);
    for (i = 0; i < 7; ++i)
        for (j = 0; j < 7; ++j) {                       /* B = A P */
            double acc = A[i * 7 + 0] * t->P[0 * 7 + j];
            for (k = 1; k < 4; ++k) acc = acc + A[i * 7 + k] * t->P[k * 7 + j];
            if (i >= 4) acc = acc + t->P[i * 7 + j];    /* A[i][i] == 1 */
            B[i * 7 + j] = acc;
        }
    for (i = 0; i < 7; ++i)
        for (j = 0; j < 7; ++j) {                       /* M = B A^T ; KRK = (K R) K^T */
            double acc = B[i * 7 + 0] * A[j * 7 + 0];
            for (k = 1; k < 4; ++k) acc = acc + B[i * 7 + k] * A[j * 7 + k];
            if (j >= 4) acc = acc + B[i * 7 + j];
            double krk = (K[i * 4 + 0] * KR[0]) * K[j * 4 + 0];
            for (k = 1; k < 4; ++k) krk = krk + (K[i * 4 + k] * KR[k]) * K[j * 4 + k];
            Pn[i * 7 + j] = acc + krk;
        }
    memcpy(t->P, Pn, sizeof(Pn));
}

/* ------------------------------------------------------------------------------------------------
 * sort.py:233-296 Sort
 */
struct wto_sort {
    int max_age, min_hits;
    int frame_count;
    track_t* trk;
    int n_trk, cap_trk;
    int64_t* id_counter;
    int64_t own_counter;
};

wto_sort* wto_sort_create(int max_age, int min_hits, int64_t* id_counter)
{
    wto_sort* s = (wto_sort*)calloc(1, sizeof(wto_sort));
    s->max_age = max_age; s->min_hits = min_hits;
    s->id_counter = id_counter ? id_counter : &s->own_counter;
    return s;
}

void wto_sort_destroy(wto_sort* s)
{
    if (!s) return;
    free(s->trk);
    free(s);
}

int wto_sort_state(const wto_sort* s, int cap, int64_t* ids, double* x7, double* P49, int* n_tracks)
{
    int i;
    *n_tracks = s->n_trk;
    if (s->n_trk > cap) return 4;
    for (i = 0; i < s->n_trk; ++i) {
        ids[i] = s->trk[i].id;
        memcpy(x7 + 7 * (size_t)i, s->trk[i].x, sizeof(double) * 7);
        memcpy(P49 + 49 * (size_t)i, s->trk[i].P, sizeof(double) * 49);
    }
    return 0;
}

static int is_bad(double v) { return v != v || v == INFINITY || v == -INFINITY; }

/* test hook: the predicted boxes the NEXT wto_sort_update will associate against (sort.py:256-265), in list order;
 * works on copies, the tracker is not changed */
int wto_sort_predicted(const wto_sort* s, int cap, double* boxes4, int* n_boxes)
{
    int i, t = 0;
    for (i = 0; i < s->n_trk; ++i) {
        track_t c = s->trk[i];
        double b[4];
        track_predict(&c);
        x_to_bbox(c.x, b);
        if (is_bad(b[0]) || is_bad(b[1]) || is_bad(b[2]) || is_bad(b[3])) continue;
        if (t < cap) memcpy(boxes4 + 4 * (size_t)t, b, sizeof(b));
        ++t;
    }
    *n_boxes = t;
    return t > cap ? 4 : 0;
}

int wto_sort_update(wto_sort* s, const float* dets5, int n, double iou_threshold, double* out6, int cap, int* k_out)
{
    int i, k, rc;
    *k_out = 0;
    s->frame_count += 1;
    /* sort.py:256-265 predict every track; drop tracks whose predicted box is not finite */
    double* trks = (double*)malloc(sizeof(double) * 4 * (size_t)(s->n_trk + 1));
    int t = 0;
    for (i = 0; i < s->n_trk; ++i) {
        double b[4];
        track_predict(&s->trk[i]);
        x_to_bbox(s->trk[i].x, b);
        if (is_bad(b[0]) || is_bad(b[1]) || is_bad(b[2]) || is_bad(b[3])) continue;    /* popped */
        if (t != i) s->trk[t] = s->trk[i];
        memcpy(trks + 4 * (size_t)t, b, sizeof(b));
        ++t;
    }
    s->n_trk = t;
    int* matches = (int*)malloc(sizeof(int) * 2 * (size_t)(n + 1));
    int* ud = (int*)malloc(sizeof(int) * (size_t)(2 * n + 1));
    int* ut = (int*)malloc(sizeof(int) * (size_t)(2 * t + 1));
    int nm = 0, nud = 0, nut = 0;
    rc = wto_associate(dets5, n, trks, t, iou_threshold, matches, &nm, ud, &nud, ut, &nut);
    if (rc) { free(trks); free(matches); free(ud); free(ut); return rc; }
    /* sort.py:270-273 update matched tracks (track order) */
    for (k = 0; k < nm; ++k) track_update(&s->trk[matches[2 * k + 1]], dets5 + 5 * (size_t)matches[2 * k]);
    /* sort.py:276-278 new tracks for unmatched detections, in unmatched_dets order */
    for (k = 0; k < nud; ++k) {
        if (s->n_trk == s->cap_trk) {
            s->cap_trk = s->cap_trk ? 2 * s->cap_trk : 16;
            s->trk = (track_t*)realloc(s->trk, sizeof(track_t) * (size_t)s->cap_trk);
        }
        track_init(&s->trk[s->n_trk], dets5 + 5 * (size_t)ud[k], *s->id_counter);
        *s->id_counter += 1;
        s->n_trk += 1;
    }
    /* sort.py:279-293 emit newest first; reap */
    rc = 0;
    for (i = s->n_trk - 1; i >= 0; --i) {
        track_t* tr = &s->trk[i];
        if (tr->time_since_update < 1 && (tr->hit_streak >= s->min_hits || s->frame_count <= s->min_hits)) {
            if (*k_out >= cap) { rc = 4; break; }
            double* o = out6 + 6 * (size_t)(*k_out);
            x_to_bbox(tr->x, o);
            o[4] = (double)(tr->id + 1);
            double err = ((tr->P[0] + tr->P[8]) + tr->P[16]) / 3.0;      /* np.mean of 3 values */
            o[5] = exp(-err * 0.1);
            *k_out += 1;
        }
    }
    t = 0;
    for (i = 0; i < s->n_trk; ++i) {
        if (s->trk[i].time_since_update > s->max_age) continue;
        if (t != i) s->trk[t] = s->trk[i];
        ++t;
    }
    s->n_trk = t;
    free(trks); free(matches); free(ud); free(ut);
    return rc;
}

/* ------------------------------------------------------------------------------------------------
 * tracking/utils.py:25-60 track_sort + :63-96 read_data_file filters + tracker_sort.py:22-51 + track.py:43-47
 */
static double clipd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

int wto_track_streams(int64_t n_dets, const double* x, const double* y, const double* w, const double* h,
                      const double* score, const int32_t* category,
                      int64_t n_frames, const int64_t* frame_det_offsets,
                      int32_t n_streams, const int64_t* stream_frame_offsets,
                      const double* clip_w, const double* clip_h,
                      int max_age, int min_hits, int n_classes,
                      const double* score_threshold, const double* iou_threshold, int64_t id_base,
                      int64_t* out_frame, int32_t* out_category, double* out_bbox4, double* out_score,
                      int64_t* out_object_id, int64_t* n_out, int64_t* n_births)
{
    int64_t counter = id_base;
    int64_t no = 0;
    int rc = 0;
    int32_t s;
    (void)n_frames;
    wto_sort** trackers = (wto_sort**)calloc((size_t)n_classes, sizeof(wto_sort*));
    int* order = (int*)malloc(sizeof(int) * (size_t)n_classes);     /* first-seen class order (dict order) */
    int64_t max_frame = 0;
    for (int64_t f = 0; f < stream_frame_offsets[n_streams]; ++f) {
        int64_t c = frame_det_offsets[f + 1] - frame_det_offsets[f];
        if (c > max_frame) max_frame = c;
    }
    float* buf = (float*)malloc(sizeof(float) * 5 * (size_t)(max_frame + 1));
    double* rows = (double*)malloc(sizeof(double) * 6 * (size_t)(max_frame + 1));
    for (s = 0; s < n_streams && rc == 0; ++s) {
        int n_order = 0;
        memset(trackers, 0, sizeof(wto_sort*) * (size_t)n_classes);
        for (int64_t f = stream_frame_offsets[s]; f < stream_frame_offsets[s + 1] && rc == 0; ++f) {
            const int64_t d0 = frame_det_offsets[f], d1 = frame_det_offsets[f + 1];
            /* tracker_sort.py:29-37: create class trackers in first-seen order (filters of utils.py:79,86 applied) */
            for (int64_t d = d0; d < d1; ++d) {
                int c = category[d];
                if (c < 1 || c > n_classes) { rc = 1; break; }
                if (w[d] < 1 || h[d] < 1) continue;
                if (score[d] < score_threshold[c - 1]) continue;
                if (!trackers[c - 1]) { trackers[c - 1] = wto_sort_create(max_age, min_hits, &counter); order[n_order++] = c; }
            }
            if (rc) break;
            for (int oi = 0; oi < n_order && rc == 0; ++oi) {          /* tracker_sort.py:41-49 */
                const int c = order[oi];
                int n = 0;
                for (int64_t d = d0; d < d1; ++d) {
                    if (category[d] != c || w[d] < 1 || h[d] < 1 || score[d] < score_threshold[c - 1]) continue;
                    buf[5 * n + 0] = (float)x[d];                     /* utils.py:33 + np.array(..., float32) */
                    buf[5 * n + 1] = (float)y[d];
                    buf[5 * n + 2] = (float)(x[d] + w[d]);
                    buf[5 * n + 3] = (float)(y[d] + h[d]);
                    buf[5 * n + 4] = (float)score[d];
                    ++n;
                }
                int k = 0;
                rc = wto_sort_update(trackers[c - 1], buf, n, iou_threshold[c - 1], rows, (int)max_frame + 1, &k);
                if (rc) break;
                for (int i = 0; i < k; ++i) {                         /* utils.py:38-58 */
                    const double* r = rows + 6 * (size_t)i;
                    double x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3], conf = r[5];
                    if (clip_w && clip_w[s] > 0) {
                        x1 = clipd(x1, 0, clip_w[s]); y1 = clipd(y1, 0, clip_h[s]);
                        x2 = clipd(x2, 0, clip_w[s]); y2 = clipd(y2, 0, clip_h[s]);
                        if ((x2 - x1) < 1 || (y2 - y1) < 1) continue;
                        conf = clipd(conf, 0.2, 1.0);
                    }
                    out_frame[no] = f; out_category[no] = c;
                    out_bbox4[4 * no + 0] = x1; out_bbox4[4 * no + 1] = y1;
                    out_bbox4[4 * no + 2] = x2 - x1; out_bbox4[4 * no + 3] = y2 - y1;
                    out_score[no] = conf;
                    out_object_id[no] = (int64_t)r[4];
                    ++no;
                }
            }
        }
        for (int c = 0; c < n_classes; ++c) wto_sort_destroy(trackers[c]);
    }
    (void)n_dets;
    free(trackers); free(order); free(buf); free(rows);
    *n_out = no;
    *n_births = counter - id_base;
    return rc;
}
