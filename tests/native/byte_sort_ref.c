/* TEST INFRASTRUCTURE ONLY.  CPU statement of the BYTE-style second association ("second association with
 * low-score detections") on top of the SORT oracle: oracle/sort_oracle.c is included as text, so track_predict, track_update,
 * track_init, x_to_bbox and wto_associate below ARE the oracle's, not copies.  Build with the oracle's flags
 * (-O2 -std=c11 -fPIC -ffp-contract=off -fno-fast-math; tests/byte_ref.py does).
 *
 * One frame of one class tracker (wtb_update), extending sort.py:244-296:
 *   1 predict every track, drop the ones whose predicted box is not finite                    (unchanged)
 *   2 H = the high detections, L = the low ones, both in input order                           (the caller splits)
 *   3 associate(H, all predicted tracks, iou_threshold); matched tracks are updated            (unchanged)
 *   4 R = tracks not matched in 3, ascending list position; if R and L are non-empty: associate(L, boxes of R, low_iou);
 *     a matched track is updated with its low detection; other low detections are dropped
 *   5 births from H only: never-assigned ascending, then threshold-rejected                    (unchanged)
 *   6 emit newest first, reap                                                                  (unchanged)
 */
#include "../../oracle/sort_oracle.c"

enum {
    WTB_SECOND_RUN = 0,      /* second associations run (R and L both non-empty) */
    WTB_SECOND_MATCH,        /* tracks updated by a low detection */
    WTB_SECOND_REJECT,       /* pairs of the second assignment below low_iou */
    WTB_SECOND_TRANSPOSED,   /* second associations with fewer tracks than low detections */
    WTB_FIRST_SKIPPED,       /* second associations run in a frame whose first one had no H or no track */
    WTB_SECOND_NO_TRACK,     /* frames with low detections and tracks alive, but no track left for them */
    WTB_NONFINITE,           /* tracks dropped for a non-finite predicted box */
    WTB_NONFINITE_SECOND,    /* ... in a frame that also ran a second association */
    WTB_LOW_CREATED,         /* class trackers created by a frame whose valid detections of the class were all low */
    WTB_N_STATS
};

static int wtb_update(wto_sort* s, const float* high5, int nh, const float* low5, int nl, double iou_threshold,
                      double low_iou, double* out6, int cap, int* k_out, int64_t* stats)
{
    int i, k, rc;
    *k_out = 0;
    s->frame_count += 1;
    /* 1: sort.py:256-265 */
    const int before = s->n_trk;
    double* trks = (double*)malloc(sizeof(double) * 4 * (size_t)(s->n_trk + 1));
    int t = 0;
    for (i = 0; i < s->n_trk; ++i) {
        double b[4];
        track_predict(&s->trk[i]);
        x_to_bbox(s->trk[i].x, b);
        if (is_bad(b[0]) || is_bad(b[1]) || is_bad(b[2]) || is_bad(b[3])) continue;
        if (t != i) s->trk[t] = s->trk[i];
        memcpy(trks + 4 * (size_t)t, b, sizeof(b));
        ++t;
    }
    s->n_trk = t;
    stats[WTB_NONFINITE] += before - t;
    const int nmax = nh > nl ? nh : nl;
    int* matches = (int*)malloc(sizeof(int) * 2 * (size_t)(nmax + 1));
    int* ud = (int*)malloc(sizeof(int) * (size_t)(2 * nh + 1));
    int* ut = (int*)malloc(sizeof(int) * (size_t)(2 * t + 1));
    int* ud2 = (int*)malloc(sizeof(int) * (size_t)(2 * nl + 1));
    int* ut2 = (int*)malloc(sizeof(int) * (size_t)(2 * t + 1));
    char* taken = (char*)calloc((size_t)t + 1, 1);
    int* rem = (int*)malloc(sizeof(int) * (size_t)(t + 1));
    double* rbox = (double*)malloc(sizeof(double) * 4 * (size_t)(t + 1));
    int nm = 0, nud = 0, nut = 0;
    /* 3: first association, exactly Sort.update's */
    rc = wto_associate(high5, nh, trks, t, iou_threshold, matches, &nm, ud, &nud, ut, &nut);
    if (rc == 0) {
        for (k = 0; k < nm; ++k) {
            track_update(&s->trk[matches[2 * k + 1]], high5 + 5 * (size_t)matches[2 * k]);
            taken[matches[2 * k + 1]] = 1;
        }
        /* 4: second association over the remaining tracks, ascending list position */
        int nr = 0;
        for (i = 0; i < t; ++i)
            if (!taken[i]) { rem[nr] = i; memcpy(rbox + 4 * (size_t)nr, trks + 4 * (size_t)i, sizeof(double) * 4); ++nr; }
        if (nl > 0 && t > 0 && nr == 0) stats[WTB_SECOND_NO_TRACK] += 1;
        if (nr > 0 && nl > 0) {
            int nm2 = 0, nud2 = 0, nut2 = 0;
            rc = wto_associate(low5, nl, rbox, nr, low_iou, matches, &nm2, ud2, &nud2, ut2, &nut2);
            if (rc == 0) {
                for (k = 0; k < nm2; ++k) track_update(&s->trk[rem[matches[2 * k + 1]]], low5 + 5 * (size_t)matches[2 * k]);
                stats[WTB_SECOND_RUN] += 1;
                stats[WTB_SECOND_MATCH] += nm2;
                stats[WTB_SECOND_REJECT] += (nl < nr ? nl : nr) - nm2;       /* every pair of the assignment is kept or rejected */
                if (nr < nl) stats[WTB_SECOND_TRANSPOSED] += 1;
                if (nh == 0) stats[WTB_FIRST_SKIPPED] += 1;
                if (before != t) stats[WTB_NONFINITE_SECOND] += before - t;
            }
        }
    }
    if (rc) { free(trks); free(matches); free(ud); free(ut); free(ud2); free(ut2); free(taken); free(rem); free(rbox); return rc; }
    /* 5: births from H only, in unmatched_dets order (sort.py:276-278) */
    for (k = 0; k < nud; ++k) {
        if (s->n_trk == s->cap_trk) {
            s->cap_trk = s->cap_trk ? 2 * s->cap_trk : 16;
            s->trk = (track_t*)realloc(s->trk, sizeof(track_t) * (size_t)s->cap_trk);
        }
        track_init(&s->trk[s->n_trk], high5 + 5 * (size_t)ud[k], *s->id_counter);
        *s->id_counter += 1;
        s->n_trk += 1;
    }
    /* 6: sort.py:279-293 */
    for (i = s->n_trk - 1; i >= 0; --i) {
        track_t* tr = &s->trk[i];
        if (tr->time_since_update < 1 && (tr->hit_streak >= s->min_hits || s->frame_count <= s->min_hits)) {
            if (*k_out >= cap) { rc = 4; break; }
            double* o = out6 + 6 * (size_t)(*k_out);
            x_to_bbox(tr->x, o);
            o[4] = (double)(tr->id + 1);
            double err = ((tr->P[0] + tr->P[8]) + tr->P[16]) / 3.0;
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
    free(trks); free(matches); free(ud); free(ut); free(ud2); free(ut2); free(taken); free(rem); free(rbox);
    return rc;
}

/* wto_track_streams with the split: a detection is valid when its category is in 1..C, !(w < 1), !(h < 1) and
 * !(score < low_score[c]); a valid one is high when !(score < score_threshold[c]).  Class trackers are created, in first-seen
 * order, by valid detections.  stats: WTB_N_STATS counters, summed over all trackers. */
int wtb_track_streams(int64_t n_dets, const double* x, const double* y, const double* w, const double* h,
                      const double* score, const int32_t* category,
                      int64_t n_frames, const int64_t* frame_det_offsets,
                      int32_t n_streams, const int64_t* stream_frame_offsets,
                      const double* clip_w, const double* clip_h,
                      int max_age, int min_hits, int n_classes,
                      const double* score_threshold, const double* iou_threshold,
                      const double* low_score, const double* low_iou, int64_t id_base,
                      int64_t* out_frame, int32_t* out_category, double* out_bbox4, double* out_score,
                      int64_t* out_object_id, int64_t* n_out, int64_t* n_births, int64_t* stats)
{
    int64_t counter = id_base;
    int64_t no = 0;
    int rc = 0;
    int32_t s;
    (void)n_frames; (void)n_dets;
    memset(stats, 0, sizeof(int64_t) * WTB_N_STATS);
    wto_sort** trackers = (wto_sort**)calloc((size_t)n_classes, sizeof(wto_sort*));
    int* order = (int*)malloc(sizeof(int) * (size_t)n_classes);
    int64_t max_frame = 0;
    for (int64_t f = 0; f < stream_frame_offsets[n_streams]; ++f) {
        int64_t c = frame_det_offsets[f + 1] - frame_det_offsets[f];
        if (c > max_frame) max_frame = c;
    }
    float* hi = (float*)malloc(sizeof(float) * 5 * (size_t)(max_frame + 1));
    float* lo = (float*)malloc(sizeof(float) * 5 * (size_t)(max_frame + 1));
    double* rows = (double*)malloc(sizeof(double) * 6 * (size_t)(max_frame + 1));
    for (s = 0; s < n_streams && rc == 0; ++s) {
        int n_order = 0;
        memset(trackers, 0, sizeof(wto_sort*) * (size_t)n_classes);
        for (int64_t f = stream_frame_offsets[s]; f < stream_frame_offsets[s + 1] && rc == 0; ++f) {
            const int64_t d0 = frame_det_offsets[f], d1 = frame_det_offsets[f + 1];
            for (int64_t d = d0; d < d1; ++d) {
                int c = category[d];
                if (c < 1 || c > n_classes) { rc = 1; break; }
                if (w[d] < 1 || h[d] < 1) continue;
                if (score[d] < low_score[c - 1]) continue;
                if (!trackers[c - 1]) {
                    trackers[c - 1] = wto_sort_create(max_age, min_hits, &counter);
                    order[n_order++] = c;
                    int any_high = 0;
                    for (int64_t e = d0; e < d1; ++e)
                        if (category[e] == c && !(w[e] < 1) && !(h[e] < 1) && !(score[e] < score_threshold[c - 1])) any_high = 1;
                    if (!any_high) stats[WTB_LOW_CREATED] += 1;
                }
            }
            if (rc) break;
            for (int oi = 0; oi < n_order && rc == 0; ++oi) {
                const int c = order[oi];
                int nh = 0, nl = 0;
                for (int64_t d = d0; d < d1; ++d) {
                    if (category[d] != c || w[d] < 1 || h[d] < 1 || score[d] < low_score[c - 1]) continue;
                    float* b;
                    if (!(score[d] < score_threshold[c - 1])) { b = hi + 5 * (size_t)nh; ++nh; } else { b = lo + 5 * (size_t)nl; ++nl; }
                    b[0] = (float)x[d];
                    b[1] = (float)y[d];
                    b[2] = (float)(x[d] + w[d]);
                    b[3] = (float)(y[d] + h[d]);
                    b[4] = (float)score[d];
                }
                int k = 0;
                rc = wtb_update(trackers[c - 1], hi, nh, lo, nl, iou_threshold[c - 1], low_iou[c - 1], rows, (int)max_frame + 1, &k, stats);
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
    free(trackers); free(order); free(hi); free(lo); free(rows);
    *n_out = no;
    *n_births = counter - id_base;
    return rc;
}
