// Host side shared by the *_host forms of the two detection metrics (det_eval.hip, det_coco_eval.hip): the layout both take,
// the checks both make before they touch a device, and the read-back of the status word.
#pragma once
#include "common.h"

namespace wt {

// The three CSR arrays of wt_det_eval_* / wt_det_coco_* (include/waymotrack.h) and their counts.  Host pointers.
struct DetLayout {
    int64_t n_gt, n_images;
    int32_t k_sets;
    const int64_t *image_gt_offsets, *set_row_offsets, *image_det_offsets;
};

// Cover and order of the ground-truth offsets; `entry` is the name of the entry point ("...._host").  The device form trusts its caller.
inline int check_det_layout(const DetLayout& in, const char* entry) {
    if (in.image_gt_offsets[0] != 0 || in.image_gt_offsets[in.n_images] != in.n_gt || in.set_row_offsets[0] != 0) {
        set_error("%s: CSR offsets do not cover the rows", entry);
        return WT_ERR_INVALID;
    }
    for (int64_t i = 0; i < in.n_images; ++i)
        if (in.image_gt_offsets[i + 1] < in.image_gt_offsets[i]) { set_error("image_gt_offsets must be non-decreasing (image %lld)", (long long)i); return WT_ERR_INVALID; }
    return WT_OK;
}

// gt_row(r) for every ground-truth row, then for every result set the cover and order of its image offsets and
// set_row(k, r - first row of the set, r) for its rows; the first status that is not WT_OK ends the walk.  After check_det_layout().
template <class GtRow, class SetRow>
int walk_det_rows(const DetLayout& in, GtRow gt_row, SetRow set_row) {
    for (int64_t r = 0; r < in.n_gt; ++r) WT_TRY(gt_row(r));
    for (int32_t k = 0; k < in.k_sets; ++k) {
        const int64_t* ido = in.image_det_offsets + (size_t)k * (size_t)(in.n_images + 1);
        const int64_t base = in.set_row_offsets[k], rows = in.set_row_offsets[k + 1] - base;
        if (rows < 0 || ido[0] != 0 || ido[in.n_images] != rows) { set_error("result set %d: image_det_offsets do not cover its rows", (int)k); return WT_ERR_INVALID; }
        for (int64_t i = 0; i < in.n_images; ++i)
            if (ido[i + 1] < ido[i]) { set_error("result set %d: image_det_offsets must be non-decreasing (image %lld)", (int)k, (long long)i); return WT_ERR_INVALID; }
        for (int64_t r = base; r < base + rows; ++r) WT_TRY(set_row(k, r - base, r));
    }
    return WT_OK;
}

// wt_det_eval_host: every label and category is one of 1..n_classes
inline int check_det_eval_rows(const DetLayout& in, const int32_t* g_label, const int32_t* category, int32_t n_classes) {
    return walk_det_rows(in, [&](int64_t r) {
        if (g_label[r] >= 1 && g_label[r] <= n_classes) return WT_OK;
        set_error("ground-truth row %lld: label %d outside 1..%d", (long long)r, (int)g_label[r], (int)n_classes);
        return WT_ERR_INVALID;
    }, [&](int32_t k, int64_t i, int64_t r) {
        if (category[r] >= 1 && category[r] <= n_classes) return WT_OK;
        set_error("result set %d, row %lld: category %d outside 1..%d", (int)k, (long long)i, (int)category[r], (int)n_classes);
        return WT_ERR_INVALID;
    });
}

// wt_det_coco_host (section 28): every category index is one of 0..n_cats - 1 and every number finite.  g = x, y, w, h, area of
// the ground truth, d = score, x, y, w, h of the results.
inline int check_det_coco_rows(const DetLayout& in, const double* const g[5], const int32_t* g_cat, const double* const d[5], const int32_t* category, int32_t n_cats) {
    auto finite = [](const double* const col[5], int64_t r) {
        for (int i = 0; i < 5; ++i)
            if (!(col[i][r] - col[i][r] == 0.0)) return false;      // NaN - NaN and inf - inf are NaN
        return true;
    };
    return walk_det_rows(in, [&](int64_t r) {
        if (g_cat[r] < 0 || g_cat[r] >= n_cats) {
            set_error("ground-truth row %lld: category index %d outside 0..%d", (long long)r, (int)g_cat[r], (int)n_cats - 1);
            return WT_ERR_INVALID;
        }
        if (!finite(g, r)) { set_error("ground-truth row %lld: a coordinate or the area is not finite", (long long)r); return WT_ERR_INVALID; }
        return WT_OK;
    }, [&](int32_t k, int64_t i, int64_t r) {
        if (category[r] < 0 || category[r] >= n_cats) {
            set_error("result set %d, row %lld: category index %d outside 0..%d", (int)k, (long long)i, (int)category[r], (int)n_cats - 1);
            return WT_ERR_INVALID;
        }
        if (!finite(d, r)) { set_error("result set %d, row %lld: the score or a coordinate is not finite", (int)k, (long long)i); return WT_ERR_INVALID; }
        return WT_OK;
    });
}

// wait for the launch and read the kernels' status word; the message is "`what` kernel reported status N`legend`"
inline int finish_det_call(const DevBuf& status, const char* what, const char* legend) {
    WT_HIP(hipDeviceSynchronize());
    int32_t st = 0;
    WT_HIP(hipMemcpy(&st, status.p, sizeof(st), hipMemcpyDeviceToHost));
    if (st) set_error("%s kernel reported status %d%s", what, (int)st, legend);
    return (int)st;
}

}  // namespace wt
