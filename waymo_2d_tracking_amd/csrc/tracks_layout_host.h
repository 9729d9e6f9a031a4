// Host side of wt_tracks_layout_host and wt_tracks_to_eval_host (tracks_layout.hip): the inputs they take, the
// checks they make before they touch a device, and the first probe of the id table.  Host code only, so that the checks can also
// be compiled into a program of their own (tools/tracks_layout_check.cpp).
#pragma once
#include "tracks_host.h"

namespace wt {

constexpr int64_t kLayoutMaxRows = 1ll << 30;     // rows of one result: row indices and twice their number stay int32 / uint32

// First probe of `id` in an open-addressing table of `capacity` slots (Fibonacci hashing of all 64 bits; the later probes follow
// linearly).  The same function runs in the kernel.
__host__ __device__ inline uint32_t layout_probe(int64_t id, uint32_t capacity) {
    const uint64_t mixed = (uint64_t)id * 0x9E3779B97F4A7C15ull;
    return (uint32_t)(mixed >> 32) % capacity;
}

// R tracking results as wt_tracks_layout_host takes them (include/waymotrack.h): the rows of the tracker, result after result.
struct LayoutInput {
    int64_t n_frames;
    int32_t n_streams;
    const int64_t* stream_frame_offsets;
    int32_t r_sets;
    const int64_t *in_row_offsets, *frame;
    const int32_t* category;
    const double *bbox, *score;
    const int64_t* object_id;
    int32_t n_classes;
};

// Arguments, stream offsets, row counts; then per row the frame slot (inside the packed set, ascending) and the category.
// On WT_OK: *max_rows is the largest row count of one result and *n_rows their sum.
inline int check_layout_input(const LayoutInput& in, int64_t* max_rows, int64_t* n_rows) {
    const char* entry = "wt_tracks_layout_host";
    if (in.r_sets < 1 || in.n_streams < 0 || in.n_frames < 0 || in.n_classes < 1 || !in.stream_frame_offsets || !in.in_row_offsets) {
        set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if (in.stream_frame_offsets[0] != 0 || in.stream_frame_offsets[in.n_streams] != in.n_frames || in.in_row_offsets[0] != 0) {
        set_error("%s: CSR offsets do not cover the rows", entry);
        return WT_ERR_INVALID;
    }
    for (int32_t s = 0; s < in.n_streams; ++s)
        if (in.stream_frame_offsets[s + 1] < in.stream_frame_offsets[s]) { set_error("stream_frame_offsets must be non-decreasing"); return WT_ERR_INVALID; }
    *max_rows = 0;
    for (int32_t r = 0; r < in.r_sets; ++r) {
        const int64_t rows = in.in_row_offsets[r + 1] - in.in_row_offsets[r];
        if (rows < 0) { set_error("result %d: negative row count", (int)r); return WT_ERR_INVALID; }
        if (rows >= kLayoutMaxRows) { set_error("result %d: %lld rows in one result", (int)r, (long long)rows); return WT_ERR_CAPACITY; }
        if (rows > *max_rows) *max_rows = rows;
    }
    *n_rows = in.in_row_offsets[in.r_sets];
    if (*n_rows > 0 && !(in.frame && in.category && in.bbox && in.score && in.object_id)) { set_error("%s: bad argument", entry); return WT_ERR_INVALID; }
    for (int32_t r = 0; r < in.r_sets; ++r) {
        const int64_t base = in.in_row_offsets[r];
        for (int64_t i = base; i < in.in_row_offsets[r + 1]; ++i) {
            const int64_t f = in.frame[i];
            if (f < 0 || f >= in.n_frames) {
                set_error("result %d, row %lld: frame slot %lld outside 0..%lld", (int)r, (long long)(i - base), (long long)f, (long long)in.n_frames - 1);
                return WT_ERR_INVALID;
            }
            if (i > base && in.frame[i - 1] > f) {
                set_error("result %d, row %lld: frame slot %lld after %lld (the rows of a result ascend by frame slot)", (int)r, (long long)(i - base),
                          (long long)f, (long long)in.frame[i - 1]);
                return WT_ERR_INVALID;
            }
            if (in.category[i] < 1 || in.category[i] > in.n_classes) {
                set_error("result %d, row %lld: category %d outside 1..%d", (int)r, (long long)(i - base), (int)in.category[i], (int)in.n_classes);
                return WT_ERR_INVALID;
            }
        }
    }
    return WT_OK;
}

// K results in the shared layout and the slot map as wt_tracks_to_eval_host takes them.
struct ToEvalInput {
    int64_t n_frames;
    int32_t k_sets;
    const int64_t *set_row_offsets, *frame_row_offsets;
    const double *x, *y, *w, *h;
    int64_t box_stride;
    const int32_t *category, *local;
    const int64_t* slot_map;
    int64_t n_gt_frames;
    int32_t n_classes;
};

// Arguments, CSR cover, slot offsets, the slot map (-1 or a ground-truth slot, none named twice), local indices.
// On WT_OK: *max_slot_rows is the most rows of one frame slot and *n_rows the rows of all results.
inline int check_to_eval_input(const ToEvalInput& in, int64_t* max_slot_rows, int64_t* n_rows) {
    const char* entry = "wt_tracks_to_eval_host";
    if (in.k_sets < 1 || in.n_frames < 0 || in.n_gt_frames < 0 || in.n_classes < 1 || in.box_stride < 1 || !in.set_row_offsets || !in.frame_row_offsets ||
        (in.n_frames > 0 && !in.slot_map)) {
        set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if (in.set_row_offsets[0] != 0) { set_error("%s: CSR offsets do not cover the rows", entry); return WT_ERR_INVALID; }
    *n_rows = in.set_row_offsets[in.k_sets];
    if (*n_rows > 0 && !(in.x && in.y && in.w && in.h && in.category && in.local)) { set_error("%s: bad argument", entry); return WT_ERR_INVALID; }
    std::vector<int64_t> named((size_t)in.n_gt_frames, -1);
    for (int64_t f = 0; f < in.n_frames; ++f) {
        const int64_t g = in.slot_map[f];
        if (g < -1 || g >= in.n_gt_frames) {
            set_error("slot_map: frame slot %lld names ground-truth slot %lld outside -1..%lld", (long long)f, (long long)g, (long long)in.n_gt_frames - 1);
            return WT_ERR_INVALID;
        }
        if (g < 0) continue;
        if (named[(size_t)g] >= 0) {
            set_error("slot_map: ground-truth slot %lld is named by the frame slots %lld and %lld", (long long)g, (long long)named[(size_t)g], (long long)f);
            return WT_ERR_INVALID;
        }
        named[(size_t)g] = f;
    }
    for (int32_t k = 0; k < in.k_sets; ++k)                   // before any row is read: every set lies inside the rows
        if (in.set_row_offsets[k + 1] < in.set_row_offsets[k]) { set_error("result %d: negative row count", (int)k); return WT_ERR_INVALID; }
    *max_slot_rows = 0;
    for (int32_t k = 0; k < in.k_sets; ++k) {
        const int64_t* fro = in.frame_row_offsets + (size_t)k * (size_t)(in.n_frames + 1);
        const int64_t base = in.set_row_offsets[k], rows = in.set_row_offsets[k + 1] - base;
        if (fro[0] != 0 || fro[in.n_frames] > rows) { set_error("result %d: frame_row_offsets do not fit its rows", (int)k); return WT_ERR_INVALID; }
        if (rows >= kLayoutMaxRows) { set_error("result %d: %lld rows in one result", (int)k, (long long)rows); return WT_ERR_CAPACITY; }
        for (int64_t f = 0; f < in.n_frames; ++f) {
            if (fro[f + 1] < fro[f]) { set_error("result %d: frame_row_offsets must be non-decreasing", (int)k); return WT_ERR_INVALID; }
            if (fro[f + 1] - fro[f] > *max_slot_rows) *max_slot_rows = fro[f + 1] - fro[f];
        }
        for (int64_t i = base; i < base + rows; ++i)
            if (in.local[i] < 0) { set_error("result %d, row %lld: trajectory index %d is negative", (int)k, (long long)(i - base), (int)in.local[i]); return WT_ERR_INVALID; }
    }
    return WT_OK;
}

}  // namespace wt
