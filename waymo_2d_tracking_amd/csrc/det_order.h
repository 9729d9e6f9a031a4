// The ordering step of the two detection metrics (det_eval.hip, det_coco_eval.hip; det_order.hip has it): a stable sort of the
// result rows by (segment, key), segment = set * C + class and K * C for the rows that take no part, and the first ordered
// position of every segment.  rocPRIM is included by det_order.hip alone.
#pragma once
#include "common.h"

namespace wt {

struct OrderBufs {
    unsigned long long *key_in, *key_out;     // [n_det] ascending sort keys before / after the first sort; the metric's prep kernel writes key_in
    long long *row_in, *row_mid, *order;      // [n_det] row indices: iota (prep kernel), after the first sort, after the second
    unsigned int *seg, *seg_in, *seg_out;     // [n_det] segment of a row (prep kernel); gathered; sorted
    long long* class_offsets;                 // [K * (C + 1)]
    void* sort_tmp;                           // rocPRIM's temporary storage
    size_t sort_tmp_bytes;
    int bits;                                 // of a segment number
};

// The arrays of a call with n_det rows in K * C segments, out of cv (a base of NULL only counts the bytes).  Carver::take aligns
// every array on its own: the bytes of a workspace do not depend on where in its carve this is called.
int carve_order(Carver& cv, size_t n_det, size_t K, size_t C, OrderBufs* o);

// Enqueue on `stream`: sort by key (64 bits), gather the segments, sort by segment into `order` (o.order or the caller's array),
// then class_offsets[k * (C + 1) + c] = first ordered position of segment k * C + c (c = C: the end of set k's last class) into
// o.class_offsets and, when it is there, class_offsets_out.  Without rows only the offsets kernel runs.
int enqueue_order(const OrderBufs& o, int64_t n_det, int K, int C, long long* order, int64_t* class_offsets_out, hipStream_t stream);

}  // namespace wt
