// The ordering step of the two detection metrics (det_order.h): rocPRIM's device radix sort twice, LSD fashion - 64 key bits,
// then the segment bits; both passes are stable, so equal keys keep the input order (image order, then file order).  Its
// temporary storage is part of the caller's workspace.  Integers only.
#include "det_order.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <algorithm>
#include <mutex>

namespace {

// Temporary storage of the two sorts.  The last answer is kept: a sweep launches the same size over and over.
int sort_tmp_bytes(size_t n_det, int bits, size_t* out) {
    static std::mutex mu;
    static size_t last_n = ~(size_t)0, last_bytes = 0;
    static int last_bits = -1;
    std::lock_guard<std::mutex> lock(mu);
    if (n_det == last_n && bits == last_bits) { *out = last_bytes; return WT_OK; }
    size_t a = 0, b = 0;
    unsigned long long* k64 = nullptr;
    unsigned int* k32 = nullptr;
    long long* v = nullptr;
    WT_HIP(rocprim::radix_sort_pairs(nullptr, a, k64, k64, v, v, n_det, 0u, 64u, (hipStream_t) nullptr));
    WT_HIP(rocprim::radix_sort_pairs(nullptr, b, k32, k32, v, v, n_det, 0u, (unsigned)bits, (hipStream_t) nullptr));
    *out = std::max(a, b) + 256;
    last_n = n_det; last_bits = bits; last_bytes = *out;
    return WT_OK;
}

__global__ void det_gather_seg_kernel(long long n, const long long* __restrict__ rows, const unsigned int* __restrict__ seg, unsigned int* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = seg[rows[i]];
}

__global__ void det_offsets_kernel(long long n, int K, int C, const unsigned int* __restrict__ seg_sorted, long long* __restrict__ class_offsets,
                                   int64_t* __restrict__ class_offsets_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)K * (C + 1)) return;
    const unsigned int s = (unsigned int)((i / (C + 1)) * C + i % (C + 1));
    long long lo = 0, hi = n;                            // lower bound of s
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (seg_sorted[mid] < s) lo = mid + 1; else hi = mid;
    }
    class_offsets[i] = lo;
    if (class_offsets_out) class_offsets_out[i] = lo;
}

}  // namespace

namespace wt {

int carve_order(Carver& cv, size_t n_det, size_t K, size_t C, OrderBufs* o) {
    o->bits = 1;                                         // segments 0 .. K * C (the last one = rows that take no part)
    while (((size_t)1 << o->bits) <= K * C) ++o->bits;
    WT_TRY(sort_tmp_bytes(n_det, o->bits, &o->sort_tmp_bytes));
    const size_t nd = n_det ? n_det : 1;
    o->key_in = cv.take<unsigned long long>(nd);
    o->key_out = cv.take<unsigned long long>(nd);
    o->row_in = cv.take<long long>(nd);
    o->row_mid = cv.take<long long>(nd);
    o->order = cv.take<long long>(nd);
    o->seg = cv.take<unsigned int>(nd);
    o->seg_in = cv.take<unsigned int>(nd);
    o->seg_out = cv.take<unsigned int>(nd);
    o->class_offsets = cv.take<long long>(K * (C + 1));
    o->sort_tmp = cv.take<char>(o->sort_tmp_bytes);
    return WT_OK;
}

int enqueue_order(const OrderBufs& o, int64_t n_det, int K, int C, long long* order, int64_t* class_offsets_out, hipStream_t stream) {
    if (n_det > 0) {
        const dim3 grid((unsigned)((n_det + 255) / 256));
        size_t bytes = o.sort_tmp_bytes;
        WT_HIP(rocprim::radix_sort_pairs(o.sort_tmp, bytes, o.key_in, o.key_out, o.row_in, o.row_mid, (size_t)n_det, 0u, 64u, stream));
        hipLaunchKernelGGL(det_gather_seg_kernel, grid, dim3(256), 0, stream, (long long)n_det, o.row_mid, o.seg, o.seg_in);
        bytes = o.sort_tmp_bytes;
        WT_HIP(rocprim::radix_sort_pairs(o.sort_tmp, bytes, o.seg_in, o.seg_out, o.row_mid, order, (size_t)n_det, 0u, (unsigned)o.bits, stream));
    }
    const long long n_off = (long long)K * (C + 1);
    hipLaunchKernelGGL(det_offsets_kernel, dim3((unsigned)((n_off + 255) / 256)), dim3(256), 0, stream, (long long)n_det, K, C, o.seg_out, o.class_offsets,
                       class_offsets_out);
    return WT_OK;
}

}  // namespace wt
