// Device side shared by the two detection metrics (det_eval.hip, det_coco_eval.hip): the sort key of a score, the accesses of
// words that a wave's own atomics wrote, the row -> set / image searches, the decoding of a block index into its problem and
// the workgroup prefix sum of the curve kernels.  The two IoUs are different definitions and stay in their units.
// Include it only from units compiled with -ffp-contract=off, like the units it serves.
#pragma once
#include "sort_device.h"

namespace wtdev {

// Larger key = larger value; -0.0 == 0.0; never 0 for a number (both metrics keep 0 for "no row here")
__device__ __forceinline__ unsigned long long desc_key(double v) {
    if (v == 0.0) v = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// A match wave reads words in the workspace that its own atomics wrote: every access of such a word goes to L2.
__device__ __forceinline__ void gsync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    __builtin_amdgcn_wave_barrier();
}
template <class T> __device__ __forceinline__ T slot_load(T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> __device__ __forceinline__ void slot_store(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// set of result row d: the last k < K with set_row_offsets[k] <= d
__device__ __forceinline__ int set_of_row(const int64_t* __restrict__ set_row_offsets, int K, long long d) {
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (set_row_offsets[mid] <= d) lo = mid; else hi = mid;
    }
    return lo;
}
// image of ground-truth row r: the last i < n_images with image_gt_offsets[i] <= r
__device__ __forceinline__ long long image_of_row(const int64_t* __restrict__ image_gt_offsets, long long n_images, long long r) {
    long long lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (image_gt_offsets[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// block p = (result set k, image img, class c), the class fastest and counted from 0; rows() = the set's rows of that image
struct DetProblem {
    long long k, img;
    int c;
    __device__ __forceinline__ DetProblem(size_t p, long long n_images, int C)
        : k((long long)(p / ((size_t)C * (size_t)n_images))), img((long long)((p / (size_t)C) % (size_t)n_images)), c((int)(p % (size_t)C)) {}
    __device__ __forceinline__ void rows(const int64_t* __restrict__ set_row_offsets, const int64_t* __restrict__ image_det_offsets, long long n_images,
                                         long long* d0, long long* d1) const {
        *d0 = set_row_offsets[k] + image_det_offsets[k * (n_images + 1) + img];
        *d1 = set_row_offsets[k] + image_det_offsets[k * (n_images + 1) + img + 1];
    }
};

// exclusive prefix sum over the kWaves wavefronts of a workgroup; *total = the sum.  lds: kWaves ints.
template <int kWaves>
__device__ __forceinline__ int block_excl_sum(int v, int* total, int* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int u = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += u;
    }
    __syncthreads();                                     // the previous use of lds is over
    if (lane == kWave - 1) lds[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int s = lds[w];
        if (w < wave) before += s;
        all += s;
    }
    *total = all;
    return before + inc - v;
}

}  // namespace wtdev
