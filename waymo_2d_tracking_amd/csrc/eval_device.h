// Device side shared by the tracking-metric kernels (mot_eval.hip, mot_identity.hip): the float64 IoU every exactness claim
// of these metrics rests on, the box columns, the per-class thresholds, the compaction of a wavefront's rows and the decoding
// of a block index into its problem.
// Include it only from units compiled with -ffp-contract=off: iou_dd is the IoU in the operation order of
// tracking/sort/sort.py:34-47, and a fused multiply-add in it would change the last bit.
#pragma once
#include "sort_device.h"

namespace wtdev {

constexpr int kMaxClasses = 16;               // thresholds travel as a kernel argument

struct Thresholds { double v[kMaxClasses]; };

// the caller's thresholds; a class beyond n_classes can never match (no IoU reaches 2)
inline Thresholds make_thresholds(const double* thr, int n_classes) {
    Thresholds t;
    for (int i = 0; i < kMaxClasses; ++i) t.v[i] = i < n_classes ? thr[i] : 2.0;
    return t;
}

// sort.py:34-47 on two float64 boxes [x1, y1, x2, y2]
__device__ __forceinline__ double iou_dd(const double a[4], const double b[4]) {
    const double xx1 = (a[0] > b[0]) ? a[0] : b[0];
    const double yy1 = (a[1] > b[1]) ? a[1] : b[1];
    const double xx2 = (a[2] < b[2]) ? a[2] : b[2];
    const double yy2 = (a[3] < b[3]) ? a[3] : b[3];
    double w = xx2 - xx1; if (!(w > 0.)) w = 0.;
    double h = yy2 - yy1; if (!(h > 0.)) h = 0.;
    const double wh = w * h;
    const double area_a = (a[2] - a[0]) * (a[3] - a[1]);
    const double area_b = (b[2] - b[0]) * (b[3] - b[1]);
    return wh / ((area_a + area_b) - wh);
}

struct Boxes {
    const double *x, *y, *w, *h;
    __device__ __forceinline__ void get(long long r, double o[4]) const {
        const double xx = x[r], yy = y[r];
        o[0] = xx; o[1] = yy; o[2] = xx + w[r]; o[3] = yy + h[r];
    }
};

__device__ __forceinline__ double bcast_d(double v, int l) {
    return __longlong_as_double((long long)readlane64((unsigned long long)__double_as_longlong(v), l));
}

// One wavefront: the positions d of [lo, hi) with keep(d), in ascending order, as d - lo into idx (ballot + popcount).
// Returns how many there are, the same number in every lane; nothing is written at or beyond idx[cap].
template <class Index, class Keep>
__device__ __forceinline__ int compact_wave(Index lo, Index hi, Keep keep, int* idx, int cap) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = lanemask_lt();
    int n = 0;
    for (Index base = lo; base < hi; base += kWave) {
        const Index d = base + lane;
        const bool mine = (d < hi) && keep(d);
        const unsigned long long mm = __ballot(mine);
        if (mine) { const int q = n + __popcll(mm & lt); if (q < cap) idx[q] = (int)(d - lo); }
        n += __popcll(mm);
    }
    return n;
}

// rows of class c in [r0, r1), in file order, as offsets from r0; returns how many (more than cap: nothing beyond cap is written)
__device__ __forceinline__ int compact_rows(const int32_t* __restrict__ cat, long long r0, long long r1, int c, int* idx, int cap) {
    return compact_wave(r0, r1, [=](long long d) { return cat[d] == c; }, idx, cap);
}

// block p = (result set k, stream s, class c), the class fastest; classes count from 1
__device__ __forceinline__ void decode_problem(size_t p, int n_streams, int C, int* k, int* s, int* c) {
    *k = (int)(p / ((size_t)n_streams * C));
    *s = (int)((p / C) % n_streams);
    *c = (int)(p % C) + 1;
}

// block p = (job j, stream s), the stream fastest (track_refine.hip)
__device__ __forceinline__ void decode_job_stream(size_t p, int n_streams, int* j, int* s) {
    *j = (int)(p / (size_t)n_streams);
    *s = (int)(p % (size_t)n_streams);
}

}  // namespace wtdev
