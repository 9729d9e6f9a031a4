// Host side of wd_resize_bilinear_u8 (det_resize.hip): PIL's Image.resize((ow, oh), Image.BILINEAR) on an 8-bit
// RGB image, restated.  The coefficient tables (float64 on the host, one rounding per operation, then 22-bit fixed point), the
// argument checks, and a CPU form of the whole resize that the tests and tools/resize_check.cpp compare with PIL and run under a
// host sanitizer.  Plain C++: no HIP header, so that the file also compiles into a program of its own.
//
// One table per axis.  For an output index xx the source window is bounds[2 * xx] (first) and bounds[2 * xx + 1] (count), its
// weights are coeffs[xx * ksize .. + count); one pass is out = clamp((2^21 + sum pixel[first + x] * k[x]) >> 22, 0, 255) per channel
// in int32.  The horizontal pass comes first and is rounded to 8 bits; the vertical pass reads those bytes.  A pass whose sizes are
// equal is skipped.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/waymotrack.h"

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif

namespace wt {

void set_error(const char* fmt, ...);

constexpr int kResizeMaxSize = 16384;           // per axis: 255 * sum(k) stays below 2^31 and a one-pixel window fits the LDS span
constexpr int kResizeBits = 22;                 // PRECISION_BITS of PIL's 8-bit resampling: 32 - 8 - 2

inline bool resize_size_ok(int v) { return v >= 1 && v <= kResizeMaxSize; }

// Number of coefficient slots per output index; 0 for sizes outside the limits.
inline int resize_ksize(int in_size, int out_size) {
    if (!resize_size_ok(in_size) || !resize_size_ok(out_size)) return 0;
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    return (int)std::ceil(support) * 2 + 1;
}

inline int check_resize_axis(const char* entry, const char* in_name, int in_size, const char* out_name, int out_size) {
    if (!resize_size_ok(in_size)) { set_error("%s: %s = %d outside 1..%d", entry, in_name, in_size, kResizeMaxSize); return WT_ERR_INVALID; }
    if (!resize_size_ok(out_size)) { set_error("%s: %s = %d outside 1..%d", entry, out_name, out_size, kResizeMaxSize); return WT_ERR_INVALID; }
    return WT_OK;
}

// bounds: out_size x 2 (first, count); coeffs: out_size x ksize, zero behind count.  `weights` is scratch of the caller.
// Every operation is rounded on its own: whatever includes this header is compiled with -ffp-contract=off.
inline void resize_build_tables(int in_size, int out_size, int32_t* bounds, int32_t* coeffs, std::vector<double>& weights) {
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    const double ss = 1.0 / fs;
    weights.assign((size_t)ksize, 0.0);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = ((double)xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            const double a = std::fabs(((double)(x + xmin) - center + 0.5) * ss);
            const double w = a < 1.0 ? 1.0 - a : 0.0;
            weights[(size_t)x] = w;
            ww += w;
        }
        int32_t* k = coeffs + (size_t)xx * ksize;
        for (int x = 0; x < xmax; ++x) {
            double w = weights[(size_t)x];
            if (ww != 0.0) w /= ww;
            k[x] = (int32_t)(w * 4194304.0 + 0.5);
        }
        for (int x = xmax; x < ksize; ++x) k[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

// What the kernels and the CPU passes do with a table entry before they use it: the window is cut to the source extent and to the
// table row, so that a wrong table gives wrong pixels and never an access outside the image or the row.
RS_HD void resize_clamp_window(int in_size, int ksize, int& first, int& count) {
    first = first < 0 ? 0 : (first > in_size ? in_size : first);
    const int room = in_size - first;
    count = count < 0 ? 0 : count;
    count = count > ksize ? ksize : count;
    count = count > room ? room : count;
}

RS_HD uint8_t resize_round(int32_t acc) {
    const int32_t v = (acc + (1 << (kResizeBits - 1))) >> kResizeBits;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// (h, w, 3) -> (h, ow, 3)
inline void resize_pass_horizontal(const uint8_t* src, int h, int w, uint8_t* dst, int ow, const int32_t* bounds, const int32_t* coeffs, int ksize) {
    for (int y = 0; y < h; ++y) {
        const uint8_t* row = src + (size_t)y * w * 3;
        uint8_t* out = dst + (size_t)y * ow * 3;
        for (int xx = 0; xx < ow; ++xx) {
            int first = bounds[2 * xx], count = bounds[2 * xx + 1];
            resize_clamp_window(w, ksize, first, count);
            const int32_t* k = coeffs + (size_t)xx * ksize;
            uint32_t acc[3] = {0u, 0u, 0u};                 // unsigned: a wrong table may wrap, a right one stays below 2^31
            for (int x = 0; x < count; ++x)
                for (int c = 0; c < 3; ++c) acc[c] += (uint32_t)row[(size_t)(first + x) * 3 + c] * (uint32_t)k[x];
            for (int c = 0; c < 3; ++c) out[(size_t)xx * 3 + c] = resize_round((int32_t)acc[c]);
        }
    }
}

// (h, row_bytes) -> (oh, row_bytes): the vertical pass does not tell channels from columns
inline void resize_pass_vertical(const uint8_t* src, int h, size_t row_bytes, uint8_t* dst, int oh, const int32_t* bounds, const int32_t* coeffs, int ksize) {
    for (int yy = 0; yy < oh; ++yy) {
        int first = bounds[2 * yy], count = bounds[2 * yy + 1];
        resize_clamp_window(h, ksize, first, count);
        const int32_t* k = coeffs + (size_t)yy * ksize;
        uint8_t* out = dst + (size_t)yy * row_bytes;
        for (size_t b = 0; b < row_bytes; ++b) {
            uint32_t acc = 0u;
            for (int y = 0; y < count; ++y) acc += (uint32_t)src[(size_t)(first + y) * row_bytes + b] * (uint32_t)k[y];
            out[b] = resize_round((int32_t)acc);
        }
    }
}

// Bytes of the 8-bit intermediate (h, ow, 3): 0 when at most one pass runs.  Sizes outside the limits give 0 too.
inline size_t resize_workspace_bytes(int h, int w, int oh, int ow) {
    if (!resize_size_ok(h) || !resize_size_ok(w) || !resize_size_ok(oh) || !resize_size_ok(ow)) return 0;
    return (w != ow && h != oh) ? (size_t)h * ow * 3 : 0;
}

inline int check_resize_args(const char* entry, const void* src, int h, int w, const void* dst, int oh, int ow) {
    if (check_resize_axis(entry, "h", h, "oh", oh) != WT_OK || check_resize_axis(entry, "w", w, "ow", ow) != WT_OK) return WT_ERR_INVALID;
    if (!src) { set_error("%s: src is null", entry); return WT_ERR_INVALID; }
    if (!dst) { set_error("%s: dst is null", entry); return WT_ERR_INVALID; }
    return WT_OK;
}

// wd_resize_tables_host: bounds holds out_size x 2 entries, coeffs out_size x resize_ksize(in_size, out_size)
inline int resize_tables_checked(const char* entry, int in_size, int out_size, int32_t* bounds, int32_t* coeffs) {
    if (check_resize_axis(entry, "in_size", in_size, "out_size", out_size) != WT_OK) return WT_ERR_INVALID;
    if (!bounds) { set_error("%s: bounds is null", entry); return WT_ERR_INVALID; }
    if (!coeffs) { set_error("%s: coeffs is null", entry); return WT_ERR_INVALID; }
    std::vector<double> weights;
    resize_build_tables(in_size, out_size, bounds, coeffs, weights);
    return WT_OK;
}

// The whole resize on the CPU.
inline int resize_bilinear_u8_cpu(const uint8_t* src, int h, int w, uint8_t* dst, int oh, int ow) {
    const char* entry = "wd_resize_bilinear_u8_host";
    const int rc = check_resize_args(entry, src, h, w, dst, oh, ow);
    if (rc != WT_OK) return rc;
    std::vector<int32_t> bounds, coeffs;
    std::vector<double> weights;
    std::vector<uint8_t> mid;
    const uint8_t* cur = src;
    if (w != ow) {
        const int ksize = resize_ksize(w, ow);
        bounds.resize((size_t)ow * 2);
        coeffs.resize((size_t)ow * ksize);
        resize_build_tables(w, ow, bounds.data(), coeffs.data(), weights);
        uint8_t* out = dst;
        if (h != oh) { mid.resize((size_t)h * ow * 3); out = mid.data(); }
        resize_pass_horizontal(src, h, w, out, ow, bounds.data(), coeffs.data(), ksize);
        cur = out;
    }
    if (h != oh) {
        const int ksize = resize_ksize(h, oh);
        bounds.resize((size_t)oh * 2);
        coeffs.resize((size_t)oh * ksize);
        resize_build_tables(h, oh, bounds.data(), coeffs.data(), weights);
        resize_pass_vertical(cur, h, (size_t)ow * 3, dst, oh, bounds.data(), coeffs.data(), ksize);
    } else if (w == ow) {
        for (size_t i = 0, n = (size_t)h * w * 3; i < n; ++i) dst[i] = src[i];
    }
    return WT_OK;
}

}  // namespace wt
