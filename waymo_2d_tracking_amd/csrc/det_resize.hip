// PIL's Image.resize((ow, oh), Image.BILINEAR) on an (h, w, 3) uint8 DEVICE image, bit for bit: the reference's
// Resize transform behind --resize (detnet/inference.py:170-178).  PIL's 8-bit resampling is 22-bit fixed point with int32 sums, so
// the kernels are integer only; the coefficient tables are built on the host (csrc/resize_host.h, float64, this unit is compiled with
// -ffp-contract=off) and read here as int32.  Two launches: the horizontal pass writes an 8-bit intermediate (h, ow, 3) into the
// caller's workspace, the vertical pass reads it.  A pass whose sizes are equal is skipped.
//
// RGB is interleaved bytes and neither a row nor a pointer needs to be 4-byte aligned, so both kernels move ALIGNED words of the
// address space: a word that lies inside the image is one dword access, the at most two words per buffer that straddle its ends are
// touched byte by byte.  No byte-wide global load is in a tap loop.
#include "common.h"
#include "resize_host.h"
#include "../../include/waymodet.h"

namespace {

constexpr int kThreads = 256;
constexpr size_t kLdsBudget = 64 * 1024;

// the aligned word at p, with the bytes outside [lo, hi) as 0
__device__ __forceinline__ uint32_t load_word(uintptr_t p, uintptr_t lo, uintptr_t hi) {
    if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (p + b >= lo && p + b < hi) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(p + b) << (8 * b);
    return v;
}

// the aligned word at p; only its bytes inside [lo, hi) are written
__device__ __forceinline__ void store_word(uintptr_t p, uint32_t v, uintptr_t lo, uintptr_t hi) {
    if (p >= lo && p + 4 <= hi) { *reinterpret_cast<uint32_t*>(p) = v; return; }
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (p + b >= lo && p + b < hi) *reinterpret_cast<uint8_t*>(p + b) = (uint8_t)(v >> (8 * b));
}

struct HorizontalArgs {
    const uint8_t* src;         // (h, w, 3)
    uint8_t* dst;               // (h, ow, 3)
    const int32_t *bounds, *coeffs;
    int h, w, ow, ksize;
    int tile, tile_shift;       // output pixels of a row per workgroup: a power of two <= 64
    int rows;                   // rows per workgroup
    int span;                   // source pixels of a row that the LDS holds: covers the windows of `tile` neighbouring outputs
    int in_words, out_words;    // LDS words per row: source span, output tile (each with room for the 0..3 bytes in front of it)
};

// Workgroup = `rows` rows x `tile` output pixels.  The source span of the tile is staged through LDS at the byte offset it has
// inside its first aligned word, every item (row, output pixel) sums its window from LDS for the three channels, and the output
// bytes go back through LDS to be stored as aligned words.
__global__ __launch_bounds__(kThreads) void resize_horizontal_kernel(HorizontalArgs a) {
    extern __shared__ uint32_t lds[];
    uint32_t* lds_in = lds;
    uint32_t* lds_out = lds + (size_t)a.rows * a.in_words;
    const int ox0 = blockIdx.x * a.tile, y0 = blockIdx.y * a.rows;
    const int n_rows = min(a.rows, a.h - y0), n_out = min(a.tile, a.ow - ox0);
    const uintptr_t src_lo = (uintptr_t)a.src, src_hi = src_lo + (size_t)a.h * a.w * 3;

    int f0 = a.bounds[2 * ox0], c0 = a.bounds[2 * ox0 + 1];
    wt::resize_clamp_window(a.w, a.ksize, f0, c0);
    const int span = min(a.span, a.w - f0);                       // pixels staged per row, from f0 on
    for (int r = 0; r < n_rows; ++r) {
        const uintptr_t first = src_lo + ((size_t)(y0 + r) * a.w + f0) * 3;
        const uintptr_t base = first & ~(uintptr_t)3;
        const int n_words = (int)((first - base) + (size_t)span * 3 + 3) / 4;
        for (int j = threadIdx.x; j < n_words; j += kThreads) lds_in[r * a.in_words + j] = load_word(base + 4 * (uintptr_t)j, src_lo, src_hi);
    }
    __syncthreads();

    for (int i = threadIdx.x; i < (n_rows << a.tile_shift); i += kThreads) {
        const int r = i >> a.tile_shift, px = i & (a.tile - 1);
        if (px >= n_out) continue;
        const int ox = ox0 + px, y = y0 + r;
        int first = a.bounds[2 * ox], count = a.bounds[2 * ox + 1];
        wt::resize_clamp_window(a.w, a.ksize, first, count);
        int rel = first - f0;                                     // a right table ascends: 0 <= rel and rel + count <= span
        rel = rel < 0 ? 0 : (rel > span ? span : rel);
        count = min(count, span - rel);
        const uintptr_t row_first = src_lo + ((size_t)y * a.w + f0) * 3;
        const uint8_t* in = reinterpret_cast<const uint8_t*>(lds_in + r * a.in_words) + (row_first & 3) + rel * 3;
        const int32_t* k = a.coeffs + (size_t)ox * a.ksize;
        uint32_t acc0 = 0, acc1 = 0, acc2 = 0;
        for (int x = 0; x < count; ++x) {
            const uint32_t c = (uint32_t)k[x];
            acc0 += in[3 * x] * c;
            acc1 += in[3 * x + 1] * c;
            acc2 += in[3 * x + 2] * c;
        }
        const uintptr_t out_first = (uintptr_t)a.dst + ((size_t)y * a.ow + ox0) * 3;
        uint8_t* out = reinterpret_cast<uint8_t*>(lds_out + r * a.out_words) + (out_first & 3) + px * 3;
        out[0] = wt::resize_round((int32_t)acc0);
        out[1] = wt::resize_round((int32_t)acc1);
        out[2] = wt::resize_round((int32_t)acc2);
    }
    __syncthreads();

    for (int r = 0; r < n_rows; ++r) {
        const uintptr_t lo = (uintptr_t)a.dst + ((size_t)(y0 + r) * a.ow + ox0) * 3, hi = lo + (size_t)n_out * 3;
        const uintptr_t base = lo & ~(uintptr_t)3;
        const int n_words = (int)((lo - base) + (size_t)n_out * 3 + 3) / 4;
        for (int j = threadIdx.x; j < n_words; j += kThreads) store_word(base + 4 * (uintptr_t)j, lds_out[r * a.out_words + j], lo, hi);
    }
}

struct VerticalArgs {
    const uint8_t* src;         // (h, row_bytes)
    uint8_t* dst;               // (oh, row_bytes)
    const int32_t *bounds, *coeffs;
    int h, oh, ksize;
    size_t row_bytes;
};

// blockIdx.y = output row, a lane owns one aligned word of it: its `count` source reads are the four bytes at the same columns of
// the rows above, neighbouring lanes read neighbouring bytes.  A source row is shifted against the output row by the rows' pitch
// modulo 4, so the four bytes come out of two aligned words.  The coefficients are uniform over the workgroup.
__global__ __launch_bounds__(kThreads) void resize_vertical_kernel(VerticalArgs a) {
    const int oy = blockIdx.y;
    const uintptr_t lo = (uintptr_t)a.dst + (size_t)oy * a.row_bytes, hi = lo + a.row_bytes;
    const uintptr_t base = lo & ~(uintptr_t)3;
    const size_t n_words = ((lo - base) + a.row_bytes + 3) / 4;
    const size_t j = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n_words) return;
    const uintptr_t src_lo = (uintptr_t)a.src, src_hi = src_lo + (size_t)a.h * a.row_bytes;
    int first = a.bounds[2 * oy], count = a.bounds[2 * oy + 1];
    wt::resize_clamp_window(a.h, a.ksize, first, count);
    const int32_t* k = a.coeffs + (size_t)oy * a.ksize;
    const int64_t column = (int64_t)(4 * j) - (int64_t)(lo - base);          // of the word's byte 0: -3 .. row_bytes - 1
    uint32_t acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    for (int t = 0; t < count; ++t) {
        const uintptr_t q = (uintptr_t)((int64_t)src_lo + (int64_t)((size_t)(first + t) * a.row_bytes) + column);
        const unsigned shift = (unsigned)(q & 3) * 8;
        const uintptr_t q0 = q & ~(uintptr_t)3;
        const uint32_t w0 = load_word(q0, src_lo, src_hi);
        const uint32_t w1 = shift ? load_word(q0 + 4, src_lo, src_hi) : 0u;
        const uint32_t v = (uint32_t)((((uint64_t)w1 << 32) | w0) >> shift);
        const uint32_t c = (uint32_t)k[t];
        acc0 += (v & 255u) * c;
        acc1 += ((v >> 8) & 255u) * c;
        acc2 += ((v >> 16) & 255u) * c;
        acc3 += (v >> 24) * c;
    }
    const uint32_t v = (uint32_t)wt::resize_round((int32_t)acc0) | ((uint32_t)wt::resize_round((int32_t)acc1) << 8) |
                       ((uint32_t)wt::resize_round((int32_t)acc2) << 16) | ((uint32_t)wt::resize_round((int32_t)acc3) << 24);
    store_word(base + 4 * j, v, lo, hi);
}

int launch_horizontal(const uint8_t* src, int h, int w, uint8_t* dst, int ow, const int32_t* bounds, const int32_t* coeffs, hipStream_t stream) {
    HorizontalArgs a;
    a.src = src; a.dst = dst; a.bounds = bounds; a.coeffs = coeffs;
    a.h = h; a.w = w; a.ow = ow; a.ksize = wt::resize_ksize(w, ow);
    const double scale = (double)w / (double)ow;
    a.tile = 64; a.rows = 4;
    size_t lds_bytes = 0;
    for (;;) {
        const double reach = std::ceil((double)(a.tile - 1) * scale) + (double)a.ksize + 2.0;      // windows of `tile` neighbouring outputs
        a.span = reach < (double)w ? (int)reach : w;
        a.in_words = (a.span * 3 + 6) / 4;
        a.out_words = (a.tile * 3 + 6) / 4;
        lds_bytes = (size_t)a.rows * (size_t)(a.in_words + a.out_words) * 4;
        if (lds_bytes <= kLdsBudget || (a.rows == 1 && a.tile == 1)) break;
        if (a.rows > 1) a.rows /= 2; else a.tile /= 2;
    }
    if (lds_bytes > kLdsBudget) { wt::set_error("wd_resize_bilinear_u8: a %d -> %d row does not fit the LDS", w, ow); return WT_ERR_CAPACITY; }
    a.tile_shift = 0;
    while ((1 << a.tile_shift) < a.tile) ++a.tile_shift;
    const dim3 grid((unsigned)((ow + a.tile - 1) / a.tile), (unsigned)((h + a.rows - 1) / a.rows));
    hipLaunchKernelGGL(resize_horizontal_kernel, grid, dim3(kThreads), lds_bytes, stream, a);
    return WT_OK;
}

void launch_vertical(const uint8_t* src, int h, size_t row_bytes, uint8_t* dst, int oh, const int32_t* bounds, const int32_t* coeffs, hipStream_t stream) {
    VerticalArgs a;
    a.src = src; a.dst = dst; a.bounds = bounds; a.coeffs = coeffs;
    a.h = h; a.oh = oh; a.ksize = wt::resize_ksize(h, oh); a.row_bytes = row_bytes;
    const size_t words = (row_bytes + 6) / 4;                    // the most aligned words a row touches
    const dim3 grid((unsigned)((words + kThreads - 1) / kThreads), (unsigned)oh);
    hipLaunchKernelGGL(resize_vertical_kernel, grid, dim3(kThreads), 0, stream, a);
}

}  // namespace

extern "C" int wd_resize_ksize(int in_size, int out_size) { return wt::resize_ksize(in_size, out_size); }

extern "C" int wd_resize_tables_host(int in_size, int out_size, int32_t* bounds, int32_t* coeffs) {
    return wt::resize_tables_checked("wd_resize_tables_host", in_size, out_size, bounds, coeffs);
}

extern "C" int wd_resize_bilinear_u8_host(const uint8_t* src, int h, int w, uint8_t* dst, int oh, int ow) {
    return wt::resize_bilinear_u8_cpu(src, h, w, dst, oh, ow);
}

extern "C" size_t wd_resize_bilinear_u8_workspace(int h, int w, int oh, int ow) { return wt::resize_workspace_bytes(h, w, oh, ow); }

extern "C" int wd_resize_bilinear_u8(const uint8_t* src, int h, int w, uint8_t* dst, int oh, int ow, const int32_t* xbounds, const int32_t* xcoeffs,
                                     const int32_t* ybounds, const int32_t* ycoeffs, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* entry = "wd_resize_bilinear_u8";
    WT_TRY(wt::check_resize_args(entry, src, h, w, dst, oh, ow));
    const bool horizontal = w != ow, vertical = h != oh;
    if (horizontal && (!xbounds || !xcoeffs)) { wt::set_error("%s: %s is null (w %d -> ow %d needs the horizontal tables)", entry, xbounds ? "xcoeffs" : "xbounds", w, ow); return WT_ERR_INVALID; }
    if (vertical && (!ybounds || !ycoeffs)) { wt::set_error("%s: %s is null (h %d -> oh %d needs the vertical tables)", entry, ybounds ? "ycoeffs" : "ybounds", h, oh); return WT_ERR_INVALID; }
    const size_t need = wt::resize_workspace_bytes(h, w, oh, ow);
    if (need && !workspace) { wt::set_error("%s: workspace is null, %zu bytes needed", entry, need); return WT_ERR_INVALID; }
    if (workspace_bytes < need) { wt::set_error("%s: workspace_bytes = %zu, %zu needed", entry, workspace_bytes, need); return WT_ERR_CAPACITY; }
    WT_TRY(wt::ensure_device());
    hipStream_t stream = (hipStream_t)stream_;
    if (!horizontal && !vertical) {
        WT_HIP(hipMemcpyAsync(dst, src, (size_t)h * w * 3, hipMemcpyDeviceToDevice, stream));
        return WT_OK;
    }
    const uint8_t* cur = src;
    if (horizontal) {
        uint8_t* out = vertical ? static_cast<uint8_t*>(workspace) : dst;
        WT_TRY(launch_horizontal(src, h, w, out, ow, xbounds, xcoeffs, stream));
        cur = out;
    }
    if (vertical) launch_vertical(cur, h, (size_t)ow * 3, dst, oh, ybounds, ycoeffs, stream);
    WT_HIP(hipGetLastError());
    return WT_OK;
}
