// The host layer of the PIL-exact bilinear resize (csrc/resize_host.h) as a program of its own, for a host sanitizer:
//
//     g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -g -O1 tools/resize_check.cpp -o resize_check && ./resize_check
//
// It runs the CPU form of the resize over the shapes of tests/resize_cases.py (every buffer a heap block of exactly its size, so that
// one byte outside is a report), checks what needs no second implementation (all-0 stays 0, all-255 stays 255, equal sizes copy, every
// table window lies inside its source and its table row, 255 * sum(k) < 2^31), then feeds the two passes tables whose bounds are
// deliberately wrong - in front of the source, behind it, longer than ksize, negative - which resize_clamp_window must turn into wrong
// pixels and nothing else, and the entry points sizes and pointers they must refuse by name.  It prints one line per case and returns
// 0 when nothing was unexpected.  Equality with PIL is tests/test_resize_cases.py; no device is touched.
#include "../waymo_2d_tracking_amd/csrc/resize_host.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace wt {
static char g_error[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
}  // namespace wt

namespace {

int failures = 0;

void report(const std::string& name, bool ok, const std::string& what) {
    printf("%-44s %s%s\n", name.c_str(), what.c_str(), ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

struct Block {                                  // a heap block of exactly n bytes (n = 0: one byte that nobody may touch)
    uint8_t* p;
    size_t n;
    explicit Block(size_t bytes) : p(static_cast<uint8_t*>(malloc(bytes ? bytes : 1))), n(bytes) {}
    Block(const Block&) = delete;
    ~Block() { free(p); }
};

uint32_t checksum(const uint8_t* p, size_t n) {          // FNV-1a
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

void fill(Block& b, int w, int content) {
    uint32_t s = 12345u + (uint32_t)b.n;
    for (size_t i = 0; i < b.n; ++i) {
        s = s * 1664525u + 1013904223u;
        const size_t pix = i / 3;
        b.p[i] = content == 0 ? (uint8_t)(s >> 24) : content == 1 ? 0 : content == 2 ? 255 : (uint8_t)((((pix / w) + (pix % w)) & 1) * 255);
    }
}

bool tables_inside(int in_size, int out_size) {
    const int ksize = wt::resize_ksize(in_size, out_size);
    std::vector<int32_t> bounds((size_t)out_size * 2), coeffs((size_t)out_size * ksize);
    std::vector<double> weights;
    wt::resize_build_tables(in_size, out_size, bounds.data(), coeffs.data(), weights);
    for (int xx = 0; xx < out_size; ++xx) {
        const int first = bounds[2 * xx], count = bounds[2 * xx + 1];
        int64_t sum = 0;
        for (int x = 0; x < ksize; ++x) {
            const int32_t k = coeffs[(size_t)xx * ksize + x];
            if (k < 0 || (x >= count && k != 0)) return false;
            sum += k;
        }
        if (first < 0 || count < 1 || count > ksize || first + count > in_size || 255 * sum >= (1ll << 31)) return false;
    }
    return true;
}

void shape_case(int h, int w, int oh, int ow) {
    char name[64];
    snprintf(name, sizeof(name), "%dx%d -> %dx%d", h, w, oh, ow);
    bool ok = (w == ow || tables_inside(w, ow)) && (h == oh || tables_inside(h, oh));
    std::string sums;
    for (int content = 0; content < 4; ++content) {
        Block src((size_t)h * w * 3), dst((size_t)oh * ow * 3);
        fill(src, w, content);
        memset(dst.p, 0x5A, dst.n);
        const int rc = wt::resize_bilinear_u8_cpu(src.p, h, w, dst.p, oh, ow);
        ok = ok && rc == WT_OK;
        if (content == 1 || content == 2)
            for (size_t i = 0; i < dst.n; ++i) ok = ok && dst.p[i] == (content == 1 ? 0 : 255);
        if (h == oh && w == ow) ok = ok && memcmp(src.p, dst.p, dst.n) == 0;
        char buf[16];
        snprintf(buf, sizeof(buf), " %08x", checksum(dst.p, dst.n));
        sums += buf;
    }
    report(name, ok, "ksize " + std::to_string(wt::resize_ksize(w, ow)) + " x " + std::to_string(wt::resize_ksize(h, oh)) + "  random / 0 / 255 / checker:" + sums);
}

// both passes of h x w -> oh x ow with the bounds of every output index replaced by (first(i), count(i))
void wrong_tables(const char* name, int h, int w, int oh, int ow, int (*first)(int i, int in_size, int right), int (*count)(int i, int ksize, int right)) {
    const int kx = wt::resize_ksize(w, ow), ky = wt::resize_ksize(h, oh);
    std::vector<double> weights;
    // the tables live in exact heap blocks too: a window longer than ksize would read behind a table row's end
    Block xb((size_t)ow * 2 * 4), xc((size_t)ow * kx * 4), yb((size_t)oh * 2 * 4), yc((size_t)oh * ky * 4);
    int32_t *xbounds = reinterpret_cast<int32_t*>(xb.p), *xcoeffs = reinterpret_cast<int32_t*>(xc.p);
    int32_t *ybounds = reinterpret_cast<int32_t*>(yb.p), *ycoeffs = reinterpret_cast<int32_t*>(yc.p);
    wt::resize_build_tables(w, ow, xbounds, xcoeffs, weights);
    wt::resize_build_tables(h, oh, ybounds, ycoeffs, weights);
    for (int i = 0; i < ow; ++i) { const int f = xbounds[2 * i], c = xbounds[2 * i + 1]; xbounds[2 * i] = first(i, w, f); xbounds[2 * i + 1] = count(i, kx, c); }
    for (int i = 0; i < oh; ++i) { const int f = ybounds[2 * i], c = ybounds[2 * i + 1]; ybounds[2 * i] = first(i, h, f); ybounds[2 * i + 1] = count(i, ky, c); }
    Block src((size_t)h * w * 3), mid((size_t)h * ow * 3), dst((size_t)oh * ow * 3);
    fill(src, w, 0);
    wt::resize_pass_horizontal(src.p, h, w, mid.p, ow, xbounds, xcoeffs, kx);
    wt::resize_pass_vertical(mid.p, h, (size_t)ow * 3, dst.p, oh, ybounds, ycoeffs, ky);
    char what[64];
    snprintf(what, sizeof(what), "ran, checksum %08x", checksum(dst.p, dst.n));
    report(name, true, what);                                  // what is unexpected here is a sanitizer report
}

void refusal(const char* name, int rc, int want, const char* text) {
    report(name, rc == want && std::string(wt::g_error).find(text) != std::string::npos, "rc " + std::to_string(rc) + "  " + wt::g_error);
}

}  // namespace

int main() {
    static const int shapes[][4] = {
        {1, 1, 1, 1}, {1, 1, 5, 7}, {7, 5, 1, 1}, {3, 300, 2, 2}, {300, 3, 2, 2}, {2, 2, 3, 300}, {64, 64, 64, 64}, {40, 63, 40, 31}, {40, 64, 40, 32},
        {40, 65, 40, 33}, {40, 257, 40, 129}, {63, 40, 31, 40}, {65, 40, 97, 40}, {48, 72, 32, 48}, {48, 72, 72, 108}, {61, 91, 30, 45}, {96, 130, 37, 50},
        {33, 1025, 33, 64}, {1025, 33, 64, 33}, {20, 30, 19, 29}, {20, 30, 21, 31}, {128, 192, 80, 120},
        {2, 16384, 1, 1}, {16384, 2, 1, 3}, {1, 1, 2, 16384}};          // and the limits
    for (const auto& s : shapes) shape_case(s[0], s[1], s[2], s[3]);

    const auto keep_first = [](int, int, int right) { return right; };
    const auto keep_count = [](int, int, int right) { return right; };
    wrong_tables("wrong: first in front of the source", 61, 91, 30, 45, [](int i, int, int) { return -1 - i; }, keep_count);
    wrong_tables("wrong: first behind the source", 61, 91, 30, 45, [](int i, int n, int) { return n + i; }, keep_count);
    wrong_tables("wrong: first = in_size - 1, count kept", 61, 91, 30, 45, [](int, int n, int) { return n - 1; }, keep_count);
    wrong_tables("wrong: count longer than ksize", 61, 91, 30, 45, keep_first, [](int i, int k, int) { return k + 1 + i; });
    wrong_tables("wrong: count 2^30", 61, 91, 30, 45, keep_first, [](int, int, int) { return 1 << 30; });
    wrong_tables("wrong: count negative", 61, 91, 30, 45, keep_first, [](int, int, int) { return -3; });
    wrong_tables("wrong: INT_MIN first, INT_MAX count", 33, 1025, 33, 64 + 1, [](int, int, int) { return INT32_MIN; }, [](int, int, int) { return INT32_MAX; });
    wrong_tables("wrong: INT_MAX first, INT_MIN count", 96, 130, 37, 50, [](int, int, int) { return INT32_MAX; }, [](int, int, int) { return INT32_MIN; });
    wrong_tables("wrong: windows descend", 48, 72, 72, 108, [](int i, int n, int) { return n - 1 - i % n; }, keep_count);

    int32_t slot[64];
    uint8_t px[64] = {};
    refusal("refuse: in_size 0", wt::resize_tables_checked("tables", 0, 4, slot, slot), WT_ERR_INVALID, "in_size = 0");
    refusal("refuse: out_size 16385", wt::resize_tables_checked("tables", 4, 16385, slot, slot), WT_ERR_INVALID, "out_size = 16385");
    refusal("refuse: bounds null", wt::resize_tables_checked("tables", 4, 2, nullptr, slot), WT_ERR_INVALID, "bounds is null");
    refusal("refuse: coeffs null", wt::resize_tables_checked("tables", 4, 2, slot, nullptr), WT_ERR_INVALID, "coeffs is null");
    refusal("refuse: h 0", wt::resize_bilinear_u8_cpu(px, 0, 4, px, 2, 2), WT_ERR_INVALID, "h = 0");
    refusal("refuse: ow 16385", wt::resize_bilinear_u8_cpu(px, 4, 4, px, 2, 16385), WT_ERR_INVALID, "ow = 16385");
    refusal("refuse: src null", wt::resize_bilinear_u8_cpu(nullptr, 4, 4, px, 2, 2), WT_ERR_INVALID, "src is null");
    refusal("refuse: dst null", wt::resize_bilinear_u8_cpu(px, 4, 4, nullptr, 2, 2), WT_ERR_INVALID, "dst is null");
    report("ksize outside the limits is 0", wt::resize_ksize(0, 4) == 0 && wt::resize_ksize(4, 16385) == 0 && wt::resize_ksize(16384, 1) == 32769, "");
    report("workspace", wt::resize_workspace_bytes(4, 4, 2, 2) == 24 && wt::resize_workspace_bytes(4, 4, 4, 2) == 0 && wt::resize_workspace_bytes(4, 4, 2, 4) == 0, "");
    printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
