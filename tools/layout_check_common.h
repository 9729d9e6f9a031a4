// What the five tools/*_layout_check.cpp share: the two functions of the library that the host headers call, kept in the program
// itself so that no device is needed, and the harness that feeds a check one input and compares what it gave.
// Include it after the stage's csrc/*_host.h.
#pragma once
#include <cmath>
#include <string>

namespace wt {
static char g_error[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
int hip_fail(hipError_t, const char* what) { set_error("%s", what); return WT_ERR_HIP; }
}  // namespace wt

namespace {

int failures = 0;

void report(const char* name, int rc, bool ok) {
    printf("%-34s rc %d  %s%s\n", name, rc, wt::g_error, ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

// check(in) must answer `want`: with the totals of the shared valid layout (largest count 2, sum 6) when that is WT_OK, with
// `text` in the error otherwise
template <class Input>
void expect_input(const char* name, const Input& in, int (*check)(const Input&, int64_t*, int64_t*), int want, const char* text) {
    int64_t max_traj = -1, total = -1;
    wt::g_error[0] = 0;
    const int rc = check(in, &max_traj, &total);
    report(name, rc, rc == want && (want == WT_OK ? (max_traj == 2 && total == 6) : std::string(wt::g_error).find(text) != std::string::npos));
}

int summary() {
    printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}

}  // namespace
