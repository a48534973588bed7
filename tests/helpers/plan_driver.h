// What the sanitizer drivers of the host-only plans (tests/helpers/*_plan_driver.cpp) share: the set_error the plan headers call,
// with the text kept in g_err, and the checks every driver makes of a plan -- a grid covers its items, the parts of a workspace
// lie one behind the other, a refusal names its entry and leaves a zero figure.  A driver includes its plan header, then this.
// Built with g++ only: no HIP in here.
#pragma once
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "slide_map_plan.h"

namespace gs {
static char g_err[1024];
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace gs
using namespace gs;

static inline int fail(const char *what, long long a, long long b, long long c = 0, long long d = 0)
{
    std::fprintf(stderr, "FAILED: %s (%lld, %lld, %lld, %lld): %s\n", what, a, b, c, d, g_err);
    return 1;
}

// covers(n, unit, total): n units of `unit` cover `total`, n - 1 do not
static inline bool covers(long long n, long long unit, long long total) { return n * unit >= total && (n - 1) * unit < total; }

// offs: the offsets of the parts of a workspace, the last one the size of the whole; need: the bytes of each part.  The parts lie
// one behind the other from 0: each aligned, large enough, with less than one alignment of slack.
template <int N>
static bool laid_out(const size_t (&offs)[N], const size_t (&need)[N - 1])
{
    for (int k = 0; k + 1 < N; ++k)
        if (offs[k] % kPlanAlign != 0 || offs[k + 1] < offs[k] + need[k] || offs[k + 1] >= offs[k] + need[k] + kPlanAlign)
            return false;
    return offs[0] == 0;
}

// a refusal: the status, `word` somewhere in the text, the entry's name in front of it, and a zero figure; clears the text
static inline bool refused(gs_status got, gs_status want, const char *word, const char *entry = "", size_t bytes = 0)
{
    const bool ok = got == want && std::strstr(g_err, word) && std::strstr(g_err, entry) == g_err && bytes == 0;
    g_err[0] = 0;
    return ok;
}

// the same with the plan itself, so that a call may plan and check in one expression: p.bytes is read after the plan has run
template <typename Plan>
static bool refused(gs_status got, gs_status want, const char *word, const char *entry, const Plan &p)
{
    return refused(got, want, word, entry, p.bytes);
}
