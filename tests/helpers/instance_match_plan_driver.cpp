// Sanitizer driver (tests/test_instance_match_host.py) for the host-only plan of gs_instance_overlaps / gs_instance_match
// (csrc/instance_match_plan.h): sweeps the plan over edge sizes -- single pixels, the largest maps taken, pair_cap 1 and
// INT_MAX -- and checks what the launcher relies on: the table is a power of two of at least 2 * cap slots, the parts of the
// workspace are aligned, in order and inside the figure, refusals leave a text.  Built with g++ only: no HIP in here.
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "instance_match_plan.h"

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

static int fail(const char *what, int h, int w, int cap)
{
    std::fprintf(stderr, "FAILED: %s (%d x %d, pair_cap %d): %s\n", what, h, w, cap, g_err);
    return 1;
}

int main()
{
    const int sizes[] = {1, 2, 3, 63, 64, 65, 255, 256, 257, 300, 517, 5000, 46340, 46341, 65536, 1 << 20, INT_MAX / 2, INT_MAX - 1, INT_MAX};
    const int caps[] = {1, 2, 127, 128, 129, 4096, 4097, 1 << 20, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, INT_MAX - 1, INT_MAX};
    const int bad[] = {0, -1, INT_MIN};
    int plans = 0, refused = 0;
    for (int h : sizes)
        for (int w : sizes)
            for (int cap : caps) {
                InstanceMatchPlan p;
                g_err[0] = 0;
                const gs_status st = plan_instance_match(h, w, cap, p);
                if ((long long)h * w > (long long)INT_MAX) {
                    if (st != GS_ERR_UNSUPPORTED || !g_err[0] || p.bytes != 0)
                        return fail("a map beyond 2^31 - 1 pixels is not refused", h, w, cap);
                    ++refused;
                    continue;
                }
                if (st != GS_OK)
                    return fail("refused", h, w, cap);
                ++plans;
                const size_t want_cap = (long long)cap < (long long)h * w ? (size_t)cap : (size_t)h * (size_t)w;
                if (p.n_pixels != h * w || (size_t)p.cap != want_cap)
                    return fail("cap", h, w, cap);
                if ((long long)p.tiles_x * kMatchTileW < w || (long long)(p.tiles_x - 1) * kMatchTileW >= w ||
                    (long long)p.tiles_y * kMatchTileH < h || (long long)(p.tiles_y - 1) * kMatchTileH >= h ||
                    (long long)p.tiles_x * p.tiles_y > (long long)p.n_pixels)
                    return fail("tiles", h, w, cap);
                if (p.slots < kMatchMinSlots || (p.slots & (p.slots - 1)) != 0 || p.slots < 2 * (size_t)p.cap || p.slots > ((size_t)1 << 32))
                    return fail("slots", h, w, cap);
                if (p.slots > kMatchMinSlots && p.slots / 2 >= 2 * (size_t)p.cap)
                    return fail("slots: more than twice what is needed", h, w, cap);
                if ((size_t)p.n_blocks * kMatchThreads != p.slots)
                    return fail("n_blocks", h, w, cap);
                const size_t offs[] = {p.state_off, p.key_off, p.val_off, p.block_off, p.dense_key_off, p.dense_slot_off, p.bytes};
                const size_t need[] = {16, p.slots * 8, p.slots * 16, (size_t)p.n_blocks * 4, (size_t)p.cap * 8, (size_t)p.cap * 4};
                for (int k = 0; k < 6; ++k)
                    if (offs[k] % kMatchAlign != 0 || offs[k + 1] < offs[k] + need[k])
                        return fail("workspace layout", h, w, cap);
            }
    for (int b : bad) {
        InstanceMatchPlan p;
        g_err[0] = 0;
        if (plan_instance_match(b, 10, 10, p) != GS_ERR_INVALID || !g_err[0] || plan_instance_match(10, b, 10, p) != GS_ERR_INVALID ||
            plan_instance_match(10, 10, b, p) != GS_ERR_INVALID || p.bytes != 0)
            return fail("a non-positive size is not refused", b, b, b);
        if (check_instance_match(b, 1, 1, 5, 1, 2) != GS_ERR_INVALID || check_instance_match(1, b - (b == 0), 1, 5, 1, 2) != GS_ERR_INVALID)
            return fail("gs_instance_match's numbers", b, b, b);
        ++refused;
    }
    // thresholds: every num / den up to 300 and the edges of the range
    int thresholds = 0;
    for (int den = -1; den <= 300; ++den)
        for (int num = -1; num <= 301; ++num) {
            const bool ok = num >= 1 && num <= den && 2 * num >= den;
            if ((check_instance_match(1, 0, 0, 5, num, den) == GS_OK) != ok)
                return fail("threshold", num, den, 0);
            thresholds += ok;
        }
    const int edge[][3] = {{65535, 65535, 1}, {32768, 65535, 1}, {32767, 65535, 0}, {65536, 65536, 0}, {32768, 65536, 0}, {INT_MAX, INT_MAX, 0},
                           {INT_MAX / 2 + 1, INT_MAX, 0}, {INT_MIN, INT_MIN, 0}, {1, INT_MIN, 0}};
    for (const auto &e : edge)
        if ((check_instance_match(1, 0, 0, 5, e[0], e[1]) == GS_OK) != (e[2] != 0))
            return fail("threshold edge", e[0], e[1], 0);
    std::printf("instance match plan ok: %d plans, %d refusals, %d thresholds\n", plans, refused, thresholds);
    return 0;
}
