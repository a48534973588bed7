// Sanitizer driver (tests/test_boundary_dist_host.py) for the host-only plan of gs_instance_boundary_dist
// (csrc/boundary_dist_plan.h): sweeps the plan over edge sizes -- single pixels, a single row and column of the largest side,
// the largest map taken, one pixel beyond each limit -- and checks what the launcher relies on: the grids cover the map, the four
// tables are aligned, in order, large enough and inside the figure, refusals leave a text and a zero figure.  Built with g++
// only: no HIP in here.
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "boundary_dist_plan.h"

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

static int fail(const char *what, int h, int w)
{
    std::fprintf(stderr, "FAILED: %s (%d x %d): %s\n", what, h, w, g_err);
    return 1;
}

int main()
{
    const int sizes[] = {1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 517, 5000, 32767, 32768, 32769, 46340, 46341, 65535, 65536,
                         1 << 20, INT_MAX / 2, INT_MAX - 1, INT_MAX};
    const int bad[] = {0, -1, INT_MIN};
    int plans = 0, refused = 0;
    size_t largest = 0;
    for (int h : sizes)
        for (int w : sizes) {
            BoundaryDistPlan p;
            g_err[0] = 0;
            const gs_status st = plan_boundary_dist(h, w, p);
            if (h > 32768 || w > 32768 || (long long)h * w > (long long)INT_MAX) {
                if (st != GS_ERR_UNSUPPORTED || !g_err[0] || p.bytes != 0)
                    return fail("a map beyond 32768 pixels a side is not refused", h, w);
                ++refused;
                continue;
            }
            if (st != GS_OK)
                return fail("refused", h, w);
            ++plans;
            if (p.n_pixels != h * w)
                return fail("n_pixels", h, w);
            if ((long long)p.row_blocks * (kBdistThreads / 64) < 2ll * h || (long long)(p.row_blocks - 1) * (kBdistThreads / 64) >= 2ll * h)
                return fail("row_blocks", h, w);
            if ((long long)p.pixel_blocks * kBdistThreads < (long long)p.n_pixels ||
                (long long)(p.pixel_blocks - 1) * kBdistThreads >= (long long)p.n_pixels)
                return fail("pixel_blocks", h, w);
            const size_t offs[] = {p.left_gt_off, p.right_gt_off, p.left_pred_off, p.right_pred_off, p.bytes};
            for (int k = 0; k < 4; ++k)
                if (offs[k] % kBdistAlign != 0 || offs[k + 1] < offs[k] + (size_t)p.n_pixels * 2)
                    return fail("workspace layout", h, w);
            if (p.bytes > 4 * ((size_t)p.n_pixels * 2 + kBdistAlign))
                return fail("more workspace than four tables", h, w);
            if (p.bytes > largest)
                largest = p.bytes;
        }
    // 32768 x 32768 is 2^30 pixels: the largest map taken, 8 GiB of tables
    if (largest != ((size_t)8 << 30))
        return fail("the largest plan", 32768, 32768);
    // the distances: the largest d2 of the largest map fits an int32, that of a side one longer does not
    const long long far = 2ll * (kBdistMaxSide - 1) * (kBdistMaxSide - 1), beyond = 2ll * kBdistMaxSide * kBdistMaxSide;
    if (far >= (long long)INT_MAX || beyond <= (long long)INT_MAX || kBdistMaxSide - 1 >= kBdistNone)
        return fail("the int32 / uint16 bounds", kBdistMaxSide, kBdistMaxSide);
    for (int b : bad) {
        BoundaryDistPlan p;
        g_err[0] = 0;
        if (plan_boundary_dist(b, 10, p) != GS_ERR_INVALID || !g_err[0] || p.bytes != 0 || plan_boundary_dist(10, b, p) != GS_ERR_INVALID ||
            p.bytes != 0)
            return fail("a non-positive size is not refused", b, b);
        if (check_boundary_dist(b - (b == 0), 1) != GS_ERR_INVALID || check_boundary_dist(1, b - (b == 0)) != GS_ERR_INVALID)
            return fail("a negative count is not refused", b, b);
        ++refused;
    }
    if (check_boundary_dist(0, 0) != GS_OK || check_boundary_dist(INT_MAX, INT_MAX) != GS_OK)
        return fail("counts", 0, 0);
    std::printf("boundary dist plan ok: %d plans, %d refusals\n", plans, refused);
    return 0;
}
