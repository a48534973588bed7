// Sanitizer driver (tests/helpers/sanitized_driver.py) for csrc/morphometry_plan.h, the host-only plan of gs_instance_morphometry:
// a size list and a rows_cap list swept through the plan, and what the launcher relies on checked -- the window grid covers the
// (height + 1) x (width + 1) windows in tiles of 256 x kMorphRows, the stride grid is 1..kMorphMaxGrid, the parts of the workspace are aligned, in order, large
// enough and inside the figure, the figure never shrinks with rows_cap and does not depend on the map, refusals leave a text and
// a zero figure, and the tiles and tasks of an instance cover its candidates.  Built with g++ only: no HIP in here.
#include "morphometry_plan.h"
#include "plan_driver.h"

static const int kSizes[] = {1, 2, 3, 63, 64, 65, 255, 256, 257, 300, 517, 5000, 32767, 32768, 32769, 46341, 65536, 1 << 20, INT_MAX};
static const long long kCaps[] = {0, 1, 2, 5, 6, 255, 256, 1023, 1024, 1025, 28700, 1 << 20, (1ll << 31) - 1, 1ll << 31, 1ll << 40,
                                  kMorphMaxRows - 1, kMorphMaxRows, kMorphMaxRows + 1, LLONG_MAX};

static const char kEntry[] = "gs_instance_morphometry: ";

int main()
{
    int plans = 0, refusals = 0;
    for (int h : kSizes)
        for (int w : kSizes) {
            size_t before = 0;
            for (long long cap : kCaps) {
                MorphometryPlan p;
                g_err[0] = 0;
                const gs_status st = plan_morphometry(h, w, cap, p);
                if (h > kMorphMaxSide || w > kMorphMaxSide) {        // the side limit comes first, whatever the number of pixels
                    if (!refused(st, GS_ERR_UNSUPPORTED, "32768", kEntry, p))
                        return fail("a map beyond 32768 pixels a side is not refused", h, w, cap);
                    ++refusals;
                    continue;
                }
                if (st != GS_OK || g_err[0])
                    return fail("refused", h, w, cap);
                ++plans;
                const long long tiles_x = w / kMorphThreads + 1, tiles_y = p.window_blocks / tiles_x;      // the launcher's split
                if (tiles_x * tiles_y != p.window_blocks || tiles_x * kMorphThreads < w + 1ll || (tiles_x - 1) * kMorphThreads >= w + 1ll ||
                    tiles_y * kMorphRows < h + 1ll || (tiles_y - 1) * kMorphRows >= h + 1ll)
                    return fail("window grid", h, w, cap);
                if (p.stride_blocks < 1 || p.stride_blocks > kMorphMaxGrid || (cap >= kMorphMaxGrid && p.stride_blocks != kMorphMaxGrid))
                    return fail("stride grid", h, w, cap);
                if (p.rows_cap != (cap < kMorphMaxRows ? cap : kMorphMaxRows))
                    return fail("rows_cap", h, w, cap);
                const size_t offs[] = {p.head_off, p.slot_off, p.rows_off, p.bytes};
                const size_t need[] = {sizeof(MorphHead), (size_t)p.rows_cap * sizeof(MorphSlot), (size_t)p.rows_cap * 8};
                for (int k = 0; k < 3; ++k)
                    if (offs[k] % kPlanAlign != 0 || offs[k + 1] < offs[k] + need[k] || offs[k + 1] >= offs[k] + need[k] + kPlanAlign)
                        return fail("workspace layout", h, w, cap);
                if (offs[0] != 0 || p.bytes < before)
                    return fail("the figure shrinks with rows_cap", h, w, cap);
                before = p.bytes;
                MorphometryPlan q;
                if (plan_morphometry(1, 1, cap, q) != GS_OK || q.bytes != p.bytes)       // never shrinks with the map: it is constant
                    return fail("the figure depends on the map", h, w, cap);
            }
        }
    const int bad[] = {0, -1, INT_MIN};
    for (int b : bad) {
        MorphometryPlan p;
        if (!refused(plan_morphometry(b, 10, 10, p), GS_ERR_INVALID, "positive", kEntry, p) ||
            !refused(plan_morphometry(10, b, 10, p), GS_ERR_INVALID, "positive", kEntry, p))
            return fail("a non-positive side is not refused", b, b);
        ++refusals;
    }
    const long long bad_caps[] = {-1, -2, LLONG_MIN};
    for (long long c : bad_caps) {
        MorphometryPlan p;
        if (!refused(plan_morphometry(10, 10, c, p), GS_ERR_INVALID, "rows_cap", kEntry, p))
            return fail("a negative rows_cap is not refused", c, 0);
        ++refusals;
    }
    // 46341^2 > INT_MAX pixels lies behind the side limit: both refusals are GS_ERR_UNSUPPORTED
    MorphometryPlan p;
    if (!refused(plan_morphometry(46341, 46341, 1, p), GS_ERR_UNSUPPORTED, "32768", kEntry, p))
        return fail("46341 x 46341", 46341, 46341);
    // the diameter: the largest feret2 of the largest map fits an int32 and packs into x | y << 16; one side longer does not
    const long long far = 2ll * (kMorphMaxSide - 1) * (kMorphMaxSide - 1), beyond = 2ll * kMorphMaxSide * kMorphMaxSide;
    if (far >= (long long)INT_MAX || beyond <= (long long)INT_MAX || kMorphMaxSide - 1 > 0x7FFF)
        return fail("the int32 bounds", kMorphMaxSide, 0);
    // tiles and tasks: the tiles cover 2 * height candidates, the tasks are the pairs (a, b >= a)
    for (int h = 1; h <= kMorphMaxSide; h = h < 600 ? h + 1 : h * 2) {
        const long long t = morph_tiles(h);
        if (t * kMorphTile < 2ll * h || (t - 1) * kMorphTile >= 2ll * h || morph_tasks(h) != t * (t + 1) / 2 || t > 256)
            return fail("tiles", h, t);
    }
    if (morph_tiles(kMorphMaxSide) != 256 || morph_tasks(kMorphMaxSide) != 32896 || morph_tiles(128) != 1 || morph_tiles(129) != 2)
        return fail("tiles of the largest box", kMorphMaxSide, 0);
    std::printf("morphometry plan ok: %d plans, %d refusals\n", plans, refusals);
    return 0;
}
