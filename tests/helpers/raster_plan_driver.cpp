// Sanitizer driver (tests/helpers/sanitized_driver.py) for csrc/raster_plan.h, the host-only plan of gs_polygon_raster: size and
// count lists swept through the plan, and what the launcher relies on checked -- the grids cover their items in workgroups of
// kRasterThreads (no point grid without points, at least one feature and one word workgroup), the parts of the workspace are
// aligned, in order, large enough and inside the figure, the figure never shrinks with any argument, and refusals leave a text
// and a zero figure.  The two integer functions of the rule are compared with a plain search, and the box words with the
// header's formula.  Built with g++ only: no device code in here.
#include "raster_plan.h"
#include "plan_driver.h"

static const int kSizes[] = {1, 2, 63, 64, 65, 255, 256, 257, 517, 5000, 46340, 46341, 1 << 20, INT_MAX};
static const long long kCounts[] = {0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 28700, 1 << 20, (1ll << 31) - 2, (1ll << 31) - 1};

static const char kEntry[] = "gs_polygon_raster: ";

static bool grid_covers(int blocks, long long items, int least)
{
    if (items == 0)
        return blocks == least;
    return (long long)blocks * kRasterThreads >= items && ((long long)blocks - 1) * kRasterThreads < items;
}

int main()
{
    int plans = 0, refusals = 0;
    for (int h : kSizes)
        for (int w : {1, 2, h}) {
            const long long pixels = (long long)h * w;
            for (long long n : kCounts)
                for (long long cap : kCounts) {
                    RasterPlan p;
                    g_err[0] = 0;
                    const long long points = n, rings = n / 3, features = n / 2;
                    const gs_status st = plan_raster(h, w, points, rings, features, cap, p);
                    if (pixels > INT_MAX) {
                        if (!refused(st, GS_ERR_UNSUPPORTED, "pixels", kEntry, p))
                            return fail("a map of more than 2^31 - 1 pixels is not refused", h, w, cap);
                        ++refusals;
                        continue;
                    }
                    if (st != GS_OK || g_err[0])
                        return fail("refused", h, w, cap);
                    ++plans;
                    if (p.n_pixels != pixels || p.n_points != points || p.n_rings != rings || p.n_features != features || p.words_cap != cap)
                        return fail("sizes", h, w, cap);
                    if (!grid_covers(p.pixel_blocks, pixels, 0) || !grid_covers(p.point_blocks, points, 0) ||
                        !grid_covers(p.feature_blocks, features, 1) || !grid_covers(p.word_blocks, cap, 1))
                        return fail("grids", h, w, cap);
                    const size_t offs[] = {p.head_off, p.box_off, p.feature_front_off, p.block_words_off, p.feature_base_off, p.scratch_off, p.bytes};
                    const size_t need[] = {sizeof(RasterHead),       (size_t)features * sizeof(RasterBox), (size_t)features * 8,
                                           (size_t)p.feature_blocks * 8, (size_t)features * 4,             (size_t)cap * 4};
                    for (int k = 0; k < 6; ++k)
                        if (offs[k] % kPlanAlign != 0 || offs[k + 1] < offs[k] + need[k] || offs[k + 1] >= offs[k] + need[k] + kPlanAlign)
                            return fail("workspace layout", h, w, cap);
                    if (offs[0] != 0)
                        return fail("the head is not first", h, w, cap);
                    // never shrinks: one less of each argument in turn
                    RasterPlan q;
                    if (cap > 0 && (plan_raster(h, w, points, rings, features, cap - 1, q) != GS_OK || q.bytes > p.bytes))
                        return fail("the figure shrinks with words_cap", h, w, cap);
                    if (features > 0 && (plan_raster(h, w, points, rings, features - 1, cap, q) != GS_OK || q.bytes > p.bytes))
                        return fail("the figure shrinks with n_features", h, w, features);
                    if (points > 0 && (plan_raster(h, w, points - 1, rings, features, cap, q) != GS_OK || q.bytes > p.bytes))
                        return fail("the figure shrinks with n_points", h, w, points);
                    if (rings > 0 && (plan_raster(h, w, points, rings - 1, features, cap, q) != GS_OK || q.bytes > p.bytes))
                        return fail("the figure shrinks with n_rings", h, w, rings);
                    if (h > 1 && w == 1 && (plan_raster(h - 1, w, points, rings, features, cap, q) != GS_OK || q.bytes > p.bytes))
                        return fail("the figure shrinks with the map", h, w, cap);
                }
        }
    const int bad[] = {0, -1, INT_MIN};
    for (int b : bad) {
        RasterPlan p;
        if (!refused(plan_raster(b, 10, 1, 1, 1, 10, p), GS_ERR_INVALID, "positive", kEntry, p) ||
            !refused(plan_raster(10, b, 1, 1, 1, 10, p), GS_ERR_INVALID, "positive", kEntry, p))
            return fail("a non-positive side is not refused", b, b);
        ++refusals;
    }
    const long long bad_counts[] = {-1, -2, LLONG_MIN, 1ll << 31, 1ll << 40, LLONG_MAX};
    for (long long c : bad_counts) {
        RasterPlan p;
        if (!refused(plan_raster(10, 10, c, 1, 1, 10, p), GS_ERR_INVALID, "n_points", kEntry, p) ||
            !refused(plan_raster(10, 10, 1, c, 1, 10, p), GS_ERR_INVALID, "n_rings", kEntry, p) ||
            !refused(plan_raster(10, 10, 1, 1, c, 10, p), GS_ERR_INVALID, "n_features", kEntry, p) ||
            !refused(plan_raster(10, 10, 1, 1, 1, c, p), GS_ERR_INVALID, "words_cap", kEntry, p))
            return fail("a count out of range is not refused", c, 0);
        refusals += 4;
    }
    for (int f : {-1, 9, INT_MIN, INT_MAX}) {
        g_err[0] = 0;
        if (check_raster_frac_bits("gs_polygon_raster", f) != GS_ERR_INVALID || !std::strstr(g_err, "frac_bits"))
            return fail("frac_bits out of range is not refused", f, 0);
        ++refusals;
    }
    for (int f = 0; f <= kRasterMaxFracBits; ++f)
        if (check_raster_frac_bits("gs_polygon_raster", f) != GS_OK)
            return fail("frac_bits refused", f, 0);

    // the first pixel whose centre (2p + 1) S is at or beyond v, by a plain search
    for (long long S : {1ll, 2ll, 8ll, 256ll})
        for (long long v = -5 * S - 3; v <= 2 * S * 9 + 3; ++v) {
            const int limit = 7;
            int want = 0;
            while (want < limit && (2ll * want + 1) * S < v)
                ++want;
            if (raster_first_pixel(v, S, limit) != want)
                return fail("raster_first_pixel", v, S, want);
        }
    const long long far = 2ll * kRasterCoordMax;
    if (raster_first_pixel(far, 256, INT_MAX) != (1 << 20) || raster_first_pixel(-far, 256, INT_MAX) != 0 ||
        raster_first_pixel(far, 1, INT_MAX) != kRasterCoordMax || raster_first_pixel(far, 1, 5) != 5)
        return fail("raster_first_pixel at the clamp", far, 0);
    if (raster_ceil_div(7, 2) != 4 || raster_ceil_div(-7, 2) != -3 || raster_ceil_div(8, 2) != 4 || raster_ceil_div(-8, 2) != -4 ||
        raster_ceil_div(0, 5) != 0 || raster_ceil_div(-1, 5) != 0 || raster_ceil_div(1, 5) != 1)
        return fail("raster_ceil_div", 7, 2);
    if (raster_clamp_coord(INT_MAX) != kRasterCoordMax || raster_clamp_coord(INT_MIN) != -kRasterCoordMax || raster_clamp_coord(-5) != -5 ||
        raster_clamp_coord(kRasterCoordMax + 1) != kRasterCoordMax)
        return fail("raster_clamp_coord", 0, 0);
    const RasterBox empty = {INT_MAX, INT_MAX, INT_MIN, INT_MIN}, one = {3, 4, 3, 5}, wide = {0, 0, 32, 2}, flat = {0, 7, 31, 7};
    const RasterBox whole = {0, 0, INT_MAX, INT_MAX};
    if (raster_box_rows(empty) * raster_box_row_words(empty) != 0 || raster_box_rows(one) != 1 || raster_box_row_words(one) != 1 ||
        raster_box_row_words(wide) != 2 || raster_box_rows(wide) != 2 || raster_box_rows(flat) != 0 || raster_box_row_words(flat) != 1 ||
        raster_box_rows(whole) != INT_MAX || raster_box_row_words(whole) != (1 << 26))
        return fail("box words", 0, 0);
    std::printf("raster plan ok: %d plans, %d refusals\n", plans, refusals);
    return 0;
}
