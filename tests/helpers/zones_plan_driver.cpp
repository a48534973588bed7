// Sanitizer driver (tests/helpers/sanitized_driver.py) for csrc/zones_plan.h, the host-only plans of gs_instance_zones and
// gs_foreign_dist: sizes swept through both plans, and what the launchers rely on checked -- the grids cover their items (bands of
// kZoneBand rows, tiles and workgroups of kZoneThreads, a wave per row), the LDS figure holds a row up to kZoneLdsCols and is 0
// beyond, the parts of the workspace are aligned, in order, large enough and inside the figure, the figure never shrinks when a
// side grows, and refusals leave a text and a zero figure.  zone_isqrt is compared with a plain search and the cap check with its
// range.  Built with g++ only: no device code in here.
#include "zones_plan.h"
#include "plan_driver.h"

static const int kSizes[] = {1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513, 5000, 16383, 16384, 16385, 32767, 32768};

template <typename Plan, typename Fn>
static bool refused(Fn plan_fn, int h, int w, gs_status want, const char *word, const char *entry)
{
    Plan p;
    g_err[0] = 0;
    return refused(plan_fn(h, w, p), want, word, entry, p);
}

int main()
{
    int plans = 0, refusals = 0;
    for (int h : kSizes)
        for (int w : kSizes) {
            const long long pixels = (long long)h * w;
            ZonePlan z, zq;
            ForeignPlan f, fq;
            g_err[0] = 0;
            if (plan_zones(h, w, z) != GS_OK || plan_foreign(h, w, f) != GS_OK || g_err[0])
                return fail("refused", h, w);
            plans += 2;
            if (!covers(z.bands, kZoneBand, h) || !covers(z.col_tiles, kZoneThreads, w) || z.band_blocks != z.bands * z.col_tiles ||
                z.carry_blocks != z.col_tiles || !covers(z.pixel_blocks, kZoneThreads, pixels))
                return fail("zone grids", h, w);
            if (w <= kZoneLdsCols ? (z.row_lds_bytes < 2 * w || z.row_lds_bytes % 16 != 0 || z.row_lds_bytes > 2 * kZoneLdsCols)
                                  : z.row_lds_bytes != 0)
                return fail("row LDS", h, w);
            const size_t table = (size_t)z.bands * (size_t)w;
            const size_t zoffs[] = {z.g_off,    z.clab_off,  z.top_d_off,  z.bot_d_off, z.down_d_off, z.up_d_off,
                                    z.top_l_off, z.bot_l_off, z.down_l_off, z.up_l_off,  z.bytes};
            const size_t zneed[] = {(size_t)pixels * 2, (size_t)pixels * 4, table * 2, table * 2, table * 2,
                                    table * 2,          table * 4,          table * 4, table * 4, table * 4};
            if (!laid_out(zoffs, zneed))
                return fail("zone workspace layout", h, w);
            if (!covers(f.row_blocks, kZoneThreads / 64, h) || !covers(f.pixel_blocks, kZoneThreads, pixels))
                return fail("foreign grids", h, w);
            const size_t foffs[] = {f.left_off, f.right_off, f.bytes};
            const size_t fneed[] = {(size_t)pixels * 2, (size_t)pixels * 2};
            if (!laid_out(foffs, fneed))
                return fail("foreign workspace layout", h, w);
            // never shrinks: one less of each side in turn
            if (h > 1 && (plan_zones(h - 1, w, zq) != GS_OK || zq.bytes > z.bytes || plan_foreign(h - 1, w, fq) != GS_OK || fq.bytes > f.bytes))
                return fail("the figure shrinks with the height", h, w);
            if (w > 1 && (plan_zones(h, w - 1, zq) != GS_OK || zq.bytes > z.bytes || plan_foreign(h, w - 1, fq) != GS_OK || fq.bytes > f.bytes))
                return fail("the figure shrinks with the width", h, w);
        }
    const auto pz = [](int h, int w, ZonePlan &p) { return plan_zones(h, w, p); };
    const auto pf = [](int h, int w, ForeignPlan &p) { return plan_foreign(h, w, p); };
    for (int b : {0, -1, INT_MIN}) {
        if (!refused<ZonePlan>(pz, b, 10, GS_ERR_INVALID, "positive", "gs_instance_zones: ") ||
            !refused<ZonePlan>(pz, 10, b, GS_ERR_INVALID, "positive", "gs_instance_zones: ") ||
            !refused<ForeignPlan>(pf, b, 10, GS_ERR_INVALID, "positive", "gs_foreign_dist: ") ||
            !refused<ForeignPlan>(pf, 10, b, GS_ERR_INVALID, "positive", "gs_foreign_dist: "))
            return fail("a non-positive side is not refused", b, b);
        refusals += 4;
    }
    for (int b : {32769, 46341, 1 << 20, INT_MAX}) {
        if (!refused<ZonePlan>(pz, b, 1, GS_ERR_UNSUPPORTED, "side above", "gs_instance_zones: ") ||
            !refused<ZonePlan>(pz, 1, b, GS_ERR_UNSUPPORTED, "side above", "gs_instance_zones: ") ||
            !refused<ForeignPlan>(pf, b, 1, GS_ERR_UNSUPPORTED, "side above", "gs_foreign_dist: ") ||
            !refused<ForeignPlan>(pf, 1, b, GS_ERR_UNSUPPORTED, "side above", "gs_foreign_dist: "))
            return fail("a side above 32768 is not refused", b, b);
        refusals += 4;
    }
    // (32768 x 32768 is 2^30 pixels: inside both limits, and planned above)
    for (long long v : {0ll, 1ll, 400ll, (1ll << 30) - 1, 1ll << 30}) {
        g_err[0] = 0;
        if (check_zone_cap("gs_instance_zones", v) != GS_OK || g_err[0])
            return fail("max_d2 refused", v, 0);
    }
    for (long long v : {-1ll, (long long)INT_MIN, (1ll << 30) + 1, (long long)INT_MAX, LLONG_MAX, LLONG_MIN}) {
        g_err[0] = 0;
        if (check_zone_cap("gs_foreign_dist", v) != GS_ERR_INVALID || !std::strstr(g_err, "max_d2") || !std::strstr(g_err, "gs_foreign_dist: "))
            return fail("max_d2 out of range is not refused", v, 0);
        ++refusals;
    }
    for (int n : {0, 1, INT_MAX})
        if (check_zone_count("gs_instance_zones", n) != GS_OK)
            return fail("n refused", n, 0);
    for (int n : {-1, INT_MIN}) {
        g_err[0] = 0;
        if (check_zone_count("gs_instance_zones", n) != GS_ERR_INVALID || !std::strstr(g_err, "negative"))
            return fail("a negative n is not refused", n, 0);
        ++refusals;
    }
    // floor(sqrt(v)) by a plain search, around every square up to 300^2 and at the far end
    int want = 0;
    for (int v = 0; v <= 90000; ++v) {
        while ((want + 1) * (want + 1) <= v)
            ++want;
        if (zone_isqrt(v) != want)
            return fail("zone_isqrt", v, want);
    }
    for (long long r : {1000ll, 16384ll, 23170ll, 32767ll, 32768ll})
        for (long long d : {-1ll, 0ll, 1ll}) {
            const long long v = r * r + d;
            if (v > kZoneMaxD2)
                continue;
            if (zone_isqrt((int)v) != (d < 0 ? r - 1 : r))
                return fail("zone_isqrt at the far end", v, r);
        }
    std::printf("zones plan ok: %d plans, %d refusals\n", plans, refusals);
    return 0;
}
