// Sanitizer driver (tests/helpers/sanitized_driver.py) for the host-only plans of the slide-map analyses -- csrc/slide_map_plan.h
// and the three headers built on it: instance_plan.h, instance_match_plan.h, boundary_dist_plan.h.  One size list -- single
// pixels, a single row and column of the largest side, the largest maps taken, one pixel beyond each limit -- swept through every
// plan, and what the launchers rely on checked: grids and tiles cover the map, the parts of a workspace are aligned, in order,
// large enough and inside the figure, refusals leave a text and a zero figure.  Built with g++ only: no HIP in here.
#include "boundary_dist_plan.h"
#include "instance_match_plan.h"
#include "instance_plan.h"
#include "plan_driver.h"

static const int kSizes[] = {1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 517, 5000, 32767, 32768, 32769, 46340, 46341, 65535, 65536,
                             1 << 20, INT_MAX / 2, INT_MAX - 1, INT_MAX};
static const int kBad[] = {0, -1, INT_MIN};

// ---- slide_map_plan.h itself
static int shared_checks()
{
    int n = 0;
    for (int h : kSizes)
        for (int w : kSizes) {
            g_err[0] = 0;
            if (check_map_sides("e", h, w) != GS_OK || g_err[0])
                return fail("positive sides refused", h, w);
            const bool fits = (long long)h * w <= (long long)INT_MAX;
            if (fits ? check_map_pixels("e", h, w) != GS_OK || g_err[0] : !refused(check_map_pixels("e", h, w), GS_ERR_UNSUPPORTED, "e: "))
                return fail("check_map_pixels", h, w);
            ++n;
        }
    for (int b : kBad) {
        if (!refused(check_map_sides("e", b, 10), GS_ERR_INVALID, "e: ") || !refused(check_map_sides("e", 10, b), GS_ERR_INVALID, "positive"))
            return fail("check_map_sides", b, b);
        if (!refused(check_instance_counts("e", b - (b == 0), 1), GS_ERR_INVALID, "e: ") ||
            !refused(check_instance_counts("e", 1, b - (b == 0)), GS_ERR_INVALID, "negative"))
            return fail("check_instance_counts", b, b);
        if (!refused(check_map_classes("e", b), GS_ERR_INVALID, "classes"))
            return fail("check_map_classes", b, 0);
    }
    if (check_instance_counts("e", 0, 0) != GS_OK || check_instance_counts("e", INT_MAX, INT_MAX) != GS_OK)
        return fail("counts", 0, 0);
    for (int c = -2; c <= GS_MAX_CLASSES + 2; ++c)
        if ((check_map_classes("e", c) == GS_OK) != (c >= 2 && c <= GS_MAX_CLASSES))
            return fail("check_map_classes", c, 0);
    if (!refused(check_map_classes("e", INT_MAX), GS_ERR_INVALID, "e: "))
        return fail("check_map_classes", INT_MAX, 0);
    // the cursor: every offset aligned, the parts in order, a part of 0 bytes takes none, sizes near 2^35 do not wrap
    const size_t parts[] = {0, 1, 255, 256, 257, 16, (size_t)INT_MAX * 4, 0, ((size_t)1 << 35) + 1, 3};
    size_t offs[11];
    PlanCursor ws;
    for (int k = 0; k < 10; ++k)
        offs[k] = ws.take(parts[k]);
    offs[10] = ws.off;
    if (!laid_out(offs, parts) || offs[1] != 0 || offs[2] != 256 || offs[5] - offs[4] != 512 || plan_align(0) != 0 || plan_align(257) != 512)
        return fail("PlanCursor", 0, 0);
    std::printf("shared checks ok: %d sizes\n", n);
    return 0;
}

// ---- instance_plan.h
static int instance_plans()
{
    const int caps[] = {1, 2, 4096, INT_MAX};
    int plans = 0, refusals = 0;
    for (int h : kSizes)
        for (int w : kSizes)
            for (int cap : caps) {
                InstancePlan p;
                g_err[0] = 0;
                const gs_status st = plan_instances(h, w, 5, cap, p);
                if ((long long)h * w > (long long)INT_MAX) {
                    if (!refused(st, GS_ERR_UNSUPPORTED, "2^31 - 1", "gs_slide_instances: ", p))
                        return fail("a map beyond 2^31 - 1 pixels is not refused", h, w, cap);
                    ++refusals;
                    continue;
                }
                if (st != GS_OK)
                    return fail("refused", h, w, cap);
                ++plans;
                if (p.n_pixels != h * w || !covers(p.tiles_x, kInstTileW, w) || !covers(p.tiles_y, kInstTileH, h) ||
                    !covers(p.n_blocks, kInstThreads, p.n_pixels))
                    return fail("tiles and blocks", h, w, cap);
                const size_t offs[] = {p.parent_off, p.block_off, p.bytes}, need[] = {(size_t)p.n_pixels * 4, (size_t)p.n_blocks * 4};
                if (!laid_out(offs, need))
                    return fail("workspace layout", h, w, cap);
            }
    InstancePlan p;
    if (plan_instances(1, INT_MAX, 5, 1, p) != GS_OK || p.n_blocks != (1 << 23) || p.bytes < (size_t)INT_MAX * 4)
        return fail("the largest plan", 1, INT_MAX);
    for (int b : kBad) {
        if (!refused(plan_instances(b, 10, 5, 10, p), GS_ERR_INVALID, "positive") || p.bytes != 0 ||
            !refused(plan_instances(10, b, 5, 10, p), GS_ERR_INVALID, "gs_slide_instances: ") || p.bytes != 0 ||
            !refused(plan_instances(10, 10, b, 10, p), GS_ERR_INVALID, "classes") || p.bytes != 0 ||
            !refused(plan_instances(10, 10, 5, b, p), GS_ERR_INVALID, "cap") || p.bytes != 0)
            return fail("a non-positive size is not refused", b, b, b);
        ++refusals;
    }
    if (!refused(plan_instances(10, 10, GS_MAX_CLASSES + 1, 10, p), GS_ERR_INVALID, "classes") || p.bytes != 0 ||
        plan_instances(10, 10, GS_MAX_CLASSES, 10, p) != GS_OK || plan_instances(10, 10, 2, 10, p) != GS_OK)
        return fail("the class range", GS_MAX_CLASSES, 0);
    std::printf("instance plan ok: %d plans, %d refusals\n", plans, refusals);
    return 0;
}

// ---- instance_match_plan.h
static int match_plans()
{
    const int caps[] = {1, 2, 127, 128, 129, 4096, 4097, 1 << 20, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, INT_MAX - 1, INT_MAX};
    int plans = 0, refusals = 0;
    for (int h : kSizes)
        for (int w : kSizes)
            for (int cap : caps) {
                InstanceMatchPlan p;
                g_err[0] = 0;
                const gs_status st = plan_instance_match(h, w, cap, p);
                if ((long long)h * w > (long long)INT_MAX) {
                    if (!refused(st, GS_ERR_UNSUPPORTED, "2^31 - 1", "gs_instance_overlaps: ", p))
                        return fail("a map beyond 2^31 - 1 pixels is not refused", h, w, cap);
                    ++refusals;
                    continue;
                }
                if (st != GS_OK)
                    return fail("refused", h, w, cap);
                ++plans;
                const size_t want_cap = (long long)cap < (long long)h * w ? (size_t)cap : (size_t)h * (size_t)w;
                if (p.n_pixels != h * w || (size_t)p.cap != want_cap)
                    return fail("cap", h, w, cap);
                if (!covers(p.tiles_x, kMatchTileW, w) || !covers(p.tiles_y, kMatchTileH, h) || (long long)p.tiles_x * p.tiles_y > (long long)p.n_pixels)
                    return fail("tiles", h, w, cap);
                if (p.slots < kMatchMinSlots || (p.slots & (p.slots - 1)) != 0 || p.slots < 2 * (size_t)p.cap || p.slots > ((size_t)1 << 32))
                    return fail("slots", h, w, cap);
                if (p.slots > kMatchMinSlots && p.slots / 2 >= 2 * (size_t)p.cap)
                    return fail("slots: more than twice what is needed", h, w, cap);
                if ((size_t)p.n_blocks * kMatchThreads != p.slots)
                    return fail("n_blocks", h, w, cap);
                const size_t offs[] = {p.state_off, p.key_off, p.val_off, p.block_off, p.dense_key_off, p.dense_slot_off, p.bytes};
                const size_t need[] = {16, p.slots * 8, p.slots * 16, (size_t)p.n_blocks * 4, (size_t)p.cap * 8, (size_t)p.cap * 4};
                if (!laid_out(offs, need))
                    return fail("workspace layout", h, w, cap);
            }
    for (int b : kBad) {
        InstanceMatchPlan p;
        if (!refused(plan_instance_match(b, 10, 10, p), GS_ERR_INVALID, "positive") || p.bytes != 0 ||
            !refused(plan_instance_match(10, b, 10, p), GS_ERR_INVALID, "gs_instance_overlaps: ") || p.bytes != 0 ||
            !refused(plan_instance_match(10, 10, b, p), GS_ERR_INVALID, "pair_cap") || p.bytes != 0)
            return fail("a non-positive size is not refused", b, b, b);
        if (!refused(check_instance_match(b, 1, 1, 5, 1, 2), GS_ERR_INVALID, "gs_instance_match: pair_cap") ||
            !refused(check_instance_match(1, b - (b == 0), 1, 5, 1, 2), GS_ERR_INVALID, "negative") ||
            !refused(check_instance_match(1, 1, 1, b, 1, 2), GS_ERR_INVALID, "classes"))
            return fail("gs_instance_match's numbers", b, b, b);
        ++refusals;
    }
    // thresholds: every num / den up to 300 and the edges of the range
    int thresholds = 0;
    for (int den = -1; den <= 300; ++den)
        for (int num = -1; num <= 301; ++num) {
            const bool ok = num >= 1 && num <= den && 2 * num >= den;
            if ((check_instance_match(1, 0, 0, 5, num, den) == GS_OK) != ok)
                return fail("threshold", num, den);
            thresholds += ok;
        }
    const int edge[][3] = {{65535, 65535, 1}, {32768, 65535, 1}, {32767, 65535, 0}, {65536, 65536, 0}, {32768, 65536, 0}, {INT_MAX, INT_MAX, 0},
                           {INT_MAX / 2 + 1, INT_MAX, 0}, {INT_MIN, INT_MIN, 0}, {1, INT_MIN, 0}};
    for (const auto &e : edge)
        if ((check_instance_match(1, 0, 0, 5, e[0], e[1]) == GS_OK) != (e[2] != 0))
            return fail("threshold edge", e[0], e[1]);
    std::printf("instance match plan ok: %d plans, %d refusals, %d thresholds\n", plans, refusals, thresholds);
    return 0;
}

// ---- boundary_dist_plan.h
static int boundary_plans()
{
    int plans = 0, refusals = 0;
    size_t largest = 0;
    for (int h : kSizes)
        for (int w : kSizes) {
            BoundaryDistPlan p;
            g_err[0] = 0;
            const gs_status st = plan_boundary_dist(h, w, p);
            if (h > 32768 || w > 32768) {             // the side limit comes first, whatever the number of pixels
                if (!refused(st, GS_ERR_UNSUPPORTED, "32768", "gs_instance_boundary_dist: ", p))
                    return fail("a map beyond 32768 pixels a side is not refused", h, w);
                ++refusals;
                continue;
            }
            if (st != GS_OK)
                return fail("refused", h, w);
            ++plans;
            if (p.n_pixels != h * w || !covers(p.row_blocks, kBdistThreads / 64, 2ll * h) || !covers(p.pixel_blocks, kBdistThreads, p.n_pixels))
                return fail("n_pixels and grids", h, w);
            const size_t offs[] = {p.left_gt_off, p.right_gt_off, p.left_pred_off, p.right_pred_off, p.bytes};
            const size_t table = (size_t)p.n_pixels * 2, need[] = {table, table, table, table};
            if (!laid_out(offs, need))
                return fail("workspace layout", h, w);
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
    for (int b : kBad) {
        BoundaryDistPlan p;
        if (!refused(plan_boundary_dist(b, 10, p), GS_ERR_INVALID, "positive") || p.bytes != 0 ||
            !refused(plan_boundary_dist(10, b, p), GS_ERR_INVALID, "gs_instance_boundary_dist: ") || p.bytes != 0)
            return fail("a non-positive size is not refused", b, b);
        ++refusals;
    }
    std::printf("boundary dist plan ok: %d plans, %d refusals\n", plans, refusals);
    return 0;
}

int main()
{
    if (shared_checks() || instance_plans() || match_plans() || boundary_plans())
        return 1;
    std::printf("slide map plans ok\n");
    return 0;
}
