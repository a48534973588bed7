// Sanitizer driver (tests/helpers/sanitized_driver.py) for csrc/lesions_plan.h, the host-only plans of gs_rim_classes and
// gs_loop_arcs: sizes swept through both plans, and what the launchers rely on checked -- the rim grid covers the map in tiles,
// the staged cells hold the tile and its halo and their LDS stays below 64 KB, rim_isqrt equals a plain search; the arcs grids
// cover their items, the parts of the workspace are aligned, in order, large enough and inside the figure, the figure never shrinks
// when an argument grows, nothing overflows at the limits (2^31 - 1 edges and points, 31 bits), and refusals leave a text and a
// zero figure.  Built with g++ only: no device code in here.
#include "lesions_plan.h"
#include "plan_driver.h"

static const int kSizes[] = {1, 2, 15, 16, 17, 63, 64, 65, 513, 5000, 32767, 32768};
static const long long kCounts[] = {0, 4, 5, 255, 256, 257, 1024, 300000, 24200000, (long long)INT_MAX - 1, (long long)INT_MAX};

static bool rim_refused(int n, int classes, int h, int w, long long d2, gs_status want, const char *word)
{
    RimPlan p;
    g_err[0] = 0;
    const gs_status st = plan_rim(n, classes, h, w, d2, p);
    return refused(st, want, word, "gs_rim_classes: ", (size_t)(p.blocks | p.lds_bytes));     // both figures zero
}

static bool arcs_refused(long long edges, long long points, long long loops, int bits, const char *word)
{
    ArcsPlan p;
    g_err[0] = 0;
    return refused(plan_arcs(edges, points, loops, bits, p), GS_ERR_INVALID, word, "gs_loop_arcs: ", p);
}

int main()
{
    int plans = 0, refusals = 0;
    // ---------------------------------------------------------------------------------------------------------------- the rim
    int want = 0;
    for (int v = 0; v <= kRimMaxD2; ++v) {
        while ((want + 1) * (want + 1) <= v)
            ++want;
        if (rim_isqrt(v) != want)
            return fail("rim_isqrt", v, want);
    }
    if (rim_isqrt(kRimMaxD2) != kRimMaxReach)
        return fail("the reach at the cap", kRimMaxD2, kRimMaxReach);
    for (int h : kSizes)
        for (int w : kSizes)
            for (int d2 : {0, 1, 2, 4, 25, 1023, 1024}) {
                RimPlan p;
                g_err[0] = 0;
                if (plan_rim(3, 5, h, w, d2, p) != GS_OK || g_err[0])
                    return fail("rim refused", h, w);
                ++plans;
                if (!covers(p.tiles_x, kRimTileW, w) || !covers(p.tiles_y, kRimTileH, h) || p.blocks != p.tiles_x * p.tiles_y)
                    return fail("rim grid", h, w);
                if (p.reach * p.reach > d2 || (p.reach + 1) * (p.reach + 1) <= d2 || p.cell_w != kRimTileW + 2 * p.reach ||
                    p.cell_h != kRimTileH + 2 * p.reach)
                    return fail("rim cells", d2, p.reach);
                if (p.lds_bytes < 5 * p.cell_w * p.cell_h || p.lds_bytes > 5 * p.cell_w * p.cell_h + 16 || p.lds_bytes > 60 * 1024)
                    return fail("rim LDS", d2, p.lds_bytes);
            }
    for (int b : {0, -1, INT_MIN}) {
        if (!rim_refused(1, 5, b, 10, 0, GS_ERR_INVALID, "positive") || !rim_refused(1, 5, 10, b, 0, GS_ERR_INVALID, "positive"))
            return fail("a non-positive side is not refused", b, b);
        refusals += 2;
    }
    for (int b : {32769, 46341, INT_MAX}) {
        if (!rim_refused(1, 5, b, 1, 0, GS_ERR_UNSUPPORTED, "side above") || !rim_refused(1, 5, 1, b, 0, GS_ERR_UNSUPPORTED, "side above"))
            return fail("a side above 32768 is not refused", b, b);
        refusals += 2;
    }
    for (int c : {INT_MIN, -1, 0, 1, 21, INT_MAX}) {
        if (!rim_refused(1, c, 10, 10, 0, GS_ERR_INVALID, "classes"))
            return fail("classes out of range are not refused", c, 0);
        ++refusals;
    }
    for (int c : {2, 5, 20}) {
        RimPlan p;
        if (plan_rim(0, c, 10, 10, 0, p) != GS_OK || plan_rim(INT_MAX, c, 10, 10, 1024, p) != GS_OK)
            return fail("classes in range are refused", c, 0);
    }
    for (long long d2 : {-1ll, (long long)INT_MIN, 1025ll, (long long)INT_MAX, LLONG_MAX, LLONG_MIN}) {
        if (!rim_refused(1, 5, 10, 10, d2, GS_ERR_INVALID, "max_d2"))
            return fail("max_d2 out of range is not refused", d2, 0);
        ++refusals;
    }
    for (int n : {-1, INT_MIN}) {
        if (!rim_refused(n, 5, 10, 10, 0, GS_ERR_INVALID, "negative"))
            return fail("a negative n is not refused", n, 0);
        ++refusals;
    }
    // --------------------------------------------------------------------------------------------------------------- the arcs
    for (long long edges : kCounts)
        for (long long points : kCounts)
            for (long long loops : kCounts)
                for (int bits : {1, 5, 20, 31}) {
                    if (points > edges || loops > edges / 4)
                        continue;
                    ArcsPlan p, q;
                    g_err[0] = 0;
                    if (plan_arcs(edges, points, loops, bits, p) != GS_OK || g_err[0])
                        return fail("arcs refused", edges, points);
                    ++plans;
                    if ((points ? !covers(p.corner_blocks, kLesionThreads, points) : p.corner_blocks != 1) ||
                        (edges ? !covers(p.edge_blocks, kLesionThreads, edges) : p.edge_blocks != 1) ||
                        (loops ? !covers(p.loop_bit_blocks, kLesionThreads, loops * bits) : p.loop_bit_blocks != 1))
                        return fail("arcs grids", edges, loops);
                    const size_t offs[] = {p.seg_len_off,   p.seg_loop_off, p.seg_sum_off, p.loop_base_off, p.edge_mask_off,
                                           p.edge_loop_off, p.carry_off,    p.wrap_off,    p.bytes};
                    const size_t need[] = {(size_t)points * 4, (size_t)points * 4, (size_t)p.corner_blocks * 8, (size_t)loops * 4,
                                           (size_t)edges * 4,  (size_t)edges * 4,  (size_t)bits * p.edge_blocks * 4,
                                           (size_t)loops * bits * 4};
                    if (!laid_out(offs, need))
                        return fail("arcs workspace layout", edges, loops);
                    // never shrinks: one less of each argument in turn
                    if (edges > 0 && points <= edges - 1 && loops <= (edges - 1) / 4 &&
                        (plan_arcs(edges - 1, points, loops, bits, q) != GS_OK || q.bytes > p.bytes))
                        return fail("the figure shrinks with the edges", edges, points);
                    if (points > 0 && (plan_arcs(edges, points - 1, loops, bits, q) != GS_OK || q.bytes > p.bytes))
                        return fail("the figure shrinks with the points", edges, points);
                    if (loops > 0 && (plan_arcs(edges, points, loops - 1, bits, q) != GS_OK || q.bytes > p.bytes))
                        return fail("the figure shrinks with the loops", edges, loops);
                    if (bits > 1 && (plan_arcs(edges, points, loops, bits - 1, q) != GS_OK || q.bytes > p.bytes))
                        return fail("the figure shrinks with the bits", edges, bits);
                }
    {   // the far end in figures: 2^31 - 1 edges and points, a quarter as many loops, 31 bits
        ArcsPlan p;
        const long long e = INT_MAX, l = e / 4;
        if (plan_arcs(e, e, l, 31, p) != GS_OK)
            return fail("the far end is refused", e, l);
        const unsigned long long least = 16ull * e + 4ull * l + 4ull * 31 * l + 4ull * 31 * ((e + 255) / 256);
        if (p.bytes < least || p.bytes > least + (1ull << 27) || p.edge_blocks != (1 << 23) || p.loop_bit_blocks <= 0)
            return fail("the far end's figure", (long long)p.bytes, (long long)least);
    }
    for (int bits : {INT_MIN, -1, 0, 32, INT_MAX}) {
        if (!arcs_refused(100, 10, 2, bits, "bits"))
            return fail("bits out of range are not refused", bits, 0);
        ++refusals;
    }
    for (long long v : {-1ll, LLONG_MIN}) {
        if (!arcs_refused(v, 0, 0, 5, "negative") || !arcs_refused(100, v, 0, 5, "negative") || !arcs_refused(100, 0, v, 5, "negative"))
            return fail("a negative count is not refused", v, 0);
        refusals += 3;
    }
    for (long long v : {(long long)INT_MAX + 1, 1ll << 40, LLONG_MAX}) {
        if (!arcs_refused(v, 0, 0, 5, "2^31 - 1"))
            return fail("too many edges are not refused", v, 0);
        ++refusals;
    }
    if (!arcs_refused(100, 101, 2, 5, "do not go with") || !arcs_refused(100, 10, 26, 5, "do not go with") ||
        !arcs_refused(3, 0, 1, 5, "do not go with") || !arcs_refused(100, LLONG_MAX, 0, 5, "do not go with") ||
        !arcs_refused(100, 0, LLONG_MAX, 5, "do not go with"))
        return fail("counts that do not go together are not refused", 0, 0);
    refusals += 5;
    {
        ArcsPlan p;
        if (plan_arcs(100, 100, 25, 5, p) != GS_OK || plan_arcs(0, 0, 0, 1, p) != GS_OK)
            return fail("counts at their limits are refused", 100, 25);
    }
    std::printf("lesions plan ok: %d plans, %d refusals\n", plans, refusals);
    return 0;
}
