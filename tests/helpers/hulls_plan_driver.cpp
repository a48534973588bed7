// Sanitizer driver (tests/helpers/sanitized_driver.py) for csrc/hulls_plan.h, the host-only plan of gs_instance_hulls and the two
// integer functions of its rule.  Without arguments: sizes swept through the plan and what the launcher relies on checked -- the
// fill grid covers the pixels, the parts of the workspace are aligned, in order, large enough and inside the figure, the figure
// never shrinks with rows_cap, nothing overflows at the limits, refusals leave a text and a zero figure -- then known answers of
// hull_slope_less (equal slopes are not less: strictness) and hull_ratio_less (a pair whose products exceed 2^64 and whose order
// a comparison modulo 2^64 gets wrong).  With --rings: reads cases from standard input, each `y0 lines` and then `L R` per lattice
// line (R < 0: the line does not exist), and prints for each the ring and the stats row formed with the header's two functions, as
// the kernels of csrc/hulls.hip form them.  Built with g++ only: no device code in here.
#include "hulls_plan.h"
#include "plan_driver.h"

#include <vector>

static const int kSizes[] = {1, 2, 15, 16, 17, 255, 256, 257, 5000, 32767, 32768};
static const long long kCaps[] = {0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 300000, 1ll << 31, kHullMaxRows - 1, kHullMaxRows, kHullMaxRows + 1,
                                  LLONG_MAX};

static bool hulls_refused(int h, int w, long long cap, gs_status want, const char *word)
{
    HullsPlan p;
    g_err[0] = 0;
    return refused(plan_hulls(h, w, cap, p), want, word, "gs_instance_hulls: ", p);
}

struct Slope {
    long long num = 0, den = 0;
};

static bool strict_vertex(const std::vector<long long> &val, const std::vector<bool> &exists, int i)
{
    Slope above, below;
    for (int j = 0; j < (int)val.size(); ++j) {
        if (!exists[j] || j == i)
            continue;
        if (j < i) {
            if (above.den == 0 || hull_slope_less(above.num, above.den, val[i] - val[j], i - j))
                above.num = val[i] - val[j], above.den = i - j;
        } else if (below.den == 0 || hull_slope_less(val[j] - val[i], j - i, below.num, below.den))
            below.num = val[j] - val[i], below.den = j - i;
    }
    return above.den == 0 || below.den == 0 || hull_slope_less(above.num, above.den, below.num, below.den);
}

static int rings_from_stdin()
{
    int y0, lines;
    while (std::scanf("%d %d", &y0, &lines) == 2) {
        if (lines < 0 || lines > 1 << 16)
            return fail("lines", lines, 0);
        std::vector<long long> L(lines), R(lines), negR(lines);
        std::vector<bool> exists(lines);
        for (int j = 0; j < lines; ++j) {
            if (std::scanf("%lld %lld", &L[j], &R[j]) != 2)
                return fail("a line is missing", j, lines);
            exists[j] = R[j] >= 0;
            negR[j] = -R[j];
        }
        std::vector<long long> lx, ly, rx, ry, px, py;
        for (int j = 0; j < lines; ++j) {
            if (exists[j] && strict_vertex(L, exists, j))
                lx.push_back(L[j]), ly.push_back(y0 + j);
            if (exists[j] && strict_vertex(negR, exists, j))
                rx.push_back(R[j]), ry.push_back(y0 + j);
        }
        if (!lx.empty())
            px.push_back(lx[0]), py.push_back(ly[0]);
        for (size_t k = 0; k < rx.size(); ++k)
            px.push_back(rx[k]), py.push_back(ry[k]);
        for (size_t k = lx.size(); k > 1; --k)
            px.push_back(lx[k - 1]), py.push_back(ly[k - 1]);
        const int k = (int)px.size();
        long long area2 = 0, far2 = 0;
        unsigned long long best_w = 0, best_l = 0;
        int best_e = 0;
        for (int e = 0; e < k; ++e) {
            const int e1 = e + 1 < k ? e + 1 : 0;
            const long long ex = px[e1] - px[e], ey = py[e1] - py[e];
            area2 += px[e] * py[e1] - px[e1] * py[e];
            long long w = 0;
            for (int j = 0; j < k; ++j) {
                const long long vx = px[j] - px[e], vy = py[j] - py[e];
                const long long cr = ex * vy - ey * vx, d = vx * vx + vy * vy;
                w = (cr < 0 ? -cr : cr) > w ? (cr < 0 ? -cr : cr) : w;
                far2 = d > far2 ? d : far2;
            }
            const unsigned long long len2 = (unsigned long long)(ex * ex + ey * ey);
            if (e == 0 || hull_ratio_less((unsigned long long)w, len2, best_w, best_l))
                best_w = (unsigned long long)w, best_l = len2, best_e = e;
        }
        std::printf("%d %lld %lld %llu %llu %d", k, area2, far2, best_w, best_l, best_e);
        for (int j = 0; j < k; ++j)
            std::printf(" %lld %lld", px[j], py[j]);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--rings") == 0)
        return rings_from_stdin();
    int plans = 0, refusals = 0;
    // --------------------------------------------------------------------------------------------------------------- the plan
    for (int h : kSizes)
        for (int w : kSizes) {
            if ((long long)h * w > INT_MAX)
                continue;
            size_t before = 0;
            for (long long cap : kCaps) {
                HullsPlan p;
                g_err[0] = 0;
                if (plan_hulls(h, w, cap, p) != GS_OK || g_err[0])
                    return fail("refused", h, w, cap);
                ++plans;
                const long long rows = cap < kHullMaxRows ? cap : kHullMaxRows;
                if (p.rows_cap != rows || !covers(p.pixel_blocks, kHullThreads, (long long)h * w))
                    return fail("the fill grid", h, w, cap);
                if (p.stride_blocks < 1 || p.stride_blocks > kHullMaxGrid || (rows >= 1 && rows <= kHullMaxGrid && p.stride_blocks != rows))
                    return fail("the stride grid", h, w, cap);
                const size_t offs[] = {p.head_off, p.slot_off, p.rows_off, p.flags_off, p.bytes};
                const size_t need[] = {sizeof(HullHead), (size_t)rows * sizeof(HullSlot), (size_t)rows * 8, (size_t)rows * 2};
                if (!laid_out(offs, need))
                    return fail("the workspace layout", h, w, cap);
                if (p.bytes < before)
                    return fail("the figure shrinks with rows_cap", h, w, cap);
                before = p.bytes;
            }
        }
    for (int b : {0, -1, INT_MIN}) {
        if (!hulls_refused(b, 10, 4, GS_ERR_INVALID, "positive") || !hulls_refused(10, b, 4, GS_ERR_INVALID, "positive"))
            return fail("a non-positive side is not refused", b, b);
        refusals += 2;
    }
    for (int b : {32769, 46341, INT_MAX}) {
        if (!hulls_refused(b, 1, 4, GS_ERR_UNSUPPORTED, "side above") || !hulls_refused(1, b, 4, GS_ERR_UNSUPPORTED, "side above"))
            return fail("a side above 32768 is not refused", b, b);
        refusals += 2;
    }
    for (long long cap : {-1ll, (long long)INT_MIN, LLONG_MIN}) {
        if (!hulls_refused(10, 10, cap, GS_ERR_INVALID, "rows_cap"))
            return fail("a negative rows_cap is not refused", cap, 0);
        ++refusals;
    }
    for (long long cap : {-1ll, LLONG_MIN, (long long)INT_MAX + 1, LLONG_MAX}) {
        g_err[0] = 0;
        if (!refused(check_hull_points_cap(cap), GS_ERR_INVALID, "points_cap", "gs_instance_hulls: "))
            return fail("a points_cap out of range is not refused", cap, 0);
        ++refusals;
    }
    if (check_hull_points_cap(0) != GS_OK || check_hull_points_cap(INT_MAX) != GS_OK)
        return fail("a points_cap in range is refused", 0, INT_MAX);
    if (hull_tiles(1) != 1 || hull_tiles(255) != 1 || hull_tiles(256) != 2 || hull_tiles(511) != 2 || hull_tiles(512) != 3 ||
        hull_tiles(32768) != 129)
        return fail("hull_tiles", hull_tiles(255), hull_tiles(256));
    // -------------------------------------------------------------------------------------------------------------- the slopes
    // strictness: 1/2 against 2/4 is not less either way; 1/2 < 2/3; negative slopes; the far ends of the operands
    if (hull_slope_less(1, 2, 2, 4) || hull_slope_less(2, 4, 1, 2) || !hull_slope_less(1, 2, 2, 3) || hull_slope_less(2, 3, 1, 2))
        return fail("equal slopes or 1/2 < 2/3", 1, 2);
    if (!hull_slope_less(-2, 3, -1, 2) || hull_slope_less(-1, 2, -2, 3) || hull_slope_less(0, 5, 0, 7) || !hull_slope_less(-1, 32768, 0, 1))
        return fail("negative slopes", -2, 3);
    if (!hull_slope_less(32767, 32768, 32768, 32768) || hull_slope_less(32768, 1, 32768, 1) || !hull_slope_less(-32768, 1, 32768, 1) ||
        !hull_slope_less(32767, 32768, 32768, 32767))
        return fail("the far ends", 32768, 32768);
    {   // three collinear lines are one segment: the middle one is no vertex; bend it by one and it is (to the convex side only)
        const std::vector<bool> all(3, true);
        if (strict_vertex({0, 2, 4}, all, 1) || !strict_vertex({0, 1, 4}, all, 1) || strict_vertex({0, 3, 4}, all, 1) ||
            !strict_vertex({0, 2, 4}, all, 0) || !strict_vertex({0, 2, 4}, all, 2))
            return fail("the vertex rule at equal slopes", 0, 2);
        if (!strict_vertex({0, 9, 4}, {true, false, true}, 0) || !strict_vertex({5}, {true}, 0))
            return fail("a side without lines counts as satisfied", 0, 0);
    }
    // -------------------------------------------------------------------------------------------------------------- the ratios
    if (hull_ratio_less(3, 9, 1, 1) || hull_ratio_less(1, 1, 3, 9) || !hull_ratio_less(3, 10, 1, 1) || !hull_ratio_less(15, 25, 15, 9))
        return fail("small ratios", 3, 9);
    {   // 4926674^2 * 5817050 and 4925423^2 * 10699477 both exceed 2^64: exactly the first is the smaller ratio, modulo 2^64 the other
        const unsigned long long w1 = 4926674, l1 = 10699477, w2 = 4925423, l2 = 5817050;
        if (!hull_ratio_less(w1, l1, w2, l2) || hull_ratio_less(w2, l2, w1, l1))
            return fail("the 128-bit comparison", (long long)w1, (long long)l1, (long long)w2, (long long)l2);
        if (!(w2 * w2 * l1 < w1 * w1 * l2))       // the wrapped products order the other way: the case is a test of the width
            return fail("the case does not wrap", (long long)(w1 * w1 * l2), (long long)(w2 * w2 * l1));
        const unsigned long long top = 4294967295ull;                  // w and len2 at the far end: 2^96 and no overflow of 128 bits
        if (hull_ratio_less(top, top, top, top) || !hull_ratio_less(top - 1, top, top, top) || !hull_ratio_less(top, top, top, top - 1))
            return fail("the far end of the ratios", 0, 0);
    }
    std::printf("hulls plan ok: %d plans, %d refusals\n", plans, refusals);
    return 0;
}
