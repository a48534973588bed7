// Sanitizer driver (tests/helpers/sanitized_driver.py) for csrc/outlines_plan.h, the host-only plan of gs_instance_outlines: a
// size list and an edges_cap list swept through the plan, and what the launcher relies on checked -- the pixel grid covers the map
// and the edge grid the cap in workgroups of kOutThreads, 2^rounds covers the cap and 2^(rounds - 1) does not, the parts of the
// workspace are aligned, in order, large enough and inside the figure, the figure never shrinks with the cap nor with the map,
// and refusals leave a text and a zero figure.  Built with g++ only: no HIP in here.
#include "outlines_plan.h"
#include "plan_driver.h"

static const int kSizes[] = {1, 2, 3, 63, 64, 65, 255, 256, 257, 300, 517, 5000, 32768, 46340, 46341, 65536, 1 << 20, INT_MAX};
static const long long kCaps[] = {0, 1, 2, 3, 4, 5, 255, 256, 257, 258, 1023, 1024, 1025, 28700, 1 << 20, (1ll << 30) - 1, 1ll << 30,
                                  (1ll << 30) + 1, (1ll << 31) - 2, (1ll << 31) - 1};

static const char kEntry[] = "gs_instance_outlines: ";

int main()
{
    int plans = 0, refusals = 0;
    for (long long cap : kCaps) {
        size_t before = 0;
        long long pixels_before = 0;
        for (int side : kSizes)
            for (int other : {1, 2, side}) {
                const int h = side, w = other;
                OutlinesPlan p;
                g_err[0] = 0;
                const gs_status st = plan_outlines(h, w, cap, p);
                const long long pixels = (long long)h * w;
                if (pixels > INT_MAX) {
                    if (!refused(st, GS_ERR_UNSUPPORTED, "pixels", kEntry, p))
                        return fail("a map of more than 2^31 - 1 pixels is not refused", h, w, cap);
                    ++refusals;
                    continue;
                }
                if (st != GS_OK || g_err[0])
                    return fail("refused", h, w, cap);
                ++plans;
                if (p.n_pixels != pixels || p.edges_cap != cap)
                    return fail("sizes", h, w, cap);
                if ((long long)p.pixel_blocks * kOutThreads < pixels || ((long long)p.pixel_blocks - 1) * kOutThreads >= pixels)
                    return fail("pixel grid", h, w, cap);
                if (p.edge_blocks < 1 || (long long)p.edge_blocks * kOutThreads < cap ||
                    (cap > 0 && ((long long)p.edge_blocks - 1) * kOutThreads >= cap))
                    return fail("edge grid", h, w, cap);
                if (p.rounds < 0 || p.rounds > 31 || (1ll << p.rounds) < cap || (p.rounds > 0 && (1ll << (p.rounds - 1)) >= cap))
                    return fail("rounds", h, w, cap);
                const size_t offs[] = {p.head_off,     p.pixel_count_off, p.pixel_base_off, p.edge_pixel_off, p.edge_side_off, p.count_a_off,
                                       p.count_b_off,  p.state_off[0],    p.state_off[1],   p.row_off,        p.bytes};
                const size_t need[] = {sizeof(OutHead),
                                       (size_t)p.pixel_blocks * 4,
                                       (size_t)pixels * 4,
                                       (size_t)cap * 4,
                                       (size_t)cap,
                                       (size_t)p.edge_blocks * 4,
                                       (size_t)p.edge_blocks * 4,
                                       (size_t)cap * sizeof(OutState),
                                       (size_t)cap * sizeof(OutState),
                                       (size_t)cap * sizeof(OutRow)};
                for (int k = 0; k < 10; ++k)
                    if (offs[k] % kPlanAlign != 0 || offs[k + 1] < offs[k] + need[k] || offs[k + 1] >= offs[k] + need[k] + kPlanAlign)
                        return fail("workspace layout", h, w, cap);
                if (offs[0] != 0)
                    return fail("the head is not first", h, w, cap);
                if (pixels >= pixels_before && p.bytes < before)         // the sizes come in rising order of pixels but for (side, 2) / (next, 1)
                    return fail("the figure shrinks with the map", h, w, cap);
                if (pixels >= pixels_before) {
                    before = p.bytes;
                    pixels_before = pixels;
                }
                OutlinesPlan q;
                if (cap > 0 && (plan_outlines(h, w, cap - 1, q) != GS_OK || q.bytes > p.bytes))
                    return fail("the figure shrinks with edges_cap", h, w, cap);
            }
    }
    const int bad[] = {0, -1, INT_MIN};
    for (int b : bad) {
        OutlinesPlan p;
        if (!refused(plan_outlines(b, 10, 10, p), GS_ERR_INVALID, "positive", kEntry, p) ||
            !refused(plan_outlines(10, b, 10, p), GS_ERR_INVALID, "positive", kEntry, p))
            return fail("a non-positive side is not refused", b, b);
        ++refusals;
    }
    const long long bad_caps[] = {-1, -2, LLONG_MIN, 1ll << 31, 1ll << 40, LLONG_MAX};
    for (long long c : bad_caps) {
        OutlinesPlan p;
        if (!refused(plan_outlines(10, 10, c, p), GS_ERR_INVALID, "edges_cap", kEntry, p))
            return fail("an edges_cap out of range is not refused", c, 0);
        ++refusals;
    }
    if (outline_rounds(0) != 0 || outline_rounds(1) != 0 || outline_rounds(2) != 1 || outline_rounds(256) != 8 || outline_rounds(257) != 9 ||
        outline_rounds(258) != 9 || outline_rounds(INT_MAX) != 31)
        return fail("rounds of the bars", 256, 258);
    std::printf("outlines plan ok: %d plans, %d refusals\n", plans, refusals);
    return 0;
}
