// Sanitizer driver (tests/helpers/sanitized_driver.py) for csrc/split_plan.h, the host-only plans of gs_foreground_edt,
// gs_label_peaks and gs_split_cut: size lists swept through the three plans, and what the launchers rely on checked -- the bands
// and column tiles cover the map, the grids are positive and within their limits, the row pass's LDS holds the row or is not used,
// the parts of every workspace are aligned, in order, large enough and inside the figure, no figure shrinks when an argument
// grows, and refusals leave a text and a zero figure.  Built with g++ only: no HIP in here.
#include "split_plan.h"
#include "plan_driver.h"

static const int kSizes[] = {1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 517, 5000, 16383, 16384, 16385, 32767, 32768, 32769, 46341,
                             65536, 1 << 20, INT_MAX};
static const int kCounts[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 4096, 262143, 262144, 262145, 1 << 24, INT_MAX - 1, INT_MAX};

int main()
{
    int plans = 0, refusals = 0;
    // the distance map
    for (int h : kSizes)
        for (int w : kSizes) {
            EdtPlan p;
            SplitPlan q;
            g_err[0] = 0;
            const gs_status st = plan_edt(h, w, p);
            const bool side = h > kSplitMaxSide || w > kSplitMaxSide, pixels = (long long)h * w > (long long)INT_MAX;
            if (side || pixels) {                  // the side limit comes first
                if (!refused(st, GS_ERR_UNSUPPORTED, side ? "32768" : "2^31", "gs_foreground_edt: ", p))
                    return fail("a map beyond the limits is not refused", h, w);
                if (!refused(plan_split(h, w, 1, 1, q), GS_ERR_UNSUPPORTED, side ? "32768" : "2^31", "gs_split_cut: ", q))
                    return fail("a map beyond the limits is not refused by the cut", h, w);
                ++refusals;
                continue;
            }
            if (st != GS_OK || g_err[0])
                return fail("refused", h, w);
            ++plans;
            if ((long long)p.bands * kEdtBand < h || (long long)(p.bands - 1) * kEdtBand >= h || (long long)p.col_tiles * kSplitThreads < w ||
                (long long)(p.col_tiles - 1) * kSplitThreads >= w || p.band_blocks != p.bands * p.col_tiles || p.carry_blocks != p.col_tiles ||
                p.band_blocks < 1)
                return fail("bands and tiles", h, w);
            if (w <= kEdtLdsCols ? (p.row_lds_bytes < 2 * w || p.row_lds_bytes % 4 || p.row_lds_bytes > 32768) : p.row_lds_bytes != 0)
                return fail("the row pass's LDS", h, w, p.row_lds_bytes);
            const size_t table = (size_t)p.bands * (size_t)w * 2;
            const size_t offs[] = {p.g_off, p.top_off, p.bot_off, p.down_off, p.up_off, p.bytes};
            const size_t need[] = {(size_t)h * (size_t)w * 2, table, table, table, table};
            if (!laid_out(offs, need))
                return fail("workspace layout of the distance map", h, w);
            // the largest distances fit: a column distance 16 bits, a carry 16 bits, a squared distance an int32
            if ((h + 1) / 2 > 16384 || h > 65535)
                return fail("16 bits", h, w);
            // never shrinks with a side
            EdtPlan a, b;
            if (h > 1 && (plan_edt(h - 1, w, a) != GS_OK || a.bytes > p.bytes))
                return fail("the figure shrinks with the height", h, w);
            if (w > 1 && (plan_edt(h, w - 1, b) != GS_OK || b.bytes > p.bytes))
                return fail("the figure shrinks with the width", h, w);
            // the cut on this map
            size_t before_n = 0;
            for (int n : kCounts) {
                size_t before_c = 0;
                for (int c : kCounts) {
                    if (plan_split(h, w, n, c, q) != GS_OK || g_err[0])
                        return fail("the cut is refused", h, w, n, c);
                    ++plans;
                    if ((long long)q.pixel_blocks * kSplitThreads < (long long)h * w || (long long)(q.pixel_blocks - 1) * kSplitThreads >= (long long)h * w)
                        return fail("pixel grid", h, w, n, c);
                    if (q.inst_blocks < 1 || q.inst_blocks > kSplitMaxGrid || q.core_blocks < 1 || q.core_blocks > kSplitMaxGrid)
                        return fail("stride grids", h, w, n, c);
                    if (n > 0 || c > 0) {
                        const size_t o[] = {q.off_off, q.cursor_off, q.owner_off, q.list_off, q.bytes};
                        const size_t nd[] = {(size_t)n * 4, (size_t)n * 4, (size_t)c * 4, (size_t)c * sizeof(SplitCore)};
                        if (!laid_out(o, nd))
                            return fail("workspace layout of the cut", h, w, n, c);
                    }
                    if (q.bytes < kPlanAlign || q.bytes < before_c)
                        return fail("the figure shrinks with c", h, w, n, c);
                    before_c = q.bytes;
                    SplitPlan one;
                    if (plan_split(1, 1, n, c, one) != GS_OK || one.bytes != q.bytes)
                        return fail("the cut's figure depends on the map", h, w, n, c);
                }
                if (before_c < before_n)
                    return fail("the figure shrinks with n", h, w, n);
                before_n = before_c;
            }
        }
    // the peaks
    size_t before = 0;
    for (int n : kCounts) {
        PeaksPlan p;
        if (plan_peaks(n, p) != GS_OK || g_err[0])
            return fail("peaks refused", n, 0);
        ++plans;
        if (p.key_off != 0 || p.bytes < (size_t)n * 8 || p.bytes < kPlanAlign || p.bytes >= (size_t)n * 8 + 2 * kPlanAlign || p.bytes % kPlanAlign ||
            p.bytes < before || p.stride_blocks < 1 || p.stride_blocks > kSplitMaxGrid)
            return fail("peaks plan", n, (long long)p.bytes);
        before = p.bytes;
    }
    if (split_stride_blocks(0) != 1 || split_stride_blocks(256) != 1 || split_stride_blocks(257) != 2 ||
        split_stride_blocks(INT_MAX) != kSplitMaxGrid)
        return fail("stride blocks", 0, 0);
    // refusals
    const int bad[] = {0, -1, INT_MIN};
    for (int b : bad) {
        EdtPlan p;
        SplitPlan q;
        if (!refused(plan_edt(b, 10, p), GS_ERR_INVALID, "positive", "gs_foreground_edt: ", p) ||
            !refused(plan_edt(10, b, p), GS_ERR_INVALID, "positive", "gs_foreground_edt: ", p) ||
            !refused(plan_split(b, 10, 1, 1, q), GS_ERR_INVALID, "positive", "gs_split_cut: ", q) ||
            !refused(plan_split(10, b, 1, 1, q), GS_ERR_INVALID, "positive", "gs_split_cut: ", q))
            return fail("a non-positive side is not refused", b, b);
        refusals += 4;
    }
    const int negative[] = {-1, -2, INT_MIN};
    for (int v : negative) {
        PeaksPlan p;
        SplitPlan q;
        if (!refused(plan_peaks(v, p), GS_ERR_INVALID, "negative", "gs_label_peaks: ", p) ||
            !refused(plan_split(10, 10, v, 1, q), GS_ERR_INVALID, "n must", "gs_split_cut: ", q) ||
            !refused(plan_split(10, 10, 1, v, q), GS_ERR_INVALID, "c must", "gs_split_cut: ", q))
            return fail("a negative count is not refused", v, 0);
        refusals += 3;
    }
    // with both sides within the limit a map has at most 2^30 pixels: the test of the pixels stands behind the side limit
    if (check_split_map("x", 32768, 32768) != GS_OK || check_split_map("x", 32768, 32769) != GS_ERR_UNSUPPORTED ||
        check_split_map("x", 46341, 46341) != GS_ERR_UNSUPPORTED)
        return fail("the map limits", 0, 0);
    std::printf("split plan ok: %d plans, %d refusals\n", plans, refusals);
    return 0;
}
