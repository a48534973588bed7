// Workspace plan of gs_polygon_raster (csrc/raster.hip): what the entry refuses about sizes, the grids of its launches and where
// the parts of the caller's workspace lie, plus the two integer functions of the rule (raster_abi.h) that host and kernels share.
// Host-only and free of device code (slide_map_plan.h, which has the shared refusals and the layout): gs_polygon_raster_plan
// answers without a device, and the launcher lays the workspace out with the same function.
//
// The workspace is a function of n_features and words_cap: 28 bytes per feature (its box, the words of the features in front of
// it in its block of 256, its word base), eight bytes per block of features and four bytes per scratch word of the cap.  The
// sides, n_points and n_rings are checked and size grids only.
#pragma once
#include "slide_map_plan.h"

namespace gs {

constexpr int kRasterThreads = 256;             // threads of every launch but the scan: four waves, one item per thread
constexpr long long kRasterMaxCount = INT_MAX;  // a point, ring, feature or word index is an int32
constexpr int kRasterMaxFracBits = 8;
constexpr int kRasterCoordMax = 1 << 28;        // a coordinate beyond it is taken as the bound: all products stay inside int64

// ceil(a / b) for b > 0
constexpr long long raster_ceil_div(long long a, long long b)
{
    return a / b + (a % b > 0 ? 1 : 0);
}

// The first pixel (column or row) whose centre is at or beyond coordinate v, v in units of 1/(2S) pixel, clamped to [0, limit].
constexpr int raster_first_pixel(long long v, long long S, int limit)
{
    const long long t = raster_ceil_div(v - S, 2 * S);
    return t < 0 ? 0 : t > limit ? limit : (int)t;
}

constexpr int raster_clamp_coord(int q)
{
    return q < -kRasterCoordMax ? -kRasterCoordMax : q > kRasterCoordMax ? kRasterCoordMax : q;
}

// The box of a feature's vertices in toggle columns and rows.  Empty as the first launch leaves it: min above max.
struct alignas(16) RasterBox {
    int col_min, row_min, col_max, row_max;
};
static_assert(sizeof(RasterBox) == 16, "the plan counts 16 bytes a box");

// rows and words per row of a box's bit scratch (raster_abi.h, "words"); 0 rows for an empty box
constexpr long long raster_box_rows(const RasterBox &b) { return b.row_max > b.row_min ? (long long)b.row_max - b.row_min : 0; }
constexpr long long raster_box_row_words(const RasterBox &b)
{
    return b.col_max >= b.col_min ? ((long long)b.col_max - b.col_min) / 32 + 1 : 0;
}

// What the scan leaves for the later launches.  One part of the workspace.
struct RasterHead {
    long long words_needed;
    int fits;                  // words_needed <= words_cap
    int pad;
};

struct RasterPlan {
    int n_pixels = 0;          // height * width <= INT_MAX
    int n_points = 0, n_rings = 0, n_features = 0, words_cap = 0;
    int pixel_blocks = 0;      // workgroups of the pixel launches
    int point_blocks = 0;      // workgroups of the point launches; 0 with no points: they are not issued
    int feature_blocks = 0;    // workgroups of the feature launches: at least one
    int word_blocks = 0;       // workgroups of the scratch launches: at least one
    size_t head_off = 0;       // RasterHead
    size_t box_off = 0;        // RasterBox [n_features]
    size_t feature_front_off = 0;  // int64 [n_features]: the words of the features in front of it in its block
    size_t block_words_off = 0;    // int64 [feature_blocks]: words per block, then (scanned in place) words in front of the block
    size_t feature_base_off = 0;   // int32 [n_features]: the feature's first scratch word
    size_t scratch_off = 0;        // uint32 [words_cap]
    size_t bytes = 0;
};

inline gs_status check_raster_count(const char *entry, const char *what, long long v)
{
    if (v >= 0 && v <= kRasterMaxCount)
        return GS_OK;
    if (v < 0)
        set_error("%s: %s must not be negative (got %lld)", entry, what, v);
    else
        set_error("%s: %s must be at most 2^31 - 1 (got %lld): an index into it is an int32", entry, what, v);
    return GS_ERR_INVALID;
}

inline gs_status check_raster_frac_bits(const char *entry, int frac_bits)
{
    if (frac_bits >= 0 && frac_bits <= kRasterMaxFracBits)
        return GS_OK;
    set_error("%s: frac_bits must be 0..%d (got %d)", entry, kRasterMaxFracBits, frac_bits);
    return GS_ERR_INVALID;
}

inline int raster_blocks(long long items) { return items ? (int)((items - 1) / kRasterThreads + 1) : 0; }

inline gs_status plan_raster(int height, int width, long long n_points, long long n_rings, long long n_features, long long words_cap,
                             RasterPlan &out)
{
    out = RasterPlan();
    const char *entry = "gs_polygon_raster";
    gs_status st;
    if ((st = check_map_sides(entry, height, width)) != GS_OK)
        return st;
    if ((st = check_raster_count(entry, "n_points", n_points)) != GS_OK || (st = check_raster_count(entry, "n_rings", n_rings)) != GS_OK ||
        (st = check_raster_count(entry, "n_features", n_features)) != GS_OK || (st = check_raster_count(entry, "words_cap", words_cap)) != GS_OK)
        return st;
    if ((st = check_map_pixels(entry, height, width)) != GS_OK)
        return st;
    out.n_pixels = height * width;
    out.n_points = (int)n_points;
    out.n_rings = (int)n_rings;
    out.n_features = (int)n_features;
    out.words_cap = (int)words_cap;
    out.pixel_blocks = raster_blocks(out.n_pixels);
    out.point_blocks = raster_blocks(n_points);
    out.feature_blocks = n_features ? raster_blocks(n_features) : 1;
    out.word_blocks = words_cap ? raster_blocks(words_cap) : 1;
    PlanCursor ws;
    out.head_off = ws.take(sizeof(RasterHead));
    out.box_off = ws.take((size_t)n_features * sizeof(RasterBox));
    out.feature_front_off = ws.take((size_t)n_features * sizeof(long long));
    out.block_words_off = ws.take((size_t)out.feature_blocks * sizeof(long long));
    out.feature_base_off = ws.take((size_t)n_features * sizeof(int));
    out.scratch_off = ws.take((size_t)words_cap * sizeof(unsigned));
    out.bytes = ws.off;
    return GS_OK;
}

}  // namespace gs
