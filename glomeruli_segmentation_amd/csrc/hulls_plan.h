// Workspace plan of gs_instance_hulls (csrc/hulls.hip, definitions in csrc/hulls_abi.h): what the entry refuses about sizes, the
// grids of its launches and where the parts of the caller's workspace lie, plus the two integer functions of the rule that the
// kernels and a host driver share: the slope comparison of the vertex rule and the 128-bit ratio comparison of the calipers.
// Host-only and free of device code (slide_map_plan.h, which has the shared refusals and the layout): gs_hulls_plan answers
// without a device, and the launcher lays the workspace out with the same function.
//
// The workspace is a function of rows_cap alone, as morphometry's: the plan does not know n, so the instance -> slot index lives
// in the caller's hull_offsets between the launches (hulls.hip), and everything else is per slot, per row or per lattice line.  A
// valid box has at least one row, so a row table that fits (rows_needed <= rows_cap) has at most rows_cap slots; a slot of
// `height` rows has height + 1 lattice lines, so all slots together have at most 2 * rows_cap lines.
#pragma once
#include "slide_map_plan.h"

namespace gs {

constexpr int kHullThreads = 256;               // threads of every launch but the scans: four waves
constexpr int kHullMaxSide = 32768;             // a coordinate is at most 32768: a cross product stays below 2^32, its square below 2^64
constexpr int kHullTile = 256;                  // lattice lines of a tile of the vertex pass: one per thread
constexpr int kHullMaxGrid = 1024;              // workgroups of the grid-stride and persistent launches at the most: four per CU
constexpr long long kHullMaxRows = (long long)INT_MAX * kHullMaxSide;       // what rows_needed can reach: n boxes of full height
constexpr long long kHullMaxPoints = INT_MAX;   // a ring index is an int32

// a / b < c / d for b, d > 0, exactly: every operand is a difference of coordinates or of line numbers, at most 32768 in size, so
// the products stay below 2^31.  The vertex rule of hulls_abi.h is this comparison, strict: equal slopes are no vertex.
constexpr bool hull_slope_less(long long a, long long b, long long c, long long d)
{
    return a * d < c * b;
}

// w1^2 / len1 < w2^2 / len2 for w >= 0, len > 0, exactly: w < 2^32 and len < 2^32, so a product reaches 2^96 and is formed in 128
// bits.  The narrowest caliper of hulls_abi.h is the edge that is less than every other by this comparison.
constexpr bool hull_ratio_less(unsigned long long w1, unsigned long long len1, unsigned long long w2, unsigned long long len2)
{
    return (unsigned __int128)w1 * w1 * len2 < (unsigned __int128)w2 * w2 * len1;
}

// the tiles of a slot of `height` rows: its height + 1 lattice lines in tiles of kHullTile; a tile is a task of the vertex pass
constexpr long long hull_tiles(int height) { return ((long long)height + 1 + kHullTile - 1) / kHullTile; }

// One valid box of the call, in instance order.  64 bytes.
struct HullSlot {
    long long row_off;         // its first row of the row table; its first lattice line is row_off + its own number
    long long task_off;        // its first task of the vertex pass (the exclusive scan of hull_tiles)
    long long base;            // its first point of `points` (the exclusive scan of right + left)
    int inst;                  // 1..n
    int x0, y0, x1, y1;        // the box, half-open, within the map
    int right;                 // vertices of the right chain: added to by the vertex pass
    int left;                  // vertices of the left chain
    int pad[3];
};
static_assert(sizeof(HullSlot) == 64, "the plan counts 64 bytes a slot");

// What the scans leave for the later launches.  One part of the workspace.
struct HullHead {
    long long rows_needed;
    long long n_tasks;         // 0 where the table does not fit
    int n_slots;               // 0 where the table does not fit
    int fits;                  // the row table fits; from the second scan on: and the points fit
};

struct HullsPlan {
    long long rows_cap = 0;    // the caller's, or kHullMaxRows where that is less
    int pixel_blocks = 0;      // the fill pass: a workgroup per kHullThreads pixels
    int stride_blocks = 0;     // every other pass: min(kHullMaxGrid, max(1, rows_cap)) workgroups
    size_t head_off = 0;       // HullHead
    size_t slot_off = 0;       // HullSlot [rows_cap]
    size_t rows_off = 0;       // int32 [rows_cap,2]: the smallest and the largest x of the instance in that row of its box
    size_t flags_off = 0;      // uint8 [2 * rows_cap]: per lattice line, bit 0 a right vertex, bit 1 a left vertex
    size_t bytes = 0;
};

inline gs_status plan_hulls(int height, int width, long long rows_cap, HullsPlan &out)
{
    out = HullsPlan();
    const char *entry = "gs_instance_hulls";
    gs_status st;
    if ((st = check_map_sides(entry, height, width)) != GS_OK)
        return st;
    if (rows_cap < 0) {
        set_error("%s: rows_cap must not be negative (got %lld)", entry, rows_cap);
        return GS_ERR_INVALID;
    }
    if (height > kHullMaxSide || width > kHullMaxSide) {
        set_error("%s: maps of %d x %d have a side above %d: a squared cross product need not fit 64 bits", entry, height, width,
                  kHullMaxSide);
        return GS_ERR_UNSUPPORTED;
    }
    if ((st = check_map_pixels(entry, height, width)) != GS_OK)
        return st;
    out.rows_cap = rows_cap < kHullMaxRows ? rows_cap : kHullMaxRows;       // < 2^46: the parts below stay far from 2^64
    out.pixel_blocks = (int)(((long long)height * width - 1) / kHullThreads + 1);     // <= 2^23
    out.stride_blocks = (int)(out.rows_cap < 1 ? 1 : out.rows_cap < kHullMaxGrid ? out.rows_cap : kHullMaxGrid);
    PlanCursor ws;
    out.head_off = ws.take(sizeof(HullHead));
    out.slot_off = ws.take((size_t)out.rows_cap * sizeof(HullSlot));
    out.rows_off = ws.take((size_t)out.rows_cap * 2 * sizeof(int));
    out.flags_off = ws.take((size_t)out.rows_cap * 2);
    out.bytes = ws.off;
    return GS_OK;
}

inline gs_status check_hull_points_cap(long long points_cap)
{
    if (points_cap >= 0 && points_cap <= kHullMaxPoints)
        return GS_OK;
    set_error("gs_instance_hulls: points_cap must be 0..2^31 - 1 (got %lld): a ring index is an int32", points_cap);
    return GS_ERR_INVALID;
}

}  // namespace gs
