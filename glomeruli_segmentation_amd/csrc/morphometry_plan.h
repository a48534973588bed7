// Workspace plan of gs_instance_morphometry (csrc/morphometry.hip): what the entry refuses about sizes, the grids of its launches
// and where the parts of the caller's workspace lie.  Host-only and free of HIP (slide_map_plan.h, which has the shared refusals
// and the layout): gs_morphometry_plan (include/glomseg_morphometry.h) answers without a device, and the launcher lays the
// workspace out with the same function.
//
// The workspace is a function of rows_cap alone: the entry has no per-instance array of its own (its plan does not know n), so
// the instance -> slot index lives in the caller's feret2 between the launches (morphometry.hip), and everything else is per
// slot or per row.  A valid box has at least one row, so a row table that fits (rows_needed <= rows_cap) has at most rows_cap
// slots.
#pragma once
#include "slide_map_plan.h"

namespace gs {

constexpr int kMorphThreads = 256;              // threads of every launch but the scan: four waves
constexpr int kMorphMaxSide = 32768;            // 2 * 32767^2 < 2^31: feret2 is an int32, and a candidate packs into x | y << 16
constexpr int kMorphRows = 16;                  // bit-quad windows a lane of the map pass walks down its column
constexpr int kMorphTile = 256;                 // candidates of a tile of the Feret pass: one per thread, 128 rows of an instance
constexpr int kMorphMaxGrid = 1024;             // workgroups of the two grid-stride launches at the most: four per CU
constexpr long long kMorphMaxRows = (long long)INT_MAX * kMorphMaxSide;     // what rows_needed can reach: n boxes of full height

// One valid box of the call, in instance order.  48 bytes.
struct MorphSlot {
    long long row_off;         // its first row of the row table
    long long task_off;        // its first task of the Feret pass (the exclusive scan of tiles * (tiles + 1) / 2)
    int inst;                  // 1..n
    int x0, y0, x1, y1;        // the box, half-open, within the map
    int best;                  // the largest d2 found so far
    int pad[2];
};
static_assert(sizeof(MorphSlot) == 48, "the plan counts 48 bytes a slot");

// What the scan leaves for the later launches.  One part of the workspace.
struct MorphHead {
    long long rows_needed;
    long long n_tasks;         // 0 where the table does not fit
    int n_slots;               // 0 where the table does not fit
    int fits;
};

struct MorphometryPlan {
    long long rows_cap = 0;    // the caller's, or kMorphMaxRows where that is less
    int window_blocks = 0;     // the map pass: a workgroup per 256 x kMorphRows bit-quad windows of the (width + 1) x (height + 1)
    int stride_blocks = 0;     // the clear pass and the Feret pass: min(kMorphMaxGrid, max(1, rows_cap)) workgroups
    size_t head_off = 0;       // MorphHead
    size_t slot_off = 0;       // MorphSlot [rows_cap]
    size_t rows_off = 0;       // int32 [rows_cap,2]: the smallest and the largest x of the instance in that row of its box
    size_t bytes = 0;
};

// the tiles of an instance of `height` rows (two candidates a row) and the tasks they make: every pair (a, b >= a)
constexpr long long morph_tiles(int height) { return (2ll * height + kMorphTile - 1) / kMorphTile; }
constexpr long long morph_tasks(int height) { return morph_tiles(height) * (morph_tiles(height) + 1) / 2; }

inline gs_status plan_morphometry(int height, int width, long long rows_cap, MorphometryPlan &out)
{
    out = MorphometryPlan();
    const char *entry = "gs_instance_morphometry";
    gs_status st;
    if ((st = check_map_sides(entry, height, width)) != GS_OK)
        return st;
    if (rows_cap < 0) {
        set_error("%s: rows_cap must not be negative (got %lld)", entry, rows_cap);
        return GS_ERR_INVALID;
    }
    if (height > kMorphMaxSide || width > kMorphMaxSide) {
        set_error("%s: maps of %d x %d have a side above %d: a squared diameter need not fit an int32", entry, height, width,
                  kMorphMaxSide);
        return GS_ERR_UNSUPPORTED;
    }
    // after the side limit, as in boundary_dist_plan.h: the sums of stats stay below 2^61 only with n_pixels <= INT_MAX
    if ((st = check_map_pixels(entry, height, width)) != GS_OK)
        return st;
    out.rows_cap = rows_cap < kMorphMaxRows ? rows_cap : kMorphMaxRows;     // < 2^46: the parts below stay far from 2^64
    out.window_blocks = (width / kMorphThreads + 1) * (height / kMorphRows + 1);  // ceil((side + 1) / unit) each: <= 129 * 2049
    out.stride_blocks = (int)(out.rows_cap < 1 ? 1 : out.rows_cap < kMorphMaxGrid ? out.rows_cap : kMorphMaxGrid);
    PlanCursor ws;
    out.head_off = ws.take(sizeof(MorphHead));
    out.slot_off = ws.take((size_t)out.rows_cap * sizeof(MorphSlot));
    out.rows_off = ws.take((size_t)out.rows_cap * 2 * sizeof(int));
    out.bytes = ws.off;
    return GS_OK;
}

}  // namespace gs
