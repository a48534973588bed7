// Plans of gs_rim_classes and gs_loop_arcs (csrc/lesions.hip, definitions in csrc/lesions_abi.h): what the entries refuse about
// sizes, the grids of their launches, the LDS of the rim kernel and where the parts of gs_loop_arcs' workspace lie.  Host-only and
// free of device code (slide_map_plan.h, which has the shared refusals and the layout): gs_loop_arcs_plan answers without a
// device, and the launchers size their launches with the same functions.
//
// The constants.  A rim tile is 64 x 16 pixels, four pixels a thread: a row of 64 labels is one wave's coalesced load.  Around it
// the kernel stages a halo of R = floor(sqrt(max_d2)) <= 32 cells, a label (4 bytes) and a class (1 byte) per cell: at most
// 128 x 80 cells, 51 200 bytes, below the 64 KB a launch may ask for without raising a limit; three such workgroups share a CU's
// 160 KB.  An arcs workgroup takes 256 corners or 256 unit edges, a lane each.
#pragma once
#include "slide_map_plan.h"

namespace gs {

constexpr int kLesionThreads = 256;             // threads of every launch but the scans: four waves
constexpr int kLesionMaxSide = 32768;           // as the zones: a tile count per side stays small and y * width + x is the pixels' check
constexpr int kRimMaxD2 = 1024;                 // max_d2 at the most: a radius of 32 map pixels
constexpr int kRimMaxReach = 32;                // floor(sqrt(kRimMaxD2))
constexpr int kRimTileW = 64, kRimTileH = 16;   // pixels of a tile: kLesionThreads * 4
constexpr int kArcMaxBits = 31;                 // bits of a mask word that may be asked for: the sign bit is left alone

struct RimPlan {
    int reach = 0;             // floor(sqrt(max_d2))
    int tiles_x = 0;           // ceil(width / kRimTileW)
    int tiles_y = 0;           // ceil(height / kRimTileH)
    int blocks = 0;            // tiles_x * tiles_y
    int cell_w = 0;            // kRimTileW + 2 * reach: the cells of a staged row
    int cell_h = 0;            // kRimTileH + 2 * reach
    int lds_bytes = 0;         // 4 * cells (labels) + cells rounded up to 16 (classes)
};

struct ArcsPlan {
    int corner_blocks = 0;     // ceil(n_points / kLesionThreads), at least 1
    int edge_blocks = 0;       // ceil(edges / kLesionThreads), at least 1
    int loop_bit_blocks = 0;   // ceil(n_loops * bits / kLesionThreads), at least 1
    size_t seg_len_off = 0;    // int32 [n_points]: the unit edges of the segment that starts at the corner
    size_t seg_loop_off = 0;   // int32 [n_points]: its loop, -1 for a corner of no loop
    size_t seg_sum_off = 0;    // int64 [corner_blocks]: the segments' lengths per workgroup, then the edges in front of it
    size_t loop_base_off = 0;  // int32 [n_loops]: the loop's first position in the edge arrays
    size_t edge_mask_off = 0;  // int32 [edges]: the mask word of every unit edge's pixel, loop by loop in walking order
    size_t edge_loop_off = 0;  // int32 [edges]: its loop, -1 where no segment reaches
    size_t carry_off = 0;      // int32 [bits, edge_blocks]: the last uncovered position of the workgroup, then of those in front
    size_t wrap_off = 0;       // int32 [n_loops, bits]: the run at the sequence's start plus the run at its end
    size_t bytes = 0;
};

inline gs_status check_lesion_map(const char *entry, int height, int width)
{
    gs_status st;
    if ((st = check_map_sides(entry, height, width)) != GS_OK)
        return st;
    if (height > kLesionMaxSide || width > kLesionMaxSide) {
        set_error("%s: maps of %d x %d have a side above %d", entry, height, width, kLesionMaxSide);
        return GS_ERR_UNSUPPORTED;
    }
    return check_map_pixels(entry, height, width);
}

// floor(sqrt(v)) for 0 <= v <= kRimMaxD2
inline int rim_isqrt(int v)
{
    int r = 0;
    while (r < kRimMaxReach && (r + 1) * (r + 1) <= v)
        ++r;
    return r;
}

inline gs_status plan_rim(int n, int classes, int height, int width, long long max_d2, RimPlan &out)
{
    out = RimPlan();
    gs_status st;
    if ((st = check_lesion_map("gs_rim_classes", height, width)) != GS_OK || (st = check_map_classes("gs_rim_classes", classes)) != GS_OK)
        return st;
    if (n < 0) {
        set_error("gs_rim_classes: n must not be negative (got %d)", n);
        return GS_ERR_INVALID;
    }
    if (max_d2 < 0 || max_d2 > kRimMaxD2) {
        set_error("gs_rim_classes: max_d2 must be 0..%d (got %lld)", kRimMaxD2, max_d2);
        return GS_ERR_INVALID;
    }
    out.reach = rim_isqrt((int)max_d2);
    out.tiles_x = (width + kRimTileW - 1) / kRimTileW;                // <= 512
    out.tiles_y = (height + kRimTileH - 1) / kRimTileH;               // <= 2048
    out.blocks = out.tiles_x * out.tiles_y;                           // <= 2^20
    out.cell_w = kRimTileW + 2 * out.reach;                           // <= 128
    out.cell_h = kRimTileH + 2 * out.reach;                           // <= 80
    const int cells = out.cell_w * out.cell_h;                        // <= 10240
    out.lds_bytes = 4 * cells + (cells + 15) / 16 * 16;               // <= 51200
    return GS_OK;
}

inline gs_status plan_arcs(long long edges, long long n_points, long long n_loops, int bits, ArcsPlan &out)
{
    out = ArcsPlan();
    if (bits < 1 || bits > kArcMaxBits) {
        set_error("gs_loop_arcs: bits must be 1..%d (got %d)", kArcMaxBits, bits);
        return GS_ERR_INVALID;
    }
    if (edges < 0 || n_points < 0 || n_loops < 0) {
        set_error("gs_loop_arcs: the counts must not be negative (got %lld edges, %lld points, %lld loops)", edges, n_points, n_loops);
        return GS_ERR_INVALID;
    }
    if (edges > (long long)INT_MAX) {
        set_error("gs_loop_arcs: more than 2^31 - 1 edges (got %lld)", edges);
        return GS_ERR_INVALID;
    }
    if (n_points > edges || n_loops > edges / 4) {                    // a corner is the end of an edge, a loop has at least four
        set_error("gs_loop_arcs: %lld points and %lld loops do not go with %lld edges", n_points, n_loops, edges);
        return GS_ERR_INVALID;
    }
    const long long per = kLesionThreads;
    out.corner_blocks = (int)((n_points + per - 1) / per);            // <= 2^23
    out.edge_blocks = (int)((edges + per - 1) / per);
    out.loop_bit_blocks = (int)((n_loops * bits + per - 1) / per);    // n_loops * bits < 2^34
    out.corner_blocks = out.corner_blocks ? out.corner_blocks : 1;
    out.edge_blocks = out.edge_blocks ? out.edge_blocks : 1;
    out.loop_bit_blocks = out.loop_bit_blocks ? out.loop_bit_blocks : 1;
    PlanCursor ws;
    out.seg_len_off = ws.take((size_t)n_points * 4);
    out.seg_loop_off = ws.take((size_t)n_points * 4);
    out.seg_sum_off = ws.take((size_t)out.corner_blocks * 8);
    out.loop_base_off = ws.take((size_t)n_loops * 4);
    out.edge_mask_off = ws.take((size_t)edges * 4);
    out.edge_loop_off = ws.take((size_t)edges * 4);
    out.carry_off = ws.take((size_t)bits * (size_t)out.edge_blocks * 4);
    out.wrap_off = ws.take((size_t)n_loops * (size_t)bits * 4);
    out.bytes = ws.off;
    return GS_OK;
}

}  // namespace gs
