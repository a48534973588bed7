// Workspace plans of gs_foreground_edt, gs_label_peaks and gs_split_cut (csrc/split.hip): what the entries refuse about sizes, the
// grids of their launches and where the parts of the caller's workspace lie.  Host-only and free of HIP (slide_map_plan.h, which
// has the shared refusals and the layout): the *_plan entries of include/glomseg_split.h answer without a device, and the launchers
// lay the workspaces out with the same functions.
#pragma once
#include "slide_map_plan.h"

namespace gs {

constexpr int kSplitThreads = 256;              // threads of every launch but the scan: four waves
constexpr int kSplitMaxSide = 32768;            // g <= 16384 fits 16 bits and d2 <= 2^28 an int32; a core's dx*dx + dy*dy < 2^31
constexpr int kEdtBand = 32;                    // rows of a band of the column pass: a lane walks them down its column
constexpr int kEdtLdsCols = 16384;              // the row pass stages a row of g in LDS up to this width (32 KB), beyond it reads global
constexpr int kPeakRows = 16;                   // rows a lane of the peak pass walks down its column
constexpr int kSplitMaxGrid = 1024;             // workgroups of the grid-stride launches at the most: four per CU
constexpr int kSplitMinCores = 2, kSplitMaxCores = 1024;

// One core of an instance's list, as the fill launch writes it: 16 bytes.
struct SplitCore {
    int cx, cy;                // the centre, from core_pos
    int r2;                    // core_r2
    int id;                    // 1..c
};
static_assert(sizeof(SplitCore) == 16, "the plan counts 16 bytes a core");

struct EdtPlan {
    int bands = 0;             // ceil(height / kEdtBand)
    int col_tiles = 0;         // ceil(width / kSplitThreads)
    int band_blocks = 0;       // bands * col_tiles: the count launch and the apply launch
    int carry_blocks = 0;      // col_tiles: a lane per column walks the bands
    int row_lds_bytes = 0;     // the row pass's LDS: 2 * width rounded up to 4, or 0 beyond kEdtLdsCols
    size_t g_off = 0;          // uint16 [height,width]: the vertical distance
    size_t top_off = 0;        // uint16 [bands,width]: foreground pixels from the band's first row down to its first gap
    size_t bot_off = 0;        // uint16 [bands,width]: from its last row up
    size_t down_off = 0;       // uint16 [bands,width]: the run of foreground that ends right above the band
    size_t up_off = 0;         // uint16 [bands,width]: the run that begins right below it
    size_t bytes = 0;
};

struct PeaksPlan {
    int stride_blocks = 0;     // the clear and the finish launch
    size_t key_off = 0;        // uint64 [n]
    size_t bytes = 0;
};

struct SplitPlan {
    int pixel_blocks = 0;      // a thread per pixel: ceil(height * width / kSplitThreads)
    int inst_blocks = 0;       // grid-stride over n
    int core_blocks = 0;       // grid-stride over c
    size_t off_off = 0;        // int32 [n]: the first list entry of every instance
    size_t cursor_off = 0;     // int32 [n]: the entries filled so far
    size_t owner_off = 0;      // int32 [c]: the owner of every core, 0 where it is not valid
    size_t list_off = 0;       // SplitCore [c]
    size_t bytes = 0;
};

inline int split_stride_blocks(long long items)
{
    const long long b = (items + kSplitThreads - 1) / kSplitThreads;
    return (int)(b < 1 ? 1 : b < kSplitMaxGrid ? b : kSplitMaxGrid);
}

inline gs_status check_split_map(const char *entry, int height, int width)
{
    gs_status st;
    if ((st = check_map_sides(entry, height, width)) != GS_OK)
        return st;
    if (height > kSplitMaxSide || width > kSplitMaxSide) {
        set_error("%s: maps of %d x %d have a side above %d: a column distance need not fit 16 bits", entry, height, width, kSplitMaxSide);
        return GS_ERR_UNSUPPORTED;
    }
    return check_map_pixels(entry, height, width);
}

inline gs_status check_split_count(const char *entry, const char *name, int v)
{
    if (v >= 0)
        return GS_OK;
    set_error("%s: %s must not be negative (got %d)", entry, name, v);
    return GS_ERR_INVALID;
}

inline gs_status plan_edt(int height, int width, EdtPlan &out)
{
    out = EdtPlan();
    const gs_status st = check_split_map("gs_foreground_edt", height, width);
    if (st != GS_OK)
        return st;
    out.bands = (height + kEdtBand - 1) / kEdtBand;                   // <= 1024
    out.col_tiles = (width + kSplitThreads - 1) / kSplitThreads;      // <= 128
    out.band_blocks = out.bands * out.col_tiles;
    out.carry_blocks = out.col_tiles;
    out.row_lds_bytes = width <= kEdtLdsCols ? (2 * width + 3) / 4 * 4 : 0;
    const size_t table = (size_t)out.bands * (size_t)width * 2;
    PlanCursor ws;
    out.g_off = ws.take((size_t)height * (size_t)width * 2);
    out.top_off = ws.take(table);
    out.bot_off = ws.take(table);
    out.down_off = ws.take(table);
    out.up_off = ws.take(table);
    out.bytes = ws.off;
    return GS_OK;
}

inline gs_status plan_peaks(int n, PeaksPlan &out)
{
    out = PeaksPlan();
    const gs_status st = check_split_count("gs_label_peaks", "n", n);
    if (st != GS_OK)
        return st;
    out.stride_blocks = split_stride_blocks(n);
    PlanCursor ws;
    out.key_off = ws.take((size_t)n * 8);
    out.bytes = ws.off > 0 ? ws.off : kPlanAlign;                     // never nothing: the caller's workspace pointer is required
    return GS_OK;
}

inline gs_status plan_split(int height, int width, int n, int c, SplitPlan &out)
{
    out = SplitPlan();
    const char *entry = "gs_split_cut";
    gs_status st;
    if ((st = check_split_map(entry, height, width)) != GS_OK)
        return st;
    if ((st = check_split_count(entry, "n", n)) != GS_OK || (st = check_split_count(entry, "c", c)) != GS_OK)
        return st;
    out.pixel_blocks = (int)(((long long)height * width + kSplitThreads - 1) / kSplitThreads);      // <= 2^23
    out.inst_blocks = split_stride_blocks(n);
    out.core_blocks = split_stride_blocks(c);
    PlanCursor ws;
    out.off_off = ws.take((size_t)n * 4);
    out.cursor_off = ws.take((size_t)n * 4);
    out.owner_off = ws.take((size_t)c * 4);
    out.list_off = ws.take((size_t)c * sizeof(SplitCore));
    out.bytes = ws.off > 0 ? ws.off : kPlanAlign;
    return GS_OK;
}

}  // namespace gs
