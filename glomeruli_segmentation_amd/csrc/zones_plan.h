// Workspace plans of gs_instance_zones and gs_foreign_dist (csrc/zones.hip, definitions in csrc/zones_abi.h): what the entries refuse
// about sizes, the grids of their launches and where the parts of the caller's workspace lie.  Host-only and free of device code
// (slide_map_plan.h, which has the shared refusals and the layout): the *_plan entries answer without a device, and the launchers
// lay the workspaces out with the same functions.
//
// The constants.  A band of the column pass is kZoneBand = 32 rows: a lane keeps a distance and a label per row in registers
// (64 VGPRs), and the carry tables cost 24 bytes per band and column, three quarters of a byte per pixel.  The row pass stages a
// row of g up to kZoneLdsCols = 16384 columns, 32 KB: five workgroups of four waves share a CU's 160 KB, and a map of slide size
// (5000 columns, 10 KB) is bounded by its waves, not by LDS.  Lanes next to each other read 16-bit words next to each other: two
// lanes share a dword, which is a broadcast, no bank conflict.
#pragma once
#include "slide_map_plan.h"

namespace gs {

constexpr int kZoneThreads = 256;               // threads of every launch: four waves
constexpr int kZoneMaxSide = 32768;             // a column distance is at most 32767: 16 bits with 0xFFFF to spare; dx*dx + g*g < 2^31
constexpr int kZoneMaxD2 = 1 << 30;             // max_d2 at the most: max_d2 + 1 and every dx*dx up to it stay inside int32
constexpr int kZoneBand = 32;                   // rows of a band of the column pass
constexpr int kZoneLdsCols = 16384;             // the row pass stages a row of g in LDS up to this width (32 KB), beyond it reads global
constexpr int kZoneNone = 0xFFFF;               // g: no instance pixel within reach (a link without a target is kLinkNone)

struct ZonePlan {
    int bands = 0;             // ceil(height / kZoneBand)
    int col_tiles = 0;         // ceil(width / kZoneThreads)
    int band_blocks = 0;       // bands * col_tiles: the count launch and the apply launch
    int carry_blocks = 0;      // col_tiles: a lane per column walks the bands
    int pixel_blocks = 0;      // a thread per pixel: the fill with n == 0
    int row_lds_bytes = 0;     // the row pass's LDS: 2 * width rounded up to 16, or 0 beyond kZoneLdsCols
    size_t g_off = 0;          // uint16 [height,width]: the vertical distance to the column's nearest instance pixel
    size_t clab_off = 0;       // int32  [height,width]: that pixel's label
    size_t top_d_off = 0;      // uint16 [bands,width]: rows from the band's first row down to its first instance pixel
    size_t bot_d_off = 0;      // uint16 [bands,width]: rows from its last row up to its last one
    size_t down_d_off = 0;     // uint16 [bands,width]: rows from the band's first row up to the nearest instance pixel above the band
    size_t up_d_off = 0;       // uint16 [bands,width]: rows from its last row down to the nearest one below it
    size_t top_l_off = 0;      // int32  [bands,width]: the labels of those four pixels
    size_t bot_l_off = 0;
    size_t down_l_off = 0;
    size_t up_l_off = 0;
    size_t bytes = 0;
};

struct ForeignPlan {
    int row_blocks = 0;        // a wave per row: ceil(height / 4)
    int pixel_blocks = 0;      // a thread per pixel
    size_t left_off = 0;       // uint16 [height,width]: the column of the nearest boundary pixel at or left of x
    size_t right_off = 0;      // uint16 [height,width]: at or right of x
    size_t bytes = 0;
};

inline gs_status check_zone_map(const char *entry, int height, int width)
{
    gs_status st;
    if ((st = check_map_sides(entry, height, width)) != GS_OK)
        return st;
    if (height > kZoneMaxSide || width > kZoneMaxSide) {
        set_error("%s: maps of %d x %d have a side above %d: a column distance need not fit 16 bits", entry, height, width, kZoneMaxSide);
        return GS_ERR_UNSUPPORTED;
    }
    return check_map_pixels(entry, height, width);
}

inline gs_status check_zone_count(const char *entry, int n)
{
    if (n >= 0)
        return GS_OK;
    set_error("%s: n must not be negative (got %d)", entry, n);
    return GS_ERR_INVALID;
}

inline gs_status check_zone_cap(const char *entry, long long max_d2)
{
    if (max_d2 >= 0 && max_d2 <= kZoneMaxD2)
        return GS_OK;
    set_error("%s: max_d2 must be 0..2^30 (got %lld)", entry, max_d2);
    return GS_ERR_INVALID;
}

// floor(sqrt(v)) for 0 <= v <= 2^30, in integers
inline int zone_isqrt(int v)
{
    int r = 0;
    for (int bit = 1 << 15; bit; bit >>= 1) {      // r + bit <= 65535: the square fits 64 bits with room
        const long long t = r + bit;
        if (t * t <= (long long)v)
            r += bit;
    }
    return r;
}

inline int zone_pixel_blocks(int height, int width)
{
    return (int)(((long long)height * width + kZoneThreads - 1) / kZoneThreads);      // <= 2^23
}

inline gs_status plan_zones(int height, int width, ZonePlan &out)
{
    out = ZonePlan();
    const gs_status st = check_zone_map("gs_instance_zones", height, width);
    if (st != GS_OK)
        return st;
    out.bands = (height + kZoneBand - 1) / kZoneBand;                 // <= 1024
    out.col_tiles = (width + kZoneThreads - 1) / kZoneThreads;        // <= 128
    out.band_blocks = out.bands * out.col_tiles;
    out.carry_blocks = out.col_tiles;
    out.pixel_blocks = zone_pixel_blocks(height, width);
    out.row_lds_bytes = width <= kZoneLdsCols ? (2 * width + 15) / 16 * 16 : 0;
    const size_t pixels = (size_t)height * (size_t)width, table = (size_t)out.bands * (size_t)width;
    PlanCursor ws;
    out.g_off = ws.take(pixels * 2);
    out.clab_off = ws.take(pixels * 4);
    out.top_d_off = ws.take(table * 2);
    out.bot_d_off = ws.take(table * 2);
    out.down_d_off = ws.take(table * 2);
    out.up_d_off = ws.take(table * 2);
    out.top_l_off = ws.take(table * 4);
    out.bot_l_off = ws.take(table * 4);
    out.down_l_off = ws.take(table * 4);
    out.up_l_off = ws.take(table * 4);
    out.bytes = ws.off;
    return GS_OK;
}

inline gs_status plan_foreign(int height, int width, ForeignPlan &out)
{
    out = ForeignPlan();
    const gs_status st = check_zone_map("gs_foreign_dist", height, width);
    if (st != GS_OK)
        return st;
    out.row_blocks = (height + kZoneThreads / 64 - 1) / (kZoneThreads / 64);
    out.pixel_blocks = zone_pixel_blocks(height, width);
    const size_t pixels = (size_t)height * (size_t)width;
    PlanCursor ws;
    out.left_off = ws.take(pixels * 2);
    out.right_off = ws.take(pixels * 2);
    out.bytes = ws.off;
    return GS_OK;
}

}  // namespace gs
