// Workspace plan of gs_slide_instances (csrc/instances.hip): what the entry refuses about sizes, how the map is cut into tiles
// and counting blocks, and where `parent` and the block counts lie in the caller's workspace.  Host-only and free of HIP
// (slide_map_plan.h, which has the shared refusals and the layout): gs_instances_plan (include/glomseg_instances.h) answers
// without a device, and the launcher lays the workspace out with the same function.
#pragma once
#include "slide_map_plan.h"

namespace gs {

constexpr int kInstTileW = 64, kInstTileH = 16;   // the local pass's tile: 1024 pixels, one int32 of LDS each
constexpr int kInstThreads = 256;                 // threads of every launch; the pixel passes take one pixel per thread

struct InstancePlan {
    int n_pixels = 0;          // height * width <= INT_MAX: a linear index is an int32
    int tiles_x = 0, tiles_y = 0;
    int n_blocks = 0;          // counting blocks of kInstThreads pixels in raster order
    size_t parent_off = 0;     // int32 [n_pixels]
    size_t block_off = 0;      // int32 [n_blocks]: roots per block, then (scanned in place) roots in front of the block
    size_t bytes = 0;
};

inline gs_status plan_instances(int height, int width, int classes, int cap, InstancePlan &out)
{
    out = InstancePlan();
    const char *entry = "gs_slide_instances";
    gs_status st;
    if ((st = check_map_sides(entry, height, width)) != GS_OK || (st = check_map_classes(entry, classes)) != GS_OK)
        return st;
    if (cap < 1) {
        set_error("%s: cap must be at least 1 (got %d)", entry, cap);
        return GS_ERR_INVALID;
    }
    if ((st = check_map_pixels(entry, height, width)) != GS_OK)
        return st;
    out.n_pixels = height * width;
    out.tiles_x = (width - 1) / kInstTileW + 1;     // (no width + 63: a width near INT_MAX is allowed)
    out.tiles_y = (height - 1) / kInstTileH + 1;
    out.n_blocks = (out.n_pixels - 1) / kInstThreads + 1;
    PlanCursor ws;
    out.parent_off = ws.take((size_t)out.n_pixels * sizeof(int));
    out.block_off = ws.take((size_t)out.n_blocks * sizeof(int));
    out.bytes = ws.off;
    return GS_OK;
}

}  // namespace gs
