// Workspace plan of gs_instance_boundary_dist (csrc/boundary_dist.hip): what the entry refuses about sizes and where the four
// link tables lie in the caller's workspace.  Host-only and free of HIP (slide_map_plan.h, which has the shared refusals and
// the layout): gs_boundary_dist_plan (include/glomseg_boundary_dist.h) answers without a device, and the launcher lays the
// workspace out with the same function.
#pragma once
#include "slide_map_plan.h"

namespace gs {

constexpr int kBdistThreads = 256;          // threads of every launch: four waves
constexpr int kBdistMaxSide = 32768;        // a column fits a uint16 beside the "none" word, and 2 * 32767^2 < 2^31: d2 is an int32
constexpr unsigned short kBdistNone = 0xFFFF;
static_assert(kBdistNone == kLinkNone, "the link tables of every row pass end in one sentinel");

struct BoundaryDistPlan {
    int n_pixels = 0;          // height * width <= INT_MAX
    int row_blocks = 0;        // the row pass: a wave per (row, side) -> ceil(2 * height / 4) workgroups (<= 16384)
    int pixel_blocks = 0;      // the query pass: a lane per pixel -> ceil(n_pixels / 256) workgroups (<= 2^23)
    size_t left_gt_off = 0;    // uint16 [height,width]: the column of the nearest boundary pixel of LG at or left of x, or none
    size_t right_gt_off = 0;   // ... at or right of x
    size_t left_pred_off = 0;  // the same two of LP
    size_t right_pred_off = 0;
    size_t bytes = 0;
};

inline gs_status plan_boundary_dist(int height, int width, BoundaryDistPlan &out)
{
    out = BoundaryDistPlan();
    const char *entry = "gs_instance_boundary_dist";
    gs_status st;
    if ((st = check_map_sides(entry, height, width)) != GS_OK)
        return st;
    if (height > kBdistMaxSide || width > kBdistMaxSide) {
        set_error("%s: maps of %d x %d have a side above %d: a squared distance need not fit an int32", entry, height, width,
                  kBdistMaxSide);
        return GS_ERR_UNSUPPORTED;
    }
    // after the side limit, which at 2^30 pixels leaves it nothing to refuse: n_pixels <= INT_MAX (2^31 - 1) is then checked
    // in this function and does not rest on kBdistMaxSide
    if ((st = check_map_pixels(entry, height, width)) != GS_OK)
        return st;
    out.n_pixels = height * width;
    out.row_blocks = (2 * height - 1) / (kBdistThreads / 64) + 1;
    out.pixel_blocks = (out.n_pixels - 1) / kBdistThreads + 1;
    const size_t table = (size_t)out.n_pixels * sizeof(unsigned short);
    PlanCursor ws;
    out.left_gt_off = ws.take(table);
    out.right_gt_off = ws.take(table);
    out.left_pred_off = ws.take(table);
    out.right_pred_off = ws.take(table);
    out.bytes = ws.off;
    return GS_OK;
}

}  // namespace gs
