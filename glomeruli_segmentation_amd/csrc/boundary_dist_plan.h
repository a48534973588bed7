// Workspace plan of gs_instance_boundary_dist (csrc/boundary_dist.hip): what the entry refuses about sizes and where the four
// link tables lie in the caller's workspace.  Host-only and free of HIP (espnet_facts.h), as instance_match_plan.h is:
// gs_boundary_dist_plan (include/glomseg_boundary_dist.h) answers without a device, and the launcher lays the workspace out with
// the same function.
#pragma once
#include <climits>
#include <cstddef>

#include "espnet_facts.h"

namespace gs {

constexpr int kBdistThreads = 256;          // threads of every launch: four waves
constexpr size_t kBdistAlign = 256;
constexpr int kBdistMaxSide = 32768;        // a column fits a uint16 beside the "none" word, and 2 * 32767^2 < 2^31: d2 is an int32
constexpr unsigned short kBdistNone = 0xFFFF;

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

inline size_t bdist_align(size_t v) { return (v + kBdistAlign - 1) / kBdistAlign * kBdistAlign; }

inline gs_status plan_boundary_dist(int height, int width, BoundaryDistPlan &out)
{
    out = BoundaryDistPlan();
    if (height <= 0 || width <= 0) {
        set_error("gs_instance_boundary_dist: height and width must be positive (got %d x %d)", height, width);
        return GS_ERR_INVALID;
    }
    if (height > kBdistMaxSide || width > kBdistMaxSide) {
        set_error("gs_instance_boundary_dist: maps of %d x %d have a side above %d: a squared distance need not fit an int32", height,
                  width, kBdistMaxSide);
        return GS_ERR_UNSUPPORTED;
    }
    if ((long long)height * (long long)width > (long long)INT_MAX) {
        set_error("gs_instance_boundary_dist: maps of %d x %d have more than 2^31 - 1 pixels", height, width);
        return GS_ERR_UNSUPPORTED;
    }
    out.n_pixels = height * width;
    out.row_blocks = (2 * height - 1) / (kBdistThreads / 64) + 1;
    out.pixel_blocks = (out.n_pixels - 1) / kBdistThreads + 1;
    const size_t table = bdist_align((size_t)out.n_pixels * sizeof(unsigned short));
    out.left_gt_off = 0;
    out.right_gt_off = table;
    out.left_pred_off = 2 * table;
    out.right_pred_off = 3 * table;
    out.bytes = 4 * table;
    return GS_OK;
}

// What gs_instance_boundary_dist refuses about its counts (the pointers are the entry's business).
inline gs_status check_boundary_dist(int n_gt, int n_pred)
{
    if (n_gt < 0 || n_pred < 0) {
        set_error("gs_instance_boundary_dist: n_gt and n_pred must not be negative (got %d, %d)", n_gt, n_pred);
        return GS_ERR_INVALID;
    }
    return GS_OK;
}

}  // namespace gs
