// What the host-only plans of the slide-map analyses (instance_plan.h, instance_match_plan.h, boundary_dist_plan.h) share: the
// refusals about sizes, each with the entry's name in front of its message, and the layout of a workspace as parts aligned to
// 256 bytes.  Host-only and free of HIP, as espnet_facts.h is: a plain C++17 compiler reads it, so the *_plan entries answer
// without a device and a sanitizer driver reaches every line.  A check returns GS_OK or sets the text and returns its status;
// the order of the checks is the plan's business.
#pragma once
#include <climits>
#include <cstddef>

#include "espnet_facts.h"

namespace gs {

constexpr size_t kPlanAlign = 256;   // every part of a workspace starts at a multiple of it
inline size_t plan_align(size_t v) { return (v + kPlanAlign - 1) / kPlanAlign * kPlanAlign; }

// A uint16 link table of a row pass (bdist_rows_kernel, foreign_rows_kernel) holds a column, below the 32768 a plan allows a side,
// or this: no boundary pixel on that side of the row.
constexpr int kLinkNone = 0xFFFF;

// The parts of a workspace one behind the other: take(n) is the offset of a part of n bytes, and `off`, when all are taken, the
// size of the whole.
struct PlanCursor {
    size_t off = 0;
    size_t take(size_t bytes)
    {
        const size_t at = off;
        off += plan_align(bytes);
        return at;
    }
};

inline gs_status check_map_sides(const char *entry, int height, int width)
{
    if (height > 0 && width > 0)
        return GS_OK;
    set_error("%s: height and width must be positive (got %d x %d)", entry, height, width);
    return GS_ERR_INVALID;
}

// a linear pixel index is an int32
inline gs_status check_map_pixels(const char *entry, int height, int width)
{
    if ((long long)height * (long long)width <= (long long)INT_MAX)
        return GS_OK;
    set_error("%s: a map of %d x %d has more than 2^31 - 1 pixels", entry, height, width);
    return GS_ERR_UNSUPPORTED;
}

inline gs_status check_map_classes(const char *entry, int classes)
{
    if (classes >= 2 && classes <= GS_MAX_CLASSES)
        return GS_OK;
    set_error("%s: classes must be 2..%d (got %d)", entry, GS_MAX_CLASSES, classes);
    return GS_ERR_INVALID;
}

inline gs_status check_instance_counts(const char *entry, int n_gt, int n_pred)
{
    if (n_gt >= 0 && n_pred >= 0)
        return GS_OK;
    set_error("%s: n_gt and n_pred must not be negative (got %d, %d)", entry, n_gt, n_pred);
    return GS_ERR_INVALID;
}

}  // namespace gs
