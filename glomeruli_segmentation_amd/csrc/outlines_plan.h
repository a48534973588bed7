// Workspace plan of gs_instance_outlines (csrc/outlines.hip): what the entry refuses about sizes, the grids of its launches, the
// number of pointer-jumping rounds and where the parts of the caller's workspace lie.  Host-only and free of HIP
// (slide_map_plan.h, which has the shared refusals and the layout): gs_outlines_plan (outlines_abi.h) answers without a device,
// and the launcher lays the workspace out with the same function.
//
// The workspace is a function of height * width and edges_cap: four bytes per pixel (the dense index of a pixel's first edge),
// 53 bytes per edge of the cap (its pixel, its side, two jumping states and its row in loop order) and the block counts of the
// scans.  The rounds are fixed here, from edges_cap alone: a loop has at most edges_cap edges where the result fits, and after
// r rounds every edge has seen the next 2^r edges of its loop, so r is the smallest number with 2^r >= edges_cap.
#pragma once
#include "slide_map_plan.h"

namespace gs {

constexpr int kOutThreads = 256;                // threads of every launch but the scans: four waves, one pixel or edge per thread
constexpr long long kOutMaxEdges = INT_MAX;     // a dense edge index is an int32

// One edge's state of the pointer jumping, and the first state (round 0): the window is the edge itself.  16 bytes, one load.
struct alignas(16) OutState {
    int min;                   // the smallest dense index among the next 2^k edges of the loop, this one included
    int off;                   // the steps from this edge to the first of them that has it
    int jump;                  // the edge 2^k steps ahead
    int succ;                  // the edge one step ahead, carried along
};
static_assert(sizeof(OutState) == 16, "the plan counts 16 bytes a state");

// What a loop's key edge leaves for the edges of its loop, in the state buffer the last round did not write.  16 bytes.
struct alignas(16) OutLoop {
    int loop;                  // the loop's number
    int base;                  // its first row of the edges in loop order
    int len;                   // its edges
    int pad;
};
static_assert(sizeof(OutLoop) == sizeof(OutState), "a loop's row lies where a state lay");

// An edge in loop order: its end vertex where that is a corner (x = -1 where not), and the loop's number in its key edge's row.
struct alignas(16) OutRow {
    int x, y;
    int loop;                  // the number of the loop that begins here, or -1
    int pad;
};
static_assert(sizeof(OutRow) == 16, "the plan counts 16 bytes a row");

// What the scans leave for the later launches.  One part of the workspace.
struct OutHead {
    long long edges_needed;
    int fits;                  // edges_needed <= edges_cap
    int n_loops;
    int n_points;
    int pad;
};

struct OutlinesPlan {
    int n_pixels = 0;          // height * width <= INT_MAX
    int edges_cap = 0;
    int rounds = 0;            // launches of the jumping kernel: the smallest r with 2^r >= edges_cap
    int pixel_blocks = 0;      // workgroups of the pixel launches
    int edge_blocks = 0;       // workgroups of the edge launches: at least one
    size_t head_off = 0;       // OutHead
    size_t pixel_count_off = 0;    // int32 [pixel_blocks]: edges per block, then (scanned in place) edges in front of the block
    size_t pixel_base_off = 0;     // int32 [n_pixels]: the dense index of the pixel's first edge
    size_t edge_pixel_off = 0;     // int32 [edges_cap]
    size_t edge_side_off = 0;      // uint8 [edges_cap]
    size_t count_a_off = 0;        // int32 [edge_blocks]: key edges per block, later corners per block
    size_t count_b_off = 0;        // int32 [edge_blocks]: edges of the loops whose key edge lies in the block
    size_t state_off[2] = {0, 0};  // OutState [edges_cap] each
    size_t row_off = 0;            // OutRow [edges_cap]
    size_t bytes = 0;
};

// the smallest r with 2^r >= edges: 0 for 0 and 1, 31 for 2^31 - 1
constexpr int outline_rounds(long long edges)
{
    int r = 0;
    while ((1ll << r) < edges)
        ++r;
    return r;
}

inline gs_status plan_outlines(int height, int width, long long edges_cap, OutlinesPlan &out)
{
    out = OutlinesPlan();
    const char *entry = "gs_instance_outlines";
    gs_status st;
    if ((st = check_map_sides(entry, height, width)) != GS_OK)
        return st;
    if (edges_cap < 0) {
        set_error("%s: edges_cap must not be negative (got %lld)", entry, edges_cap);
        return GS_ERR_INVALID;
    }
    if (edges_cap > kOutMaxEdges) {
        set_error("%s: edges_cap must be at most 2^31 - 1 (got %lld): a dense edge index is an int32", entry, edges_cap);
        return GS_ERR_INVALID;
    }
    if ((st = check_map_pixels(entry, height, width)) != GS_OK)
        return st;
    out.n_pixels = height * width;
    out.edges_cap = (int)edges_cap;
    out.rounds = outline_rounds(edges_cap);
    out.pixel_blocks = (out.n_pixels - 1) / kOutThreads + 1;
    out.edge_blocks = edges_cap ? (int)((edges_cap - 1) / kOutThreads + 1) : 1;
    PlanCursor ws;
    out.head_off = ws.take(sizeof(OutHead));
    out.pixel_count_off = ws.take((size_t)out.pixel_blocks * sizeof(int));
    out.pixel_base_off = ws.take((size_t)out.n_pixels * sizeof(int));
    out.edge_pixel_off = ws.take((size_t)edges_cap * sizeof(int));
    out.edge_side_off = ws.take((size_t)edges_cap);
    out.count_a_off = ws.take((size_t)out.edge_blocks * sizeof(int));
    out.count_b_off = ws.take((size_t)out.edge_blocks * sizeof(int));
    out.state_off[0] = ws.take((size_t)edges_cap * sizeof(OutState));
    out.state_off[1] = ws.take((size_t)edges_cap * sizeof(OutState));
    out.row_off = ws.take((size_t)edges_cap * sizeof(OutRow));
    out.bytes = ws.off;
    return GS_OK;
}

}  // namespace gs
