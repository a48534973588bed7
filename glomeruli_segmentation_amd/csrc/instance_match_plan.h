// Workspace plan of gs_instance_overlaps (csrc/instance_match.hip): what the entry refuses about sizes, the capacity of the
// pair table and where its parts lie in the caller's workspace.  Host-only and free of HIP (slide_map_plan.h, which has the
// shared refusals and the layout): gs_instance_match_plan (include/glomseg_instance_match.h) answers without a device, and the
// launcher lays the workspace out with the same function.
#pragma once
#include "slide_map_plan.h"

namespace gs {

constexpr int kMatchThreads = 256;          // threads of every launch; also the slots / pairs a counting block covers
constexpr size_t kMatchMinSlots = 256;      // one whole counting block at least
constexpr int kMatchTileW = 64, kMatchTileH = 64;   // the pixel pass's tile: one workgroup, a wave per row of 64 pixels at a time

struct InstanceMatchPlan {
    int n_pixels = 0;          // height * width <= INT_MAX
    int tiles_x = 0, tiles_y = 0;   // tiles_x * tiles_y <= n_pixels
    int cap = 0;               // min(pair_cap, n_pixels): a map has no more distinct pairs than pixels, so a larger pair_cap
                               // overflows in no case the smaller one does not, and the table need not be sized for it
    size_t slots = 0;          // a power of two >= 2 * cap (<= 2^32): the table is never more than half full without overflow
    int n_blocks = 0;          // slots / kMatchThreads (<= 2^24)
    size_t state_off = 0;      // uint32 [4]: distinct pairs claimed, overflow raised by the pixel pass; 16 bytes
    size_t key_off = 0;        // uint64 [slots]: (gt id << 32) | pred id, 0 = empty
    size_t val_off = 0;        // uint64 [slots,2]: inter, agree
    size_t block_off = 0;      // int32 [n_blocks]: occupied slots per block, then (scanned in place) those in front of it
    size_t dense_key_off = 0;  // uint64 [cap]: the occupied slots' keys, in slot order
    size_t dense_slot_off = 0; // uint32 [cap]: ... and their slots
    size_t bytes = 0;
};

inline gs_status check_pair_cap(const char *entry, int pair_cap)
{
    if (pair_cap >= 1)
        return GS_OK;
    set_error("%s: pair_cap must be at least 1 (got %d)", entry, pair_cap);
    return GS_ERR_INVALID;
}

inline gs_status plan_instance_match(int height, int width, int pair_cap, InstanceMatchPlan &out)
{
    out = InstanceMatchPlan();
    const char *entry = "gs_instance_overlaps";
    gs_status st;
    if ((st = check_map_sides(entry, height, width)) != GS_OK || (st = check_pair_cap(entry, pair_cap)) != GS_OK ||
        (st = check_map_pixels(entry, height, width)) != GS_OK)
        return st;
    out.n_pixels = height * width;
    out.tiles_x = (width - 1) / kMatchTileW + 1;      // (no width + 63: a width near INT_MAX is allowed)
    out.tiles_y = (height - 1) / kMatchTileH + 1;
    out.cap = pair_cap < out.n_pixels ? pair_cap : out.n_pixels;
    out.slots = kMatchMinSlots;
    while (out.slots < 2 * (size_t)out.cap)          // ends at 2^32 at the latest: 2 * cap < 2^32
        out.slots <<= 1;
    out.n_blocks = (int)(out.slots / kMatchThreads);
    PlanCursor ws;
    out.state_off = ws.take(4 * sizeof(unsigned));
    out.key_off = ws.take(out.slots * sizeof(unsigned long long));
    out.val_off = ws.take(out.slots * 2 * sizeof(unsigned long long));
    out.block_off = ws.take((size_t)out.n_blocks * sizeof(int));
    out.dense_key_off = ws.take((size_t)out.cap * sizeof(unsigned long long));
    out.dense_slot_off = ws.take((size_t)out.cap * sizeof(unsigned));
    out.bytes = ws.off;
    return GS_OK;
}

// What gs_instance_match refuses about its numbers (the pointers are the entry's business).
inline gs_status check_instance_match(int pair_cap, int n_gt, int n_pred, int classes, int iou_num, int iou_den)
{
    const char *entry = "gs_instance_match";
    gs_status st;
    if ((st = check_pair_cap(entry, pair_cap)) != GS_OK || (st = check_instance_counts(entry, n_gt, n_pred)) != GS_OK ||
        (st = check_map_classes(entry, classes)) != GS_OK)
        return st;
    if (iou_num < 1 || iou_den > 65535 || iou_num > iou_den || 2LL * iou_num < (long long)iou_den) {
        set_error("gs_instance_match: the threshold must be num / den with 1 <= num <= den <= 65535 and 2 * num >= den: below "
                  "1/2 a match is not unique (got %d / %d)", iou_num, iou_den);
        return GS_ERR_INVALID;
    }
    return GS_OK;
}

}  // namespace gs
