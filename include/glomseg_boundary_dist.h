/*
 * glomseg_boundary_dist.h -- boundary distances of matched glomeruli: for every matched pair of gs_instance_match
 * (glomseg_instance_match.h) the exact squared distance from each boundary pixel of one instance to the boundary of its partner,
 * in both directions, on the device where gs_slide_instances leaves the label maps and gs_instance_match the match arrays (an
 * addition to glomseg.h; the ABI number stays 10: no signature changes, and a caller finds out whether a library has these two
 * entries by looking the symbols up).
 *
 * LG, LP: the two label maps, int32 [height,width] (ground truth, prediction); match_gt int32 [n_gt], match_pred int32 [n_pred]:
 * what gs_instance_match writes.  Everything is integer.
 *   boundary pixel   of instance i in a label map L: a pixel with L == i that has at least one of its four edge neighbours outside
 *                    the map or with L != i.  The rule is 4-neighbour whatever connectivity labelled the map; the border of a
 *                    hole counts, and so does the map's edge (mask & ~binary_erosion(mask) with scipy's default structure and
 *                    border_value=0).  A label below 1 or above n_gt / n_pred is background here (gs_slide_instances writes ids
 *                    beyond its cap into `labels`): such a pixel is no boundary pixel and is never indexed through.
 *   pair             gt instance g and pred instance p are a pair iff 1 <= p <= n_pred, match_gt[g-1] == p and
 *                    match_pred[p-1] == g.  Anything else is unmatched, and is never indexed through.
 *   d2(x, S)         the minimum over s in S of dy*dy + dx*dx.  S is the boundary of THE PARTNER INSTANCE ONLY, not of whichever
 *                    instance lies nearest.
 *   direction 0      every boundary pixel of g against the boundary of p;  direction 1: every boundary pixel of p against the
 *                    boundary of g.
 * With both sides of a map at most 32768 pixels every d2 is at most 2 * 32767^2 = 2147352578 < 2^31, so d2 is an int32; larger
 * maps are refused.  The Hausdorff distance of a pair is sqrt(max d2 over both directions); the percentile, the average surface
 * distance and the root mean square follow from the maps and the sums on the host (instance_eval.boundary_distances).
 *
 * Kernels and their safety rules: csrc/boundary_dist.hip.
 */
#ifndef GLOMSEG_BOUNDARY_DIST_H
#define GLOMSEG_BOUNDARY_DIST_H

#include "glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only: the bytes of workspace gs_instance_boundary_dist needs.  It refuses what that entry refuses about sizes:
 * non-positive height / width and a NULL workspace_bytes (GS_ERR_INVALID); height > 32768, width > 32768 or
 * height * width > 2^31 - 1 (GS_ERR_UNSUPPORTED: beyond them a d2 need not fit an int32 nor a column a uint16).  The figure never
 * shrinks with height * width. */
gs_status gs_boundary_dist_plan(int height, int width, size_t *workspace_bytes);

/* The distances.  Stream-ordered, no host wait, no allocation, capturable.  All pointers device.
 *   labels_gt, labels_pred  int32 [height,width], contiguous, 4-byte aligned
 *   match_gt    int32 [n_gt], match_pred int32 [n_pred], 4-byte aligned (may be NULL where the count is 0)
 *   workspace   at least gs_boundary_dist_plan's bytes, 8-byte aligned; its contents on entry do not matter
 *   dist_gt     int32 [height,width] or NULL: at a boundary pixel of a paired gt instance its d2 (direction 0), elsewhere -1
 *   dist_pred   int32 [height,width] or NULL: the same for the paired pred instances (direction 1)
 *   stats       uint64 [n_gt,2,3], 8-byte aligned (may be NULL where n_gt is 0): row g-1, direction, {boundary pixels, max d2,
 *               sum of d2}; the rows of an unmatched g are zero
 * Every element of a map that is given and every row of stats is written; either map being NULL changes nothing else.
 * n_gt == 0 or n_pred == 0 is valid: the maps become -1, stats zero, and nothing else is launched.
 * Inconsistent inputs: a pixel whose partner id occurs nowhere on the boundary of the other label map has no d2.  Its search ends
 * at the map's edges, it is stored as -1 and left out of stats; nothing is read or written out of bounds.
 * GS_ERR_INVALID before any device work: what gs_boundary_dist_plan refuses (sizes: GS_ERR_UNSUPPORTED as there), a negative
 * n_gt / n_pred, a NULL or misaligned required pointer, a workspace smaller than the plan. */
gs_status gs_instance_boundary_dist(const int32_t *labels_gt, const int32_t *labels_pred, const int32_t *match_gt, int n_gt,
                                    const int32_t *match_pred, int n_pred, int height, int width, void *workspace,
                                    size_t workspace_bytes, int32_t *dist_gt, int32_t *dist_pred, unsigned long long *stats,
                                    void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOMSEG_BOUNDARY_DIST_H */
