/*
 * glomseg_instance_match.h -- per-glomerulus scoring against ground truth: the overlap table of two labelled slide maps and
 * the matching on it, on the device where gs_slide_instances (glomseg_instances.h) leaves labels and counts (an addition to
 * glomseg.h; the ABI number stays 10: no signature changes, and a caller finds out whether a library has these three entries
 * by looking the symbols up).
 *
 * G, P: the two class maps, uint8 [height,width] (ground truth, prediction).  LG, LP: their label maps, int32, 0 = background,
 * ids 1..n; counts_gt, counts_pred: their class histograms -- all three exactly what gs_slide_instances writes.
 *   overlap pair (g,p)   g >= 1, p >= 1 and some pixel has LG == g and LP == p
 *   inter(g,p)           the number of such pixels;  agree(g,p): those of them where G == P (the same class byte)
 *   area                 the sum of an instance's row of counts;  union = area_g + area_p - inter
 *   match                inter * den > num * union, the threshold num / den with 1 <= num <= den <= 65535 and 2 * num >= den
 *                        (every product stays below 2^48: uint64 arithmetic, no overflow)
 *   order                pairs are listed ascending by (g, p)
 * Everything is integer arithmetic: the result is exact, order included.
 *
 * A match is unique, so there is no assignment problem and no tie-break.  Proof: a match has inter * den > num * union and
 * 2 * num >= den, so 2 * inter > union >= area_g: p holds more than half of g's pixels.  Two predictions are disjoint sets of
 * pixels, so no second one can hold more than half of g as well; by union >= area_p the same holds with the sides swapped.
 * Below 1/2 this fails, and such thresholds are refused.
 *
 * Kernels and their safety rules: csrc/instance_match.hip.
 */
#ifndef GLOMSEG_INSTANCE_MATCH_H
#define GLOMSEG_INSTANCE_MATCH_H

#include "glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only: the bytes of workspace gs_instance_overlaps needs.  It refuses what that entry refuses about sizes: non-positive
 * height / width, pair_cap < 1 (GS_ERR_INVALID, a NULL workspace_bytes too), height * width > 2^31 - 1 (GS_ERR_UNSUPPORTED).
 * The figure never shrinks with pair_cap nor with height * width (it stops growing with pair_cap at height * width: two maps
 * have no more distinct pairs than pixels). */
gs_status gs_instance_match_plan(int height, int width, int pair_cap, size_t *workspace_bytes);

/* The overlap table.  Stream-ordered, no host wait, no allocation, capturable.  All pointers device.
 *   labels_gt, labels_pred  int32 [height,width], contiguous, 4-byte aligned; a pixel with a label < 1 on either side is skipped
 *   map_gt, map_pred        uint8 [height,width], contiguous, 4-byte aligned, any width
 *   workspace   at least gs_instance_match_plan's bytes, 8-byte aligned; its contents on entry do not matter
 *   pairs       int32  [pair_cap,2]  gt id, pred id; ascending by (gt id, pred id)
 *   inter       uint64 [pair_cap,2]  inter, agree
 *   n_pairs     int32  [2]  the number of distinct pairs stored; overflow 0 / 1
 * Rows [n_pairs[0], pair_cap) of pairs / inter are not written.
 * Overflow: with more distinct pairs than pair_cap the call still returns GS_OK and n_pairs becomes {0, 1}; no row is written
 * then, nothing is written out of bounds, and the work stays bounded (the pixel pass stops inserting once it has seen the
 * overflow word).  With n_pairs[1] == 0 the result is exact and complete.
 * GS_ERR_INVALID before any device work: what gs_instance_match_plan refuses, a NULL or misaligned pointer, a workspace smaller
 * than the plan. */
gs_status gs_instance_overlaps(const int32_t *labels_gt, const int32_t *labels_pred, const uint8_t *map_gt, const uint8_t *map_pred,
                               int height, int width, void *workspace, size_t workspace_bytes, int pair_cap, int32_t *pairs,
                               unsigned long long *inter, int32_t *n_pairs, void *hip_stream);

/* The matching on the table.  Stream-ordered, no host wait, no allocation, capturable.  All pointers device.
 *   pairs, inter, n_pairs   what gs_instance_overlaps wrote with this pair_cap
 *   counts_gt   uint64 [n_gt,classes], counts_pred uint64 [n_pred,classes]: gs_slide_instances' counts of the two maps
 *   match_gt    int32 [n_gt]    the matched pred id or 0
 *   match_pred  int32 [n_pred]  the matched gt id or 0
 * n_gt == 0 or n_pred == 0 is valid: nothing is launched for that side (its pointers may be NULL) and the other side's array
 * becomes all zero.  With n_pairs[1] == 1 both arrays become all zero.  A pair with an id outside 1..n_gt / 1..n_pred is
 * skipped, never stored through.
 * GS_ERR_INVALID before any device work: pair_cap < 1, a negative n_gt / n_pred, classes outside 2..GS_MAX_CLASSES, a threshold
 * outside the range above, a NULL or misaligned pointer. */
gs_status gs_instance_match(const int32_t *pairs, const unsigned long long *inter, const int32_t *n_pairs, int pair_cap,
                            const unsigned long long *counts_gt, int n_gt, const unsigned long long *counts_pred, int n_pred,
                            int classes, int iou_num, int iou_den, int32_t *match_gt, int32_t *match_pred, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOMSEG_INSTANCE_MATCH_H */
