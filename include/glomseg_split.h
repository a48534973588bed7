/*
 * glomseg_split.h -- splitting touching glomeruli: the exact Euclidean distance map of the foreground of a label map, the peak of
 * an int32 map over every label (with the distance map: the maximal inscribed circle of every instance), and the power cut that
 * separates the parts of an instance that holds several cores (an addition to glomseg.h; the ABI number stays 10: no signature
 * changes, and a caller finds out whether a library has these six entries by looking the symbols up).
 *
 * Pixel (x, y) is the point (x, y); its linear index is pos = y * width + x.  Everything outside the map is background.  labels:
 * int32 [height,width] as gs_slide_instances writes them; a label below 1 or above n is background and is never indexed through.
 * Everything is integer and exact.
 *   distance map d2[p] = 0 where labels[p] is not in 1..n; otherwise the smallest dx*dx + dy*dy from p to any pixel that is
 *                background or lies outside the map.  So a pixel in column x has d2 <= (x+1)^2 and <= (width-x)^2, and likewise
 *                for rows.  With both sides at most 32768 a d2 is at most 16384^2 = 2^28, below 2^29: d2 is an int32.
 *   peaks        for labels 1..n and an int32 value map: peak_value[i-1] = the largest value over the pixels of i, peak_pos[i-1]
 *                = the smallest pos that attains it; a label without pixels gives peak_value = INT32_MIN and peak_pos = -1.  With
 *                the d2 map the peak of an instance is its maximal inscribed circle: centre peak_pos, radius sqrt(peak_value).
 *   cores        (the caller's part) the connected components of d2 > core_d2, labelled by gs_slide_instances with classes = 2;
 *                the peaks of the core labels over d2 give each core's centre core_pos and squared radius core_r2.  A core the
 *                caller drops has core_pos = -1.
 *   valid core   core k (1..c) is valid iff 0 <= core_pos[k-1] < height * width and the label at that position is in 1..n: that
 *                label is its owner.
 *   cores_per_instance[i-1] = the number of valid cores owned by i: the true count, whatever max_cores is.
 *   parts[p]     0 where labels[p] is not in 1..n or where the owner's count is < 2 or > max_cores; otherwise the valid core k of
 *                labels[p] that minimises ((x-cx_k)^2 + (y-cy_k)^2 - core_r2[k-1], k) lexicographically, compared in int64
 *                (core_r2 is any int32).  This is a power diagram: between two overlapping discs the boundary is the line through
 *                the circles' two intersection points (the radical axis); an exact tie goes to the lower core id.
 *   out_map[p]   0 where parts[p] > 0 and some 8-neighbour q inside the map has labels[q] == labels[p] and parts[q] > parts[p];
 *                everywhere else class_map[p].  The 8-neighbour rule holds for both connectivities: after it no two remaining
 *                pixels of different parts of one instance are 8-adjacent.
 *   cut_pixels   the number of pixels the rule hits.
 * A map in which no instance has two valid cores comes back byte-identical.  An instance of more than max_cores cores (2..1024;
 * the bound of the per-pixel loop) is no pair of touching glomeruli and is left whole.
 * Sides above 32768 and maps of more than 2^31 - 1 pixels are refused.
 *
 * Kernels and their safety rules: csrc/split.hip.  The caller's side (cores, inscribed circles, the command line):
 * glomeruli_segmentation_amd/split.py.
 */
#ifndef GLOMSEG_SPLIT_H
#define GLOMSEG_SPLIT_H

#include "glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only: the bytes of workspace of the three entries below.  Each refuses what its entry refuses about sizes: non-positive
 * height / width, a negative n or c, a NULL bytes (GS_ERR_INVALID); height > 32768, width > 32768 or height * width > 2^31 - 1
 * (GS_ERR_UNSUPPORTED).  No figure ever shrinks when an argument grows. */
gs_status gs_edt_plan(int height, int width, size_t *bytes);
gs_status gs_label_peaks_plan(int n, size_t *bytes);
gs_status gs_split_plan(int height, int width, int n, int c, size_t *bytes);

/* The three entries: stream-ordered, no host wait, no allocation, capturable.  All pointers device; labels, values, parts, d2:
 * int32 [height,width], contiguous, 4-byte aligned; class_map, out_map: uint8 [height,width], contiguous.  workspace: at least
 * the plan's bytes, 8-byte aligned; its contents on entry do not matter.  Every output byte is written on every call.
 * GS_ERR_INVALID before any device work: what the plan refuses (sizes: GS_ERR_UNSUPPORTED as there), a NULL or misaligned required
 * pointer, a workspace smaller than the plan, max_cores outside 2..1024. */

/* d2 of the foreground labels in 1..n.  n == 0 is legal: d2 = 0 throughout. */
gs_status gs_foreground_edt(const int32_t *labels, int n, int height, int width, void *workspace, size_t workspace_bytes, int32_t *d2,
                            void *hip_stream);

/* peak_value, peak_pos: int32 [n], 4-byte aligned; with n == 0 both may be NULL and nothing is written. */
gs_status gs_label_peaks(const int32_t *labels, const int32_t *values, int n, int height, int width, void *workspace,
                         size_t workspace_bytes, int32_t *peak_value, int32_t *peak_pos, void *hip_stream);

/* core_pos, core_r2: int32 [c] (NULL with c == 0); cores_per_instance: int32 [n] (NULL with n == 0); cut_pixels: int64 [1], 8-byte
 * aligned.  out_map must not be class_map. */
gs_status gs_split_cut(const uint8_t *class_map, const int32_t *labels, int n, const int32_t *core_pos, const int32_t *core_r2, int c,
                       int max_cores, int height, int width, void *workspace, size_t workspace_bytes, int32_t *parts, uint8_t *out_map,
                       int32_t *cores_per_instance, long long *cut_pixels, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOMSEG_SPLIT_H */
