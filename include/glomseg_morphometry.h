/*
 * glomseg_morphometry.h -- per-glomerulus morphometry: the exact integer shape sums of every instance of a label map and its
 * maximum Feret (caliper) diameter, squared, on the device where gs_slide_instances (glomseg_instances.h) leaves the label map and
 * the boxes (an addition to glomseg.h; the ABI number stays 10: no signature changes, and a caller finds out whether a library has
 * these two entries by looking the symbols up).
 *
 * labels: int32 [height,width]; boxes: int32 [n,4] (xmin, ymin, xmax, ymax, half-open), both as gs_slide_instances writes them.
 * A label below 1 or above n is background (gs_slide_instances writes ids beyond its cap into `labels`): such a pixel belongs to
 * no instance and is never indexed through.  Pixel (x, y) is the point (x, y).  Everything is integer.
 *   stats[i-1]   ten unsigned 64-bit sums over the pixels with labels == i, wherever they lie:
 *                  0        A    the number of pixels
 *                  1, 2     Sx, Sy         the sums of x and of y (map coordinates)
 *                  3, 4, 5  Sxx, Syy, Sxy  the sums of x*x, y*y and x*y
 *                  6..9     Q1, Q2, QD, Q3 Gray's bit-quad counts of the mask labels == i
 *   bit quads    the (height+1) x (width+1) windows of 2 x 2 pixels whose lower-right pixel is (x, y), 0 <= x <= width,
 *                0 <= y <= height; everything outside the map is background.  Q1: windows with exactly one pixel of i; Q3: with
 *                exactly three; QD: with exactly two, on a diagonal; Q2: with exactly two that share an edge.  Windows with four are
 *                not stored: Q4 = (4A - Q1 - 2 Q2 - 2 QD - 3 Q3) / 4.  A window can hold up to four different instances and counts
 *                once for each.
 *   feret2[i-1]  the largest dy*dy + dx*dx over all pairs of pixels of instance i INSIDE ITS DECLARED BOX: the maximum Feret
 *                diameter, squared; 0 for a single pixel, and 0 for a valid box that holds no pixel of i.  A box that is empty or
 *                does not lie within the map gives -1.  A pixel of i outside its box is left out of feret2 only: stats counts it.
 *   rows_needed  the sum of ymax - ymin over the valid boxes: the rows of the row table (the smallest and the largest x of every
 *                instance in every row of its box), which lives in the workspace.  If it exceeds rows_cap every feret2 becomes
 *                -1, stats is still complete and the status is GS_OK: the caller retries with a larger cap, the pattern of `cap`
 *                in gs_slide_instances.
 * With both sides of a map at most 32768 pixels a feret2 is at most 2 * 32767^2 = 2147352578 < 2^31, so it is an int32, and with
 * at most 2^31 - 1 pixels Sxx < 2^31 * 2^30 = 2^61: no sum overflows.  Larger maps are refused.
 *
 * Kernels and their safety rules: csrc/morphometry.hip.  The measures that follow from the sums (centroid, axes, perimeter,
 * holes, ...): glomeruli_segmentation_amd/instances.py, morphometry().
 */
#ifndef GLOMSEG_MORPHOMETRY_H
#define GLOMSEG_MORPHOMETRY_H

#include "glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only: the bytes of workspace gs_instance_morphometry needs.  It refuses what that entry refuses about sizes: non-positive
 * height / width, a negative rows_cap and a NULL workspace_bytes (GS_ERR_INVALID); height > 32768, width > 32768 or
 * height * width > 2^31 - 1 (GS_ERR_UNSUPPORTED).  The figure never shrinks with height * width nor with rows_cap. */
gs_status gs_morphometry_plan(int height, int width, long long rows_cap, size_t *workspace_bytes);

/* The sums and the diameters.  Stream-ordered, no host wait, no allocation, capturable.  All pointers device.
 *   labels       int32 [height,width], contiguous, 4-byte aligned
 *   boxes        int32 [n,4], 4-byte aligned; any content: nothing is read or written out of bounds
 *   workspace    at least gs_morphometry_plan's bytes for this rows_cap, 8-byte aligned; its contents on entry do not matter
 *   stats        uint64 [n,10], 8-byte aligned
 *   feret2       int32 [n], 4-byte aligned
 *   rows_needed  int64 [1], 8-byte aligned
 * Every row of stats and every element of feret2 and rows_needed is written on every call.  With n == 0 the stats, feret2 and
 * boxes pointers may be NULL, and only rows_needed = 0 is written.
 * GS_ERR_INVALID before any device work: what gs_morphometry_plan refuses (sizes: GS_ERR_UNSUPPORTED as there), a negative n, a
 * NULL or misaligned required pointer, a workspace smaller than the plan. */
gs_status gs_instance_morphometry(const int32_t *labels, const int32_t *boxes, int n, int height, int width, void *workspace,
                                  size_t workspace_bytes, long long rows_cap, unsigned long long *stats, int32_t *feret2,
                                  long long *rows_needed, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOMSEG_MORPHOMETRY_H */
