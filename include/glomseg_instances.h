/*
 * glomseg_instances.h -- the per-glomerulus table of a slide map: connected components of the composited 1/8 class map, on the
 * device where the compositor leaves it (an addition to glomseg.h; the ABI number stays 10: no signature of glomseg.h changes, and
 * a caller finds out whether a library has these two entries by looking the symbols up).
 *
 * The reference stops at per-crop pixel counts (module/tools/area_stats.py: one row per detector box).  A box can hold two
 * glomeruli, overlapping boxes count one glomerulus twice and a box edge cuts one in part; max-compositing into the slide map
 * has resolved all of that, so the instances are read from the map:
 *   foreground   map >= 1 (the glomerulus outline of module/common/boundary_extractor.py:27)
 *   instance     a connected component of the foreground, 8-connected (or 4)
 *   numbering    1..n by the raster position y * width + x of the component's first pixel: scipy.ndimage.label's numbering
 * Everything is integer arithmetic: the result is exact, order included.  Kernels and their safety rules: csrc/instances.hip.
 */
#ifndef GLOMSEG_INSTANCES_H
#define GLOMSEG_INSTANCES_H

#include "glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only: the bytes of workspace gs_slide_instances needs for a map of this size.  It refuses what that entry refuses about
 * sizes: non-positive height / width, classes outside 2..GS_MAX_CLASSES, cap < 1 (GS_ERR_INVALID, a NULL workspace_bytes too),
 * height * width > 2^31 - 1 (GS_ERR_UNSUPPORTED).  The figure grows with height * width and never shrinks with cap (counts and
 * boxes accumulate in the caller's outputs: nothing of cap's size lives in the workspace). */
gs_status gs_instances_plan(int height, int width, int classes, int cap, size_t *workspace_bytes);

/* Stream-ordered, no host wait, no allocation, capturable.  All pointers device.
 *   class_map  uint8 [height,width], contiguous, base 4-byte aligned, any width
 *   connectivity  4 or 8
 *   workspace  at least gs_instances_plan's bytes, 4-byte aligned; its contents on entry do not matter
 *   boxes      int32  [cap,4]  xmin, ymin, xmax, ymax in map pixels, half-open (as gs_eval_box)
 *   counts     uint64 [cap,classes]  counts[i][c] = pixels of class c in instance i+1; column 0 holds the component's bytes
 *              >= classes (0 for any map a forward wrote: the rule gs_crops_from_masks has)
 *   labels     int32 [height,width] or NULL: 0 = background, else the instance id 1..n (ids beyond cap included)
 *   n_found    int32 [1]: the number of components, whatever cap is
 * Rows [min(n_found,cap), cap) of boxes / counts are not written.  More components than cap is not an error.
 * GS_ERR_INVALID before any device work: a connectivity other than 4 or 8, what gs_instances_plan refuses, a NULL or misaligned
 * class_map / workspace, a NULL boxes / counts / n_found, a workspace smaller than the plan. */
gs_status gs_slide_instances(const uint8_t *class_map, int height, int width, int classes, int connectivity, void *workspace,
                             size_t workspace_bytes, int cap, int32_t *boxes, unsigned long long *counts, int32_t *labels,
                             int32_t *n_found, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOMSEG_INSTANCES_H */
