/*
 * outlines_abi.h -- the C declarations of the per-glomerulus outline entries of libglomseg.so (csrc/outlines.hip), in the style
 * of include/glomseg_morphometry.h.
 */
#ifndef GLOMSEG_OUTLINES_ABI_H
#define GLOMSEG_OUTLINES_ABI_H

#include "../../include/glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-glomerulus outlines on the device: for every instance of a label map (int32 [height,width], as gs_slide_instances of
 * glomseg_instances.h writes it) one closed loop of crack edges for its outer boundary and one for each of its holes, as lists of
 * lattice corner points in a fixed order.  Everything is integer.  The ABI number stays 10: no signature changes, and a caller
 * finds out whether a library has these two entries by looking the symbols up.
 * The two entries are exported by libglomseg.so and declared here, beside their sources, not under include/: the entry set
 * of every public header there is fixed.  glomeruli_segmentation_amd/outlines.py binds them (OUTLINE_ENTRIES).
 *   lattice     point (x, y) is the top-left corner of pixel (x, y), 0 <= x <= width, 0 <= y <= height; x to the right, y down.
 *   instances   a label below 1 or above n is background: such a pixel belongs to no instance and is never indexed through.
 *               "in i" means inside the map and labels == i.
 *   edges       a crack edge (p, s) of instance i: pixel p = y * width + x in i, side s (0 top, 1 right, 2 bottom, 3 left), the
 *               neighbour across that side not in i.  It is directed so that the instance lies to its right:
 *                 top     (x, y)     -> (x+1, y)     east        right   (x+1, y)   -> (x+1, y+1)   south
 *                 bottom  (x+1, y+1) -> (x, y+1)     west        left    (x, y+1)   -> (x, y)       north
 *               Its key is 4 * p + s.  A grid edge between two instances carries two directed edges, one for each; a map holds
 *               at most 4 * height * width edges.
 *   successor   at the end vertex of (p, s), A_R is the pixel ahead and to the right of the heading, A_L ahead and to the left
 *               (top edge of (x, y): A_R = (x+1, y), A_L = (x+1, y-1)).  Connectivity 8: A_L in i turns left, else A_R in i goes
 *               straight, else right.  Connectivity 4: A_R not in i turns right, else A_L in i left, else straight.  Left gives
 *               (A_L, (s + 3) % 4), straight (A_R, s), right (p, (s + 1) % 4).  The connectivity is the one the map was labelled
 *               with; the rule is well-formed, and one to one on the edges of an instance, for any labels and either value.
 *   loops       the cycles of the successor.  A loop's key edge is its edge of smallest key; loops are numbered 0..n_loops-1 by
 *               key, the raster order of their first edge.  loop_label is the instance, loop_first the pixel of the key edge,
 *               loop_edges the number of unit edges (the exact crack perimeter), loop_area2 the sum over the edges of
 *               sx * ey - ex * sy (start (sx, sy), end (ex, ey)): positive for an outer boundary, clockwise on screen, negative for
 *               a hole; the loop_area2 of an instance sum to twice its pixels.
 *   points      walk e0 (the key edge), e1 = its successor, ...: the end vertex of e_k is listed exactly when the side of e_k+1
 *               differs from the side of e_k, in order of k.  Only corners are stored: an even number, at least 4, per loop.
 *               loop_offsets[l] .. loop_offsets[l+1] indexes points, int32 [n_points,2] holding (x, y).
 * Kernels and their safety rules: csrc/outlines.hip.  Polygons, GeoJSON and labelme: glomeruli_segmentation_amd/outlines.py.
 *
 * The plan is host-only: the bytes of workspace the entry needs.  It refuses what the entry refuses about sizes: non-positive
 * height / width, edges_cap < 0 or > 2^31 - 1, a NULL workspace_bytes (GS_ERR_INVALID); height * width > 2^31 - 1
 * (GS_ERR_UNSUPPORTED).  The figure never shrinks with height * width nor with edges_cap. */
gs_status gs_outlines_plan(int height, int width, long long edges_cap, size_t *workspace_bytes);
/* Stream-ordered, no host wait, no allocation, capturable.  All pointers device.
 *   labels        int32 [height,width], contiguous, 4-byte aligned; connectivity 4 or 8
 *   workspace     at least the plan's bytes for this edges_cap, 16-byte aligned; its contents on entry do not matter
 *   loop_label, loop_first, loop_edges   int32 [edges_cap / 4] (a loop has at least 4 edges); loop_area2 int64 [edges_cap / 4]
 *   loop_offsets  int32 [edges_cap / 4 + 1];  points int32 [edges_cap,2] (a corner is the end of an edge)
 *   counts        int64 [3]: edges_needed, n_loops, n_points
 * counts, loop_offsets[0 .. n_loops], the first n_loops rows of the loop arrays and the first n_points of points are written on
 * every call.  If edges_needed > edges_cap, counts becomes (edges_needed, -1, -1), nothing else is promised and the status is
 * GS_OK: the caller retries with a larger cap, the pattern of `cap` in the labelling entry.  With no edges counts is (0, 0, 0)
 * and loop_offsets[0] = 0.  With edges_cap < 4 the loop arrays, with edges_cap == 0 points may be NULL.
 * GS_ERR_INVALID before any device work: what the plan refuses (the number of pixels: GS_ERR_UNSUPPORTED as there), a negative n,
 * a connectivity other than 4 and 8, a NULL or misaligned required pointer, a workspace smaller than the plan. */
gs_status gs_instance_outlines(const int32_t *labels, int n, int height, int width, int connectivity, void *workspace,
                               size_t workspace_bytes, long long edges_cap, int32_t *loop_label, int32_t *loop_first,
                               int32_t *loop_edges, long long *loop_area2, int32_t *loop_offsets, int32_t *points,
                               long long *counts, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOMSEG_OUTLINES_ABI_H */
