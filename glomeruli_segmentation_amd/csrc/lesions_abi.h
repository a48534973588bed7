/*
 * lesions_abi.h -- the C declarations of the per-glomerulus lesion entries of libglomseg.so (csrc/lesions.hip), in the style of
 * csrc/zones_abi.h.
 */
#ifndef GLOMSEG_LESIONS_ABI_H
#define GLOMSEG_LESIONS_ABI_H

#include "../../include/glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which classes line which part of a glomerulus' outline: for every boundary pixel of an instance the classes found within reach
 * inside that instance (gs_rim_classes), and for every loop of gs_instance_outlines (csrc/outlines_abi.h) and every bit of such a
 * map how many of the loop's unit edges are covered, in how many arcs, the longest how long (gs_loop_arcs).  Everything is integer
 * and exact, and every output byte is a pure function of the inputs.  The ABI number stays 10: no signature changes, and a caller
 * finds out whether a library has these three entries by looking the symbols up.  They are exported by libglomseg.so and declared
 * here, beside their sources, not under include/: the entry set of every public header there is fixed.
 * glomeruli_segmentation_amd/lesions.py binds them (LESION_ENTRIES).
 *   labels       int32 [height,width] as gs_slide_instances writes it.  A value in 1..n is an instance; anything else is background
 *                and is never used as an index.
 *   pixels       pixel (x, y) is the point (x, y), pos = y * width + x, and |p - q|^2 the squared Euclidean distance of two.
 *   sizes        a side above 32768 or more than 2^31 - 1 pixels: GS_ERR_UNSUPPORTED.
 *   boundary     a pixel whose label is in 1..n and one of whose 4-neighbours carries another value or lies outside the map
 *                (gs_instance_boundary_dist's test).
 *   near_classes for a boundary pixel p of instance i the bitwise OR of 1 << class_map[q] over the pixels q with labels[q] == i,
 *                |p - q|^2 <= max_d2 and class_map[q] < classes.  p is its own q: with max_d2 == 0 this is the class of p itself.  A
 *                pixel of another instance or of the background contributes nothing, however near it is; a class value >= classes
 *                contributes no bit.  0 at every pixel that is no boundary pixel.
 * Stream-ordered, no host wait, no allocation, no workspace, capturable; reads no device value on the host.  All pointers device.
 *   labels       int32 [height,width], contiguous, 4-byte aligned; n >= 0, and with n == 0 near_classes is all 0
 *   class_map    uint8 [height,width], contiguous
 *   near_classes int32 [height,width], 4-byte aligned, written in full on every call
 * GS_ERR_INVALID before any device work: non-positive height / width, classes outside 2..20, max_d2 outside 0..1024 (a radius of 32
 * map pixels), a negative n, a NULL or misaligned pointer.  Sizes: GS_ERR_UNSUPPORTED as above. */
gs_status gs_rim_classes(const int32_t *labels, const uint8_t *class_map, int n, int classes, int height, int width, int max_d2,
                         int32_t *near_classes, void *hip_stream);

/* The loops are those gs_instance_outlines wrote for the label map that `mask` belongs to; n_loops, n_points and edges are its
 * counts (counts[1], counts[2], counts[0]).
 *   unit edges   the corners of loop l are points[loop_offsets[l] .. loop_offsets[l+1]), m of them.  Segment k runs from corner k
 *                to corner (k + 1) % m and is axis-parallel; the segments in order of k, each split into unit edges in its direction,
 *                are the loop's loop_edges[l] edges in walking order.  The first corner is the end of the key edge's straight run, so
 *                the sequence is a rotation of the walk from the key edge; nothing below depends on the rotation.
 *   pixel        of a unit edge with start vertex (X, Y): heading east (X, Y), its top side; south (X - 1, Y), its right side;
 *                west (X - 1, Y - 1), its bottom side; north (X, Y - 1), its left side.  It lies in the map, belongs to the loop's
 *                instance and is a boundary pixel.
 *   covered      edge t of loop l is covered by bit b when bit b of mask[pixel(t)] is set.
 *   arcs         int32 [n_loops,bits,3], for every loop l and every b < bits: covered, the number of covered edges; n_arcs, the
 *                number of maximal runs of covered edges on the cycle (a run that passes the end of the sequence and continues at
 *                its start is one run), 1 when all are covered and 0 when none is; longest, the length of the longest such run,
 *                loop_edges[l] when all are covered and 0 when none is.
 * Kernels and their safety rules (what happens for loop arrays of any other contents): csrc/lesions.hip.  The lesion table and the
 * command line: glomeruli_segmentation_amd/lesions.py.
 *
 * The plan is host-only: the bytes of workspace gs_loop_arcs needs.  GS_ERR_INVALID: bits outside 1..31, a negative count,
 * edges > 2^31 - 1, n_points > edges, 4 * n_loops > edges, a NULL workspace_bytes.  The figure never shrinks when an argument
 * grows. */
gs_status gs_loop_arcs_plan(long long edges, long long n_points, long long n_loops, int bits, size_t *workspace_bytes);
/* Stream-ordered, no host wait, no allocation, capturable; reads no device value on the host.  All pointers device.
 *   mask         int32 [height,width], contiguous, 4-byte aligned (gs_rim_classes' near_classes, or any other map of bit words)
 *   loop_edges   int32 [n_loops]; loop_offsets int32 [n_loops + 1]; points int32 [n_points,2]: gs_instance_outlines' outputs
 *   workspace    at least the plan's bytes, 8-byte aligned; its contents on entry do not matter
 *   arcs         int32 [n_loops,bits,3], 4-byte aligned, written in full on every call
 * With n_loops == 0 nothing is written and the status is GS_OK.  GS_ERR_INVALID before any device work: what the plan refuses,
 * non-positive height / width (sizes: GS_ERR_UNSUPPORTED as above), a NULL or misaligned pointer, a workspace smaller than the
 * plan. */
gs_status gs_loop_arcs(const int32_t *mask, int height, int width, int bits, const int32_t *loop_edges, const int32_t *loop_offsets,
                       const int32_t *points, long long n_loops, long long n_points, long long edges, void *workspace,
                       size_t workspace_bytes, int32_t *arcs, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOMSEG_LESIONS_ABI_H */
