/*
 * hulls_abi.h -- the C declarations of the per-glomerulus convex-hull entries of libglomseg.so (csrc/hulls.hip), in the style of
 * csrc/outlines_abi.h.
 */
#ifndef GLOMSEG_HULLS_ABI_H
#define GLOMSEG_HULLS_ABI_H

#include "../../include/glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-glomerulus convex hulls on the device: for every instance of a label map (int32 [height,width], as gs_slide_instances of
 * glomseg_instances.h writes it) the ring of its hull's vertices and six integers -- the vertex count, twice the hull's area, the
 * largest squared distance of two vertices and the narrowest caliper.  Everything is integer and exact, and every output byte is
 * a pure function of the inputs.  The ABI number stays 10: no signature changes, and a caller finds out whether a library has
 * these two entries by looking the symbols up.  They are exported by libglomseg.so and declared here, beside their sources, not
 * under include/: the entry set of every public header there is fixed.  glomeruli_segmentation_amd/hulls.py binds them
 * (HULL_ENTRIES).
 *   lattice     that of gs_instance_outlines (outlines_abi.h): point (x, y) is the top-left corner of pixel (x, y), 0 <= x <= width,
 *               0 <= y <= height; x to the right, y down.
 *   instances   a label below 1 or above n is background: such a pixel belongs to no instance and is never indexed through.
 *   boxes       int32 [n,4] (xmin, ymin, xmax, ymax), half-open, caller-supplied, any content.  A box is valid when it is not
 *               empty and lies within the map.
 *   hull        of instance i: the convex hull of the closed unit squares of its pixels inside its box -- gs_instance_morphometry's
 *               rule for feret2: a pixel of i outside the box is left out.  Equivalently the hull of those pixels' corner points,
 *               so twice the hull's area is at least twice the pixels and a rectangle has solidity 1.  feret2 is measured between
 *               pixel centres and stays as it is.  skimage.measure.regionprops differs: for its convex_area it rasterises a hull
 *               back to pixels and counts those, a whole number of pixels; this figure is the polygon's exact area.
 *   lines       lattice line Y, ymin <= Y <= ymax.  L(Y) is the smallest xmin over the non-empty rows Y - 1 and Y of the
 *               instance in its box, R(Y) the largest xmax + 1 over the same rows.  A line with no non-empty adjacent row does
 *               not exist: it has no points.
 *   vertices    exactly the points (L(Y), Y) that are strict vertices of the convex minorant of L over the lines that exist, and
 *               the points (R(Y), Y) that are strict vertices of the concave majorant of R.  Line i is a left vertex iff
 *                 max over j < i of (L_i - L_j) / (i - j)  <  min over k > i of (L_k - L_i) / (k - i),
 *               fractions compared by cross-multiplication in int64; a side without lines counts as satisfied, so the first and
 *               the last existing line are vertices of both chains.  The right chain is the same rule applied to -R.  Collinear
 *               points are dropped: the vertex set is minimal and unique, and an instance with a pixel has at least 4 vertices.
 *   ring        starts at (L(Ymin), Ymin), Ymin the first existing line, and runs clockwise on screen, as an outer loop of
 *               gs_instance_outlines (positive loop_area2): the right-chain vertices in increasing Y, then the left-chain
 *               vertices in decreasing Y, without the start.  hull_offsets[i - 1] .. hull_offsets[i] indexes points, int32
 *               [points_needed,2] holding (x, y).
 *   stats       int64 [n,6], row i - 1:
 *                 0  k, the number of vertices
 *                 1  twice the hull's area: the sum over the ring's edges of sx * ey - ex * sy, as loop_area2
 *                 2  the largest squared distance between two vertices (up to 2 * 32768^2, hence int64)
 *                 3  w of the narrowest edge      4  len2 of the narrowest edge      5  its ring index e
 *               For edge e from vertex a = e to vertex b = (e + 1) % k, w is the largest |(b - a) x (v - a)| over the ring's
 *               vertices v and len2 = |b - a|^2: the caliper width across edge e is w / sqrt(len2).  Columns 3..5 are those of the
 *               edge with the smallest w^2 / len2, compared exactly in 128 bits (the products reach 2^93); among equal ratios
 *               the lowest e.
 *               An invalid box gives a row of -1 and an empty ring; a valid box without a pixel of i a row of 0 and an empty ring.
 *   counts      int64 [2]: rows_needed, the sum of the valid boxes' heights, and points_needed, the vertices of all rings.  Where
 *               rows_needed exceeds rows_cap the rings cannot be formed, and points_needed is the bound that always suffices:
 *               2 * (rows_needed + the number of valid boxes), two vertices for every lattice line.
 * Kernels and their safety rules: csrc/hulls.hip.  Measures, polygons and the command line: glomeruli_segmentation_amd/hulls.py.
 *
 * The plan is host-only: the bytes of workspace the entry needs, a function of rows_cap alone.  It refuses what the entry refuses
 * about sizes: non-positive height / width, a negative rows_cap, a NULL workspace_bytes (GS_ERR_INVALID); a side above 32768 or
 * more than 2^31 - 1 pixels (GS_ERR_UNSUPPORTED).  The figure never shrinks with rows_cap. */
gs_status gs_hulls_plan(int height, int width, long long rows_cap, size_t *workspace_bytes);
/* Stream-ordered, no host wait, no allocation, capturable; reads no device value on the host.  All pointers device.
 *   labels        int32 [height,width], contiguous, 4-byte aligned
 *   boxes         int32 [n,4], 4-byte aligned
 *   workspace     at least the plan's bytes for this rows_cap, 8-byte aligned; its contents on entry do not matter
 *   hull_offsets  int32 [n + 1];  points int32 [points_cap,2];  stats int64 [n,6];  counts int64 [2]
 * counts, hull_offsets, stats and the first points_needed rows of points are written on every call.  If rows_needed > rows_cap or
 * points_needed > points_cap, every stats row is -1, every offset is 0, counts tells both figures and the status is GS_OK: the
 * caller retries with larger caps, the pattern of `cap` in the labelling entry.  With n == 0 only counts = (0, 0) and
 * hull_offsets[0] = 0 are written, and boxes, points and stats may be NULL; with points_cap == 0 points may be NULL.
 * GS_ERR_INVALID before any device work: what the plan refuses (sizes: GS_ERR_UNSUPPORTED as there), a negative n, a points_cap
 * outside 0..2^31 - 1, a NULL or misaligned required pointer, a workspace smaller than the plan. */
gs_status gs_instance_hulls(const int32_t *labels, const int32_t *boxes, int n, int height, int width, void *workspace,
                            size_t workspace_bytes, long long rows_cap, int32_t *hull_offsets, int32_t *points, long long points_cap,
                            long long *stats, long long *counts, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOMSEG_HULLS_ABI_H */
