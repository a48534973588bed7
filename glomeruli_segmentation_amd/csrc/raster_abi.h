/*
 * raster_abi.h -- the C declarations of the polygon rasteriser entries of libglomseg.so (csrc/raster.hip), in the style of
 * csrc/outlines_abi.h.
 */
#ifndef GLOMSEG_RASTER_ABI_H
#define GLOMSEG_RASTER_ABI_H

#include "../../include/glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Polygons back to a map on the device: the inverse of gs_instance_outlines (outlines_abi.h).  gs_polygon_raster paints features
 * into an int32 owner map [height,width] by the even-odd rule at pixel centres.  Everything is integer and exact.  The ABI number
 * stays 10: no signature changes, and a caller finds out whether a library has these two entries by looking the symbols up.
 * The two entries are exported by libglomseg.so and declared here, beside their sources, not under include/: the entry set of
 * every public header there is fixed.  glomeruli_segmentation_amd/rasterize.py binds them (RASTER_ENTRIES).
 *   features     a feature is a set of rings, a ring a closed list of vertices (the first is not repeated at the end).  Ring r
 *                holds points[ring_offsets[r] .. ring_offsets[r+1]) and belongs to feature ring_feature[r]; the rings of a
 *                feature need not be adjacent.  A ring whose ring_feature is outside [0, n_features) is ignored.
 *   coordinates  int32 fixed point with frac_bits fractional bits, 0..8; S = 1 << frac_bits.  Vertex (qx, qy) is the lattice
 *                point (qx / S, qy / S) of the outlines' lattice: point (x, y) is the top-left corner of pixel (x, y).  A
 *                coordinate outside [-2^28, 2^28] is taken as the nearer bound: this clamp on load is part of the definition
 *                and keeps all arithmetic inside int64.  In units of 1/(2S) pixel a vertex is (X, Y) = (2qx, 2qy) and the
 *                centre of pixel (x, y) is ((2x+1)S, (2y+1)S).
 *   crossings    edge k of a ring runs from vertex k to the next, the last to the first; orient it so that Y0 < Y1 (an edge with
 *                Y0 == Y1 has none).  It crosses row j when Y0 <= (2j+1)S < Y1 -- half-open, a scanline through a vertex counts
 *                once -- and 0 <= j < height.  There, with den = Y1 - Y0 and num = X0 * den + ((2j+1)S - Y0) * (X1 - X0), the
 *                crossing toggles column t = clamp(ceil((num - S * den) / (2S * den)), 0, width): the first pixel whose centre
 *                is at or right of the crossing.
 *   inside       pixel (x, j) is inside feature f when the number of crossings of f's edges at row j with t <= x is odd:
 *                even-odd, so holes, self-intersections and rings of either orientation follow.  A centre exactly on an edge
 *                belongs to the feature whose left boundary the edge is: two features that share an edge split the pixels
 *                exactly.  Rings of 0, 1 or 2 vertices and repeated vertices contribute nothing, by the same arithmetic.
 *   owner        owner[p] = 1 + the largest feature index whose inside contains p, or 0: later features win.
 *   class_map    optional, uint8: feature_class[owner - 1], or 0.
 *   words        the bit scratch of a feature covers its box: with col(X) = clamp(ceil((X - S) / (2S)), 0, width) and
 *                row(Y) = clamp(ceil((Y - S) / (2S)), 0, height) taken over every vertex of its rings, rows row_min .. row_max - 1
 *                and columns col_min .. col_max (every t of the feature lies there), a row in 32-bit words:
 *                (row_max - row_min) * ceil((col_max - col_min + 1) / 32) words, none for a feature without vertices.
 *                words_needed is the sum over the features.
 * Kernels and their safety rules: csrc/raster.hip.  GeoJSON, labelme and the command line: glomeruli_segmentation_amd/rasterize.py.
 *
 * The plan is host-only: the bytes of workspace the entry needs.  It refuses what the entry refuses about sizes: non-positive
 * height / width, a negative n_points, n_rings, n_features or words_cap or one above 2^31 - 1, a NULL workspace_bytes
 * (GS_ERR_INVALID); height * width > 2^31 - 1 (GS_ERR_UNSUPPORTED).  The figure never shrinks with any argument. */
gs_status gs_polygon_raster_plan(int height, int width, long long n_points, long long n_rings, long long n_features,
                                 long long words_cap, size_t *workspace_bytes);
/* Stream-ordered, no host wait, no allocation, capturable; reads no device value on the host.  All pointers device.
 *   points         int32 [n_points,2] holding (qx, qy); ring_offsets int32 [n_rings + 1], non-decreasing from 0 to n_points;
 *                  ring_feature int32 [n_rings].  4-byte aligned; each may be NULL exactly where its count is 0 (ring_offsets
 *                  where n_rings is 0).  For ring_offsets that break the rule the output is unspecified, and nothing outside the
 *                  arrays given is touched.
 *   feature_class  uint8 [n_features] or NULL; class_map uint8 [height,width] or NULL, and NULL where feature_class is
 *   workspace      at least the plan's bytes for these sizes, 16-byte aligned; its contents on entry do not matter
 *   owner          int32 [height,width], written in full on every call
 *   counts         int64 [2]: words_needed, crossings (the toggles applied)
 * If words_needed > words_cap, counts becomes (words_needed, -1), nothing else is promised and the status is GS_OK: the caller
 * retries with a larger cap, the pattern of edges_cap in the outline entry.  With no feature, or none that covers a pixel,
 * owner is all zero.
 * GS_ERR_INVALID before any device work: what the plan refuses (the number of pixels: GS_ERR_UNSUPPORTED as there), frac_bits
 * outside 0..8, a NULL or misaligned required pointer, class_map without feature_class, a workspace smaller than the plan. */
gs_status gs_polygon_raster(const int32_t *points, long long n_points, const int32_t *ring_offsets, const int32_t *ring_feature,
                            long long n_rings, const uint8_t *feature_class, long long n_features, int frac_bits, int height,
                            int width, void *workspace, size_t workspace_bytes, long long words_cap, int32_t *owner,
                            uint8_t *class_map, long long *counts, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOMSEG_RASTER_ABI_H */
