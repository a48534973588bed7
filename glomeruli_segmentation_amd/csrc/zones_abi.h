/*
 * zones_abi.h -- the C declarations of the influence-zone and neighbour-gap entries of libglomseg.so (csrc/zones.hip), in the style
 * of csrc/raster_abi.h.
 */
#ifndef GLOMSEG_ZONES_ABI_H
#define GLOMSEG_ZONES_ABI_H

#include "../../include/glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Where a glomerulus lies among the others: for every pixel of a slide map the nearest instance (gs_instance_zones) and for every
 * boundary pixel of an instance the nearest pixel of any OTHER instance (gs_foreign_dist).  Everything is integer and exact, and
 * every output byte is a pure function of the inputs.  The ABI number stays 10: no signature changes, and a caller finds out
 * whether a library has these four entries by looking the symbols up.  They are exported by libglomseg.so and declared here,
 * beside their sources, not under include/: the entry set of every public header there is fixed.
 * glomeruli_segmentation_amd/zones.py binds them (ZONE_ENTRIES).
 *   labels       int32 [height,width] as gs_slide_instances writes it.  A value in 1..n is an instance; anything else is background
 *                and is never used as an index.  The outside of the map holds nothing: it is neither an instance nor a site.
 *   pixels       pixel (x, y) is the point (x, y), pos = y * width + x, and |p - q|^2 the squared Euclidean distance of two.
 *   sizes        a side above 32768 or more than 2^31 - 1 pixels: GS_ERR_UNSUPPORTED.  max_d2 outside 0..2^30: GS_ERR_INVALID.
 *   zone         S = the instance pixels.  For every pixel p the lexicographic minimum of (|p - q|^2, labels[q]) over q in S with
 *                |p - q|^2 <= max_d2: zone[p] is that label and zone_d2[p] that distance; (0, -1) where there is no such q.  A
 *                pixel of instance a gets (a, 0).  An exact tie between two instances goes to the lower id.  zone is
 *                skimage.segmentation.expand_labels with that tie rule, and the exact disc dilation of the map by sqrt(max_d2).
 *   boundary     a pixel whose label is in 1..n and one of whose 4-neighbours carries another value or lies outside the map
 *                (gs_instance_boundary_dist's test).
 *   near         for a boundary pixel p of instance a the lexicographic minimum of (|p - q|^2, labels[q]) over pixels q of
 *                instances b != a with |p - q|^2 <= max_d2: near_d2[p] is that distance and near_id[p] that label; (-1, 0) where
 *                there is none, and at every pixel that is no boundary pixel.
 * Kernels and their safety rules: csrc/zones.hip.  Territories, neighbour tables and the command line:
 * glomeruli_segmentation_amd/zones.py.
 *
 * The plans are host-only: the bytes of workspace the entry of the same name needs.  Each refuses what its entry refuses about
 * sizes: non-positive height / width, a NULL workspace_bytes (GS_ERR_INVALID); a side above 32768 or height * width > 2^31 - 1
 * (GS_ERR_UNSUPPORTED).  The figure never shrinks when an argument grows. */
gs_status gs_instance_zones_plan(int height, int width, size_t *workspace_bytes);
gs_status gs_foreign_dist_plan(int height, int width, size_t *workspace_bytes);

/* Both entries: stream-ordered, no host wait, no allocation, capturable; they read no device value on the host.  All pointers
 * device.
 *   labels       int32 [height,width], contiguous, 4-byte aligned; n >= 0, and with n == 0 every pixel is background
 *   workspace    at least the plan's bytes, 8-byte aligned; its contents on entry do not matter
 *   zone, zone_d2 / near_d2, near_id   int32 [height,width], 4-byte aligned, written in full on every call
 * GS_ERR_INVALID before any device work: what the plan refuses (sizes: GS_ERR_UNSUPPORTED as there), a negative n, max_d2 outside
 * 0..2^30, a NULL or misaligned pointer, a workspace smaller than the plan. */
gs_status gs_instance_zones(const int32_t *labels, int n, int height, int width, int max_d2, void *workspace, size_t workspace_bytes,
                            int32_t *zone, int32_t *zone_d2, void *hip_stream);
gs_status gs_foreign_dist(const int32_t *labels, int n, int height, int width, int max_d2, void *workspace, size_t workspace_bytes,
                          int32_t *near_d2, int32_t *near_id, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOMSEG_ZONES_ABI_H */
