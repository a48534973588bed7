/*
 * glomseg_scoring.h -- scoring of labelled crops in the batched crop pass of libglomseg.so (an addition to glomseg.h; the ABI
 * number stays 8: no signature of glomseg.h changes, and a caller finds out whether a library has these two entries by
 * looking the symbols up).
 *
 * With --label_data_dir the reference's loop body (module/espnet/test/VisualizeResults_iou.py:191-222) resizes every crop's
 * label image to the network size (cv2.resize INTER_NEAREST, :195), adds the confusion matrix of that label and
 * img_out.max(1)[1] to its iouEval (:201-203, module/common/IOUEval.py:19-21), takes np.unique of the resized label (:196) and
 * blends the palette-coloured label over the crop (:218-222).  Here that is one descriptor-table kernel per batch behind the
 * forward (crops_score_kernel, csrc/crops.hip) and a second launch of the overlay kernel; nothing is resized in memory.
 */
#ifndef GLOMSEG_SCORING_H
#define GLOMSEG_SCORING_H

#include "glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device-resident stage, stream-ordered; it needs no handle.  Behind gs_espnet_segment_crops on the same stream it scores that
 * call's net_masks.  For every network pixel (oy, ox) of crop i:
 *     g = label_i[min(floor(oy * h_i / net_h), h_i - 1)][min(floor(ox * w_i / net_w), w_i - 1)]     (OpenCV's double arithmetic)
 *     p = net_masks[i][oy][ox]
 *     bit g of seen[i] is set (all 256 byte values);  conf[i][g][p] += 1 when g < classes (rows = ground truth)
 *   net_masks      device uint8 [n,net_h,net_w], 4-byte aligned; a byte >= classes (no forward writes one) is not counted
 *   packed_labels  device: crop i's label, uint8 [descs[i].h, descs[i].w], at descs[i].out_off (the layout of packed_out)
 *   descs          HOST memory, n <= GS_MAX_CROPS_PER_CALL (they travel as kernel arguments); in_off, x1, y1 are not read
 *   conf           device uint64 [n,classes,classes]; seen device uint64 [n,4] (a 256-bit set: bit v of word v / 64) or NULL.
 * Both are WRITTEN (zeroed on the stream first), not accumulated into.  2 <= classes <= GS_MAX_CLASSES, net_h and net_w positive
 * multiples of 8; anything else, a NULL mask / label / conf pointer included, is GS_ERR_INVALID before any device work. */
gs_status gs_espnet_score_crops(const uint8_t *net_masks, const uint8_t *packed_labels, const gs_crop_desc *descs, int n, int net_h,
                                int net_w, int classes, unsigned long long *conf, unsigned long long *seen, void *hip_stream);

/* What gs_espnet_segment_crops_host_scored adds to gs_espnet_segment_crops_host. */
typedef struct gs_crop_scoring {
    const uint8_t *const *labels;   /* labels[i]: host uint8 [heights[i], widths[i]], uploaded with the batch's crops */
    unsigned long long *conf;       /* host uint64 [n_crops, classes, classes] of the models' class count; comes back with the counts */
    unsigned long long *seen;       /* host uint64 [n_crops, 4] or NULL */
    uint8_t *const *gt_overlay_bgr; /* or NULL.  gt_overlay_bgr[i]: host uint8 [heights[i], widths[i], 3]: the label coloured with the
                                     * palette and blended over the crop with the weights of the call's `overlay` argument
                                     * (GS_ERR_INVALID without one), by a second launch of the overlay kernel over the packed labels */
    int32_t gt_clamp;               /* a label value beyond the palette: 0 = black (as in `overlay`), non-zero = the palette's last
                                     * row (np.minimum(label, n_colours - 1), what the segment command has always written) */
} gs_crop_scoring;

/* gs_espnet_segment_crops_host with a scoring block (NULL: exactly that entry, which is this one called with NULL).  The
 * network-resolution masks are scored on the device where the forward leaves them; net_masks is downloaded only when the caller
 * asks for it.  One model, ensembles of either kind and ESPNet-C handles alike.  A NULL labels / labels[i] / conf pointer is
 * GS_ERR_INVALID before any device work. */
gs_status gs_espnet_segment_crops_host_scored(gs_espnet *const *models, int n_models, const uint8_t *const *crops, const int *heights,
                                              const int *widths, int n_crops, const float *means, const float *stds, int net_h,
                                              int net_w, int batch, uint8_t *const *masks, uint8_t *net_masks,
                                              unsigned long long *hist, const gs_paste_target *paste, const int *x1, const int *y1,
                                              const gs_crop_overlay *overlay /* or NULL */, const gs_crop_scoring *scoring /* or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GLOMSEG_SCORING_H */
