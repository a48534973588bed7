/*
 * glomseg_detector_steps.h -- the detector's kernels one step at a time, FOR TESTS (an addition to glomseg.h; the ABI number
 * stays: no signature changes, and a caller finds out whether a library has the entries by looking the symbols up).
 *
 * gs_detector_forward (glomseg.h) runs its glue kernels and its packed-weight convolutions only on what the previous stage
 * produced.  The entries below run ONE of them on device buffers the caller supplies, through the same host launchers the
 * forward calls (csrc/detector.hip: launch_det_*, the per-layer convolution), so that a test can choose the inputs: negative
 * maps under the max-pool, saturated logits, NaN deltas, sizes that are no multiple of anything.  Nothing in the product calls
 * them.  Every entry checks pointers and sizes on the host and returns GS_ERR_INVALID with a message (gs_last_error) instead
 * of launching; what a step reads THROUGH an index list (sel, keep, box_image) is the caller's to keep in range, as noted.
 */
#ifndef GLOMSEG_DETECTOR_STEPS_H
#define GLOMSEG_DETECTOR_STEPS_H

#include "glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only.  TensorFlow's [kh,kw,cin,cout] weights -> the [kh*kw*cin / 4][cout][4] layout the tiled and wide convolution
 * kernels read with one 16-byte load per lane (what gs_detector_create does to every layer).  cin % 8 != 0 is refused with the
 * packed kernels' GS_ERR_UNSUPPORTED.  `packed` holds kh*kw*cin*cout floats and must not overlap `weight`. */
gs_status gs_conv2d_nhwc_pack4(const float *weight, int kh, int kw, int cin, int cout, float *packed);

/* gs_conv2d_nhwc with `packed_weight` already in gs_conv2d_nhwc_pack4's layout (device memory): the <true> instances of the
 * tiled / wide kernels, chosen by gs_conv2d_nhwc_form(..., packed = 1), whose refusals it shares. */
gs_status gs_conv2d_nhwc_packed(const float *in, int n, int h, int w, int cin, const float *packed_weight, int kh, int kw, int cout,
                                const float *bias_or_null, int stride, int pad, int relu, float *out, void *hip_stream);

/* The arguments of one step: device pointers and sizes, each step reading the fields its row below names (the rest are
 * ignored).  Floats unless noted; A = 12 anchors per cell, P = gs_detector_num_proposals().
 *
 *   step               in[0]                 in[1]                in[2]              sizes                     out[0]                    out[1]          out[2]
 *   "preprocess"       u8 [n,h,w,3]                                                  n h w                     [n,ceil(h/2),ceil(w/2),16]
 *   "maxpool"          [n,h,w,c]                                                     n h w c k stride pad      [n,ho,wo,c]     (c % 4 == 0, pad < k; ho = (h + 2 pad - k) / stride + 1)
 *   "conv"             [n,h,w,cin]                                                   n h w layer               [n,ho,wo,cout]  (row `layer` of gs_detector_layer_info with the HANDLE's packed
 *                                                                                                                               weights and bias, planned as the forward plans the layer)
 *   "objectness"       rpn [n,h,w,6A]                                                n h w                     [n,h,w,A]
 *   "rpn_decode"       rpn [n,h,w,6A]        sel int [n,count]                       n h w count win_h win_w   [n,count,4]     (sel: anchor index in [0, h*w*A), or negative = none)
 *   "gather_proposals" boxes [n,count,4]     keep int [n,P]                          n count win_h win_w       prop [n,P,4]              norm [n,P,4]    image int [n,P]
 *                                                                                                                              (keep: position in [0, count), or negative = padding)
 *   "crop_pool"        feat [n,h,w,c]        boxes [count,4]      image int [count]  n h w c count crop        [count,crop/2,crop/2,c]   (c % 4 == 0, crop even; any image index)
 *   "avgpool"          [n,h,w,c]                                                     n h w c                   [n,c]           (mean over the h*w positions)
 *   "head_decode"      head [count,6]        prop [count,4]       keep int [count]   count win_h win_w         score [count]             boxes [count,4]
 */
typedef struct gs_detector_step_args {
    const void *in[3];
    void *out[3];
    int64_t n;            /* images (or rows) */
    int32_t h, w, c;      /* the input map */
    int32_t k, stride, pad;
    int32_t layer;
    int32_t count;        /* entries per image, boxes, or proposals in all: see the table */
    int32_t crop;
    float win_h, win_w;   /* the window in pixels (box decode, clip and normalisation) */
} gs_detector_step_args;

/* Name of step i in the table's order, NULL past the last: what gs_detector_step accepts. */
const char *gs_detector_step_name(int i);

/* Runs step `step` on stream `hip_stream` (asynchronous, like the forward).  `handle` is needed by "conv" only and may be NULL
 * for the others.  An unknown name, a missing pointer or a size the kernel cannot take: GS_ERR_INVALID, nothing launched; a
 * "conv" shape the packed kernels refuse: their GS_ERR_UNSUPPORTED. */
gs_status gs_detector_step(gs_detector *handle, const char *step, const gs_detector_step_args *args, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif
