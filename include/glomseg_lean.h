/*
 * glomseg_lean.h -- the one decision of the ESPNet forward plan that depends on the REQUEST and not only on the model and the
 * shape (an addition to glomseg.h and glomseg_plan.h; the ABI number stays: no signature changes, and a caller finds out
 * whether a library has the entry by looking the symbol up).
 *
 * A forward is "lean" when it is asked for no logits and the plan computes both decoder projections as side sums of their
 * producers (GS_PLAN_L3C_IN_REDUCE and GS_PLAN_CLS_IN_L3 of glomseg_plan.h: a full five-class network with q >= 1).  Nothing of
 * such a forward reads the last level-3 block's map, so that launch does not store it.  What gs_espnet_read_stage serves after
 * which kind of request is listed at its declaration in glomseg.h.
 */
#ifndef GLOMSEG_LEAN_H
#define GLOMSEG_LEAN_H

#include "glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only, no handle and no device.  *lean = 1 if a forward of n tiles of height x width for ESPNet(classes, p, q)
 * (encoder_only != 0: ESPNet-C) on a device with num_cus compute units is lean when it is asked for logits (want_logits != 0) or
 * not (0), else 0.  An ESPNet-C handle, a class count other than five, q = 0 and every request with logits are never lean.
 * Refuses what gs_espnet_plan_forward refuses. */
gs_status gs_espnet_plan_lean(int n, int height, int width, int p, int q, int classes, int encoder_only, int num_cus, int want_logits,
                              int *lean);

#ifdef __cplusplus
}
#endif

#endif
