/*
 * glomseg_plan.h -- the yes/no decisions of the ESPNet forward plan (an addition to glomseg.h; the ABI number stays 9: no
 * signature of glomseg.h changes, and a caller finds out whether a library has this entry by looking the symbol up).
 *
 * gs_espnet_plan_forward (glomseg.h) reports one kernel form per launch class.  The planner (csrc/forward_plan.h) also makes
 * decisions that are no form of a launch class; this entry reports them for the same arguments, plus whether the handle is an
 * ESPNet-C one (encoder_only, as in gs_espnet_create), which the forms do not depend on.
 */
#ifndef GLOMSEG_PLAN_H
#define GLOMSEG_PLAN_H

#include "glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* output1_0 is stored raw and b2 is applied by its consumers on load (every model with p > 0) */
#define GS_PLAN_LAZY_B2 1
/* the level-3 stride-2 reduce also computes level3_C (the decoder's 1x1 over output1_cat) and dec2 reads those class planes
 * instead of the 131 of output1_cat; the stage "level3_C" of gs_espnet_read_stage exists exactly then */
#define GS_PLAN_L3C_IN_REDUCE 2

/* Host-only, no handle and no device.  *flags = the GS_PLAN_* bits of the plan of a forward of n tiles of height x width for
 * ESPNet(classes, p, q) (encoder_only != 0: ESPNet-C) on a device with num_cus compute units.  Refuses what
 * gs_espnet_plan_forward refuses. */
gs_status gs_espnet_plan_flags(int n, int height, int width, int p, int q, int classes, int encoder_only, int num_cus, int *flags);

#ifdef __cplusplus
}
#endif

#endif
