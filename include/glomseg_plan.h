/*
 * glomseg_plan.h -- the yes/no decisions of the ESPNet forward plan, and a handle's set-up without a device (an addition to
 * glomseg.h; the ABI number stays 9: no signature of glomseg.h changes, and a caller finds out whether a library has an entry
 * by looking the symbol up).
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
/* the encoder classifier behind b3 is summed in the epilogues of the level-3 down-sampler and of the last level-3 ESP block,
 * and a small kernel adds their partial planes where dec1_kernel would re-read both 128-channel maps: the full five-class
 * networks with q >= 1 (no ESPNet-C handle, no other class count).  (An enumerator, not a macro: tests/test_l3c_side_sums.py
 * holds the list of GS_PLAN_* macros to the two above.) */
enum { GS_PLAN_CLS_IN_L3 = 4 };

/* Host-only, no handle and no device.  *flags = the GS_PLAN_* bits of the plan of a forward of n tiles of height x width for
 * ESPNet(classes, p, q) (encoder_only != 0: ESPNet-C) on a device with num_cus compute units.  Refuses what
 * gs_espnet_plan_forward refuses. */
gs_status gs_espnet_plan_flags(int n, int height, int width, int p, int q, int classes, int encoder_only, int num_cus, int *flags);

/* ---- handle set-up without a handle: what gs_espnet_create packs and what gs_espnet_reserve allocates.  Host-only, no device. */

/* a named piece of the packed weight blob: `floats` floats from float `offset` on (a multiple of 4) */
typedef struct gs_weight_piece {
    char name[32];
    long long offset, floats;
} gs_weight_piece;

/* The device weight blob of a handle (csrc/espnet_weights.h), exactly what gs_espnet_create uploads for the same first seven
 * arguments, and the same refusals: classes outside 2..20 is GS_ERR_UNSUPPORTED, a missing or mis-shaped tensor GS_ERR_INVALID
 * with its name in gs_last_error.  *n_floats = its size; `out` (room for `cap` floats) may be NULL to ask for the size alone.
 * `pieces` (room for `piece_cap`; may be NULL) receives every piece of the blob in order -- "w1", "bn1", "b1", "b2", per block
 * "l2_0.c1" / "l2_0.br", "l2.<i>.c1", "l3_0.c1", "l3.<i>.br", ..., "b3", the decoder's "br", "wup3", "w3c", "cbr0", "wcc",
 * "wcc_mfma", "bncc", "wup2", "bnu2", "wconv", "wclassifier", "wtail" where the model has them, and the zero "guard" --,
 * *n_pieces (may be NULL) their count. */
gs_status gs_espnet_pack_weights(const float *blob, const gs_layer_desc *table, int n_layers, int classes, int p, int q,
                                 int encoder_only, float *out, size_t cap, size_t *n_floats, gs_weight_piece *pieces, int piece_cap,
                                 int *n_pieces);

/* *bytes = the activation workspace gs_espnet_reserve(h, n, height, width) allocates for ONE lane of such a handle
 * (csrc/workspace_plan.h), or its refusal: GS_ERR_INVALID for a batch or tile size no forward takes, GS_ERR_UNSUPPORTED for
 * classes outside 2..20 and for a tile so large that an activation of one image exceeds 2 GiB. */
gs_status gs_espnet_workspace_plan(int n, int height, int width, int p, int q, int classes, int encoder_only, size_t *bytes);

#ifdef __cplusplus
}
#endif

#endif
