/*
 * glomseg_forms.h -- what a kernel form of the ESPNet forward plan's table carries beyond its name (an addition to glomseg.h;
 * the ABI number stays: no signature changes, and a caller finds out whether a library has the entry by looking the symbol up).
 */
#ifndef GLOMSEG_FORMS_H
#define GLOMSEG_FORMS_H

#include "glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only, no handle and no device.  F_ODD_2B (csrc/conv_mfma.h: the odd last input channel of a level-3 branch convolution
 * in one two-block K = 1 matrix instruction per pixel-group pair) of form `form` of launch class `launch_class`, both numbered
 * as gs_espnet_form_info numbers them: bit 0 (GS_FORM_ODD_2B_LEGAL) = the form may carry it -- a level-3 branch form with its
 * pixel groups in pairs and a tap row per chunk --, bit 1 (GS_FORM_ODD_2B_BUILT) = its kernels in this library do: every legal
 * form unless the library is a -DCFG_L3_ODD_2B=0 build (GS_BUILD_NO_ODD_2B of gs_build_flags).  -1 past the last class or form. */
#define GS_FORM_ODD_2B_LEGAL 1
#define GS_FORM_ODD_2B_BUILT 2
int gs_espnet_form_odd_2b(int launch_class, int form);

#ifdef __cplusplus
}
#endif

#endif
