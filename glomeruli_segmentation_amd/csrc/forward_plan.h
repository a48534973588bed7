// The kernel-form plan of the ESPNet forward: which conv_mfma_kernel instantiation (or plain kernel) each launch class of
// the forward (espnet.hip: encode, decode) runs for a batch size, a tile size, a model depth, a padded class count and a CU count.
// plan_forward decides, the forward executes: it switches over the plan's forms and asks nothing about widths or task counts
// itself.  Host-only and free of HIP calls; gs_espnet_plan_forward / gs_espnet_form_info (include/glomseg.h) expose the
// function and the table to CPU tests, which is how tests/test_kernel_forms.py knows what a GPU case runs.
// A new form is added in three places: a row of the table, a branch of plan_forward, its Spec in espnet.hip (tuple and mask; the
// class's switch is generated from the table, so a row without a Spec does not compile, and a static_assert there holds the
// row's pixels per lane to the Spec's).  Included by espnet.hip only, after espnet_config.h (whose CFG_* tuples and switches it reads).
#pragma once
#include "espnet_config.h"

namespace gs {

// pixels per lane of a configuration: the 9th element of a CFG_* tuple
constexpr int cfg_pixels(int, int, int, int, int, int, int, int, int p, int) { return p; }

// ---- the facts of the model that the packing, the workspace and the plan share (padded_classes, b2_is_lazy, l2_c1_fused,
// l3_c1_fused, dec3_on_mfma, l3c_side_sums, dec_tail_fused) are in espnet_facts.h; the MFMA shape of the decoder's 3x3 launches:
constexpr int dec_mt(int cp) { return cp <= 16 ? 16 : 32; }
constexpr int dec_pixels(int cp) { return cp <= 16 ? 8 : 4; }

// ---- the table: every launch class of the forward and its forms, X(id, name, pixels per lane of the form's vector pixel
// mapping -- F_VEC, which needs the output width to be a multiple of it -- or 0 for a form without one).  The only place a form
// is named: the enums, the name strings and the ABI's form codes (the position in a class's list) are generated from it.
// "unfused": without the next block's 1x1 in the epilogue.
#define GS_FORMS_L2_DOWN(X)   /* the level-2 down-sampler's branches */                           \
    X(P2S_VEC, "CFG_L2_BR_P2S+F_VEC", cfg_pixels(CFG_L2_BR_P2S))                                  \
    X(P4S_VEC_SKIP, "CFG_L2_BR_P4S+F_VEC+F_SKIP_PAD", cfg_pixels(CFG_L2_BR_P4S))                  \
    X(P4_VEC, "CFG_L2_BR_P4+F_VEC", cfg_pixels(CFG_L2_BR_P4))                                     \
    X(P4, "CFG_L2_BR_P4", 0)                                                                      \
    X(UNFUSED_P4_VEC, "unfused CFG_L2_BR_P4+F_VEC", cfg_pixels(CFG_L2_BR_P4))                     \
    X(UNFUSED_P4, "unfused CFG_L2_BR_P4", 0)
#define GS_FORMS_L2_ESP_FUSED(X)   /* every level-2 ESP block but the last */                     \
    X(P2S_VEC, "CFG_L2_BR_P2S+F_VEC", cfg_pixels(CFG_L2_BR_P2S))                                  \
    X(P4_VEC, "CFG_L2_BR_P4+F_VEC", cfg_pixels(CFG_L2_BR_P4))                                     \
    X(P4, "CFG_L2_BR_P4", 0)                                                                      \
    X(UNFUSED_P4_VEC, "unfused CFG_L2_BR_P4+F_VEC", cfg_pixels(CFG_L2_BR_P4))                     \
    X(UNFUSED_P4, "unfused CFG_L2_BR_P4", 0)
#define GS_FORMS_L2_ESP_LAST(X)   /* the last one: stores only its b2-normalised form */          \
    X(P2S_VEC, "CFG_L2_BR_P2S+F_VEC", cfg_pixels(CFG_L2_BR_P2S))                                  \
    X(P4_VEC, "CFG_L2_BR_P4+F_VEC", cfg_pixels(CFG_L2_BR_P4))                                     \
    X(P4, "CFG_L2_BR_P4", 0)
#define GS_FORMS_CAT_B2(X)   /* b2 as a kernel of its own (no lazy b2) */                         \
    X(KERNEL, "cat_b2_kernel", 0)
#define GS_FORMS_L3_REDUCE(X)   /* the level-3 stride-2 reduce */                                 \
    X(BNL_P1, "CFG_L3_C1S_BNL_P1", 0)                                                             \
    X(BNL, "CFG_L3_C1S_BNL", 0)                                                                   \
    X(C1S, "CFG_L3_C1S", 0)
#define GS_FORMS_L3_DOWN(X)   /* the level-3 down-sampler's branches */                           \
    X(P1R, "CFG_L3_BR_P1R", 0)                                                                    \
    X(P2R_VEC, "CFG_L3_BR_P2R+F_VEC", cfg_pixels(CFG_L3_BR_P2R))                                  \
    X(BR_VEC, "CFG_L3_BR+F_VEC", cfg_pixels(CFG_L3_BR))                                           \
    X(P2F, "CFG_L3_BR_P2F", 0)                                                                    \
    X(UNFUSED_BR_VEC, "unfused CFG_L3_BR+F_VEC", cfg_pixels(CFG_L3_BR))                           \
    X(UNFUSED_BR, "unfused CFG_L3_BR", 0)
#define GS_FORMS_L3_ESP_FUSED(X)   /* the level-3 ESP blocks that compute the next block's 1x1 */ \
    X(P1R, "CFG_L3_BR_P1R", 0)                                                                    \
    X(P2R_VEC, "CFG_L3_BR_P2R+F_VEC", cfg_pixels(CFG_L3_BR_P2R))                                  \
    X(P2F, "CFG_L3_BR_P2F", 0)
#define GS_FORMS_L3_ESP_LAST(X)   /* ... and those that do not: the last one */                   \
    X(P1R, "CFG_L3_BR_P1R", 0)                                                                    \
    X(P2R_VEC, "CFG_L3_BR_P2R+F_VEC", cfg_pixels(CFG_L3_BR_P2R))                                  \
    X(BR_VEC, "CFG_L3_BR+F_VEC", cfg_pixels(CFG_L3_BR))                                           \
    X(P2, "CFG_L3_BR_P2", 0)
#define GS_FORMS_DEC3(X)   /* combine_l2_l3.1's 3x3 (+ up_l2) */                                  \
    X(KERNEL, "dec3_kernel", 0)                                                                   \
    X(MT16, "MFMA MT16", 0)                                                                       \
    X(MT16_VEC, "MFMA MT16+F_VEC", dec_pixels(16))                                                \
    X(MT32, "MFMA MT32", 0)                                                                       \
    X(MT32_VEC, "MFMA MT32+F_VEC", dec_pixels(20))
#define GS_FORMS_DEC_CONV(X)   /* conv CBR(19 + c, c, 3) (+ classifier) */                        \
    X(TAIL, "dec_tail_kernel", 0)                                                                 \
    X(MT16, "MFMA MT16", 0)                                                                       \
    X(MT16_VEC, "MFMA MT16+F_VEC", dec_pixels(16))                                                \
    X(MT32, "MFMA MT32", 0)                                                                       \
    X(MT32_VEC, "MFMA MT32+F_VEC", dec_pixels(20))
#define GS_LAUNCH_CLASSES(C)               \
    C(l2_down, GS_FORMS_L2_DOWN)           \
    C(l2_esp_fused, GS_FORMS_L2_ESP_FUSED) \
    C(l2_esp_last, GS_FORMS_L2_ESP_LAST)   \
    C(cat_b2, GS_FORMS_CAT_B2)             \
    C(l3_reduce, GS_FORMS_L3_REDUCE)       \
    C(l3_down, GS_FORMS_L3_DOWN)           \
    C(l3_esp_fused, GS_FORMS_L3_ESP_FUSED) \
    C(l3_esp_last, GS_FORMS_L3_ESP_LAST)   \
    C(dec3, GS_FORMS_DEC3)                 \
    C(dec_conv, GS_FORMS_DEC_CONV)

struct FormInfo {
    const char *name;
    int pixels_per_lane;
};
struct LaunchClassInfo {
    const char *name;
    const FormInfo *forms;
    int n_forms;
};

#define GS_FORM_ID(id, name, ppl) id,
#define GS_FORM_INFO(id, name, ppl) {name, ppl},
// form::<class>: `none` (a class this model does not launch), then the class's forms in table order
#define GS_CLASS_ENUM(cls, FORMS) enum class cls : int { none = -1, FORMS(GS_FORM_ID) };
#define GS_CLASS_FORMS(cls, FORMS)                                          \
    constexpr FormInfo kForms_##cls[] = {FORMS(GS_FORM_INFO)};              \
    constexpr int pixels_per_lane(form::cls f) { return kForms_##cls[(int)f].pixels_per_lane; }
#define GS_CLASS_INFO(cls, FORMS) {#cls, kForms_##cls, (int)(sizeof kForms_##cls / sizeof kForms_##cls[0])},
#define GS_PLAN_MEMBER(cls, FORMS) form::cls cls = form::cls::none;
#define GS_PLAN_CODE(cls, FORMS) *out++ = (int)cls;
namespace form {
GS_LAUNCH_CLASSES(GS_CLASS_ENUM)
}
GS_LAUNCH_CLASSES(GS_CLASS_FORMS)
constexpr LaunchClassInfo kLaunchClasses[] = {GS_LAUNCH_CLASSES(GS_CLASS_INFO)};
constexpr int kLaunchClassCount = (int)(sizeof kLaunchClasses / sizeof kLaunchClasses[0]);

struct ForwardPlan {
    GS_LAUNCH_CLASSES(GS_PLAN_MEMBER)
    bool lazy_b2 = false;
    bool l3c_in_reduce = false;   // the stride-2 reduce also writes level3_C's raw output (F_SIDE1X1); dec2 reads that
    bool cls_in_l3 = false;       // the level-3 down-sampler and the last ESP block also write the classifier's partial sums
                                  // (F_CLS1X1); dec1_sums_kernel adds them in dec1_kernel's place
    bool lean = false;            // a fact of the REQUEST: no logits are asked for and both side sums are planned, so nothing of the
                                  // forward reads output2 (the last level-3 block's map) -- that launch does not store it
                                  // (F_CLS_ONLY) -- or the normalised cat, which dec2_br_kernel is then not launched for: the
                                  // stages "level3.<q-1>" and "combine_t" do not exist after such a forward
    // one form code per launch class, in table order (the ABI's view of a plan)
    void codes(int *out) const { GS_LAUNCH_CLASSES(GS_PLAN_CODE) }
};
#undef GS_FORM_ID
#undef GS_FORM_INFO
#undef GS_CLASS_ENUM
#undef GS_CLASS_FORMS
#undef GS_CLASS_INFO
#undef GS_PLAN_MEMBER
#undef GS_PLAN_CODE

// the vector pixel mapping of form `v` fits an output width of w
template <typename F>
constexpr bool vec_fits(F v, int w, bool no_vec)
{
    return !no_vec && w % pixels_per_lane(v) == 0;
}

// ---- the forms a block takes without the next block's 1x1: plan_forward's where nothing is fused, and the single-block test
// hook's (gs_espnet_block_forward), which runs a block alone in its whole-row shape at any batch
constexpr form::l2_down unfused_l2_down(int W2, bool no_vec)
{
    return vec_fits(form::l2_down::UNFUSED_P4_VEC, W2, no_vec) ? form::l2_down::UNFUSED_P4_VEC : form::l2_down::UNFUSED_P4;
}
constexpr form::l2_esp_fused unfused_l2_esp(int W2, bool no_vec)
{
    return vec_fits(form::l2_esp_fused::UNFUSED_P4_VEC, W2, no_vec) ? form::l2_esp_fused::UNFUSED_P4_VEC : form::l2_esp_fused::UNFUSED_P4;
}
constexpr form::l3_down unfused_l3_down(int W3, bool no_vec)
{
    return vec_fits(form::l3_down::UNFUSED_BR_VEC, W3, no_vec) ? form::l3_down::UNFUSED_BR_VEC : form::l3_down::UNFUSED_BR;
}
// four consecutive pixels per lane and 16-byte accesses when the width allows it (0.170 ms per launch at batch 32), else the
// two-run mapping with its deeper ring (0.175 ms)
constexpr form::l3_esp_last whole_row_l3_esp(int W3, bool no_vec)
{
    return vec_fits(form::l3_esp_last::BR_VEC, W3, no_vec) ? form::l3_esp_last::BR_VEC : form::l3_esp_last::P2;
}

// What a forward of n tiles of H x W runs on a device with num_cus CUs, for ESPNet(classes, p, q) with cp = padded_classes(classes).
// no_vec (GS_NO_VEC of -DGS_DIAG builds; false in the product) keeps every launch off the vector mappings and the small-batch forms.
// (An ESPNet-C handle -- encoder_only -- stops before the decoder: its dec3 / dec_conv entries are not launched, and nothing of
// it asks for level3_C.)  want_logits: whether the request has a logits buffer (ForwardReq::logits) -- it changes no form, only `lean`.
inline ForwardPlan plan_forward(int n, int H, int W, int p, int q, int cp, int num_cus, bool no_vec, bool encoder_only = false,
                                bool want_logits = true)
{
    namespace f = form;
    const int W1 = W / 2, H2 = H / 4, W2 = W / 4, H3 = H / 8, W3 = W / 8;
    const long long cus = num_cus;
    ForwardPlan pl;
    pl.lazy_b2 = b2_is_lazy(p);
    pl.l3c_in_reduce = !encoder_only && l3c_side_sums(cp);   // in every form of the reduce: lazy or not, any task shape
    pl.cls_in_l3 = !encoder_only && cls_side_sums(cp, q);    // in every form of the two launches: a fact of the model only
    pl.lean = !want_logits && pl.cls_in_l3 && pl.l3c_in_reduce;   // a full five-class network with q >= 1, asked for the mask only

    // ---- level 2.  Small batches: 32-pixel tasks (two pixels per lane) while there are at most CFG_SMALL2_WAVES of them per CU
    const bool small2 = CFG_SMALL2_WAVES > 0 && (long long)n * H2 * cdiv(W2, 64) * 2 <= cus * CFG_SMALL2_WAVES &&
                        vec_fits(f::l2_down::P2S_VEC, W2, no_vec);
    if (!l2_c1_fused(0, p))
        pl.l2_down = unfused_l2_down(W2, no_vec);
    else if (small2)
        pl.l2_down = f::l2_down::P2S_VEC;
    else if (CFG_L2_DOWN_SKIP && vec_fits(f::l2_down::P4S_VEC_SKIP, W2, no_vec))   // tap-row chunks, tap rows in the zero halo skipped
        pl.l2_down = f::l2_down::P4S_VEC_SKIP;
    else
        pl.l2_down = vec_fits(f::l2_down::P4_VEC, W2, no_vec) ? f::l2_down::P4_VEC : f::l2_down::P4;
    if (p > 1) {
        if (!l2_c1_fused(1, p))
            pl.l2_esp_fused = unfused_l2_esp(W2, no_vec);
        else if (small2)
            pl.l2_esp_fused = f::l2_esp_fused::P2S_VEC;
        else
            pl.l2_esp_fused = vec_fits(f::l2_esp_fused::P4_VEC, W2, no_vec) ? f::l2_esp_fused::P4_VEC : f::l2_esp_fused::P4;
    }
    if (p > 0)
        pl.l2_esp_last = small2                                            ? f::l2_esp_last::P2S_VEC
                         : vec_fits(f::l2_esp_last::P4_VEC, W2, no_vec) ? f::l2_esp_last::P4_VEC
                                                                          : f::l2_esp_last::P4;
    if (!pl.lazy_b2)
        pl.cat_b2 = f::cat_b2::KERNEL;

    // ---- level 3.  The stride-2 reduce: whole-row tasks (128 pixels) are one per wave at batch 32; below a quarter of that the
    // row is cut into 32-pixel tasks (batch 1: 64 -> 256 tasks, profiles/r04_latency.json).  Without lazy b2 the plain form.
    if (!pl.lazy_b2)
        pl.l3_reduce = f::l3_reduce::C1S;
    else
        pl.l3_reduce = (long long)n * H3 * cdiv(W3, 128) * 4 <= cus * 8 ? f::l3_reduce::BNL_P1 : f::l3_reduce::BNL;
    // Small batches: a half-row task per SIMD does not fill the chip below 8 tiles (64 rows x 2 strips x n tasks for 1024
    // SIMDs); with 32-pixel strips (one pixel per lane, the same accumulation chain per pixel: same bits) there are twice as
    // many, each half as long.  Used up to one such task per wave slot (CFG_SMALL3_WAVES per CU: 8 tiles).
    const bool small3 = (long long)n * H3 * cdiv(W3, 64) * 2 <= cus * CFG_SMALL3_WAVES && !no_vec;
    if (!l3_c1_fused(0, q))
        pl.l3_down = unfused_l3_down(W3, no_vec);
    else if (small3)
        pl.l3_down = f::l3_down::P1R;
    else if (CFG_L3_DOWN_P2 && vec_fits(f::l3_down::P2R_VEC, W3, no_vec))
        pl.l3_down = f::l3_down::P2R_VEC;
    else   // no residual here: the four-pixel vector mapping still fits with the second accumulator set -- but not with the
           // classifier's twenty running sums on top (F_CLS1X1: 256 registers and 96 bytes of scratch), so a model that has them
           // takes the two-pixel form; only builds with CFG_L3_DOWN_P2 = 0 ever get here with an even width
        pl.l3_down = !pl.cls_in_l3 && vec_fits(f::l3_down::BR_VEC, W3, no_vec) ? f::l3_down::BR_VEC : f::l3_down::P2F;
    // Fused ESP blocks: two consecutive pixels per lane, a 13-step operand ring (CFG_L3_RING), a whole slot's residual in
    // registers.  A task is then half a row, so the 256 waves of an XCD have TWO images in flight instead of four and the
    // reduced maps the taps re-read stay in that XCD's 4 MiB L2: beyond-L2 fetch of a launch 542 -> 296 MB, 0.1898 -> 0.1834 ms
    // (profiles/README.md).  Small batches: one pixel per lane, a whole slot's residual requested a dilation ahead.
    if (q > 1 && l3_c1_fused(1, q))
        pl.l3_esp_fused = small3                                              ? f::l3_esp_fused::P1R
                          : vec_fits(f::l3_esp_fused::P2R_VEC, W3, no_vec) ? f::l3_esp_fused::P2R_VEC
                                                                             : f::l3_esp_fused::P2F;
    if (q > 0) {
        if (small3)
            pl.l3_esp_last = f::l3_esp_last::P1R;
        else if (CFG_L3_LAST_P2 && vec_fits(f::l3_esp_last::P2R_VEC, W3, no_vec))   // the half-row task shape of the fused blocks
            pl.l3_esp_last = f::l3_esp_last::P2R_VEC;
        else
            pl.l3_esp_last = whole_row_l3_esp(W3, no_vec);
    }

    // ---- decoder
    if (!dec3_on_mfma(cp))
        pl.dec3 = f::dec3::KERNEL;
    else if (dec_mt(cp) == 16)
        pl.dec3 = vec_fits(f::dec3::MT16_VEC, W2, no_vec) ? f::dec3::MT16_VEC : f::dec3::MT16;
    else
        pl.dec3 = vec_fits(f::dec3::MT32_VEC, W2, no_vec) ? f::dec3::MT32_VEC : f::dec3::MT32;
    if (dec_tail_fused(cp))
        pl.dec_conv = f::dec_conv::TAIL;
    else if (dec_mt(cp) == 16)
        pl.dec_conv = vec_fits(f::dec_conv::MT16_VEC, W1, no_vec) ? f::dec_conv::MT16_VEC : f::dec_conv::MT16;
    else
        pl.dec_conv = vec_fits(f::dec_conv::MT32_VEC, W1, no_vec) ? f::dec_conv::MT32_VEC : f::dec_conv::MT32;
    return pl;
}

}  // namespace gs
