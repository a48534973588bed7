// What the host-only set-up of an ESPNet handle (espnet_weights.h: the weight packer, workspace_plan.h: the activation layout)
// shares with the kernels and the forward plan: the activation descriptor, the float layout of a conv_mfma image, the facts of
// the model by depth and padded class count, the decoder tail's image size.  No HIP: compiles with a plain C++17 compiler, so
// CPU tests and a sanitizer driver reach the set-up.  Included by gs_internal.h; conv_mfma.h, forward_plan.h and
// dec_tail_args.h describe what the definitions below mean to the kernels.
#pragma once
#include <cstddef>

#include "../../include/glomseg.h"

namespace gs {

void set_error(const char *fmt, ...);   // espnet.hip (a stand-alone driver brings its own)

static inline long long round_up(long long a, long long b) { return (a + b - 1) / b * b; }

// A [N][C][H][W] fp32 activation in HBM with a zero halo.  `base` is the start of the allocation of
// image 0; (n,c,y,x) lives at base + n*sn + c*sc + off + y*pitch + x (all in floats).  Kernels only
// ever write the interior, so the halo (zeroed when the workspace is laid out) stays zero and the
// convolution taps that fall outside the image read exact zeros without any predication.
struct Act {
    float *base = nullptr;
    long long sn = 0;   // floats per image
    int sc = 0;         // floats per channel plane
    int pitch = 0;      // floats per row
    int off = 0;        // pad_top*pitch + pad_left
    int C = 0, Cp = 0;  // real / allocated channel planes (extra planes stay zero)
    int H = 0, W = 0;
    size_t bytes(int n) const { return (size_t)n * sn * sizeof(float); }
};

// ---- conv_mfma.h: the F_SIDE1X1 table and the packed image of a configuration
constexpr int SIDE_REC = 8;   // floats per channel record of the table (dec2_record of up to eight classes)
constexpr int SIDE_ZROWS = 16;   // zero rows behind the channels' (a chunk's row groups read rows CINP + g * KL of them for tap row 0)
constexpr int side_table_floats(int CINP) { return (CINP + SIDE_ZROWS) * SIDE_REC; }
// float offset of the side table behind a configuration's image: the F_BNLOAD table is part of the blob of such a reduce
// whether the form applies it or not
constexpr int side_table_offset(int image_total, int CINP, int KL) { return image_total + (3 * (CINP + KL) + 3) / 4 * 4; }

// Float layout of a configuration's packed image in the weight blob: [weights NDIL*TAPS*CINP*NROW | BN scale, shift,
// alpha (3*COUT, twice with F_DUAL) | F_FUSE1X1 table NDIL*NACC*64], rounded up to whole float4s.
struct ConvImage {
    int nrow, cout, w, bn, tab, total;
};
constexpr ConvImage conv_image(int CINP, int TAPS, int NDIL, int NOUT1, int NOUT, bool bn, bool dual = false, int fuse_nacc = 0)
{
    ConvImage im{};
    im.nrow = NOUT1 > NOUT ? NOUT1 : NOUT;
    im.cout = NOUT1 + (NDIL - 1) * NOUT;
    im.w = NDIL * TAPS * CINP * im.nrow;
    im.bn = (bn ? 3 * im.cout : 0) + (dual ? 3 * im.cout : 0);
    im.tab = NDIL * fuse_nacc * 64;
    im.total = (im.w + im.bn + im.tab + 3) / 4 * 4;
    return im;
}
// number of floats of a configuration's image in the weight blob (see conv_image)
constexpr int conv_wfloats(int CINP, int TAPS, int NDIL, int NOUT1, int NOUT, bool bn, bool dual = false, int fuse_nacc = 0)
{
    return conv_image(CINP, TAPS, NDIL, NOUT1, NOUT, bn, dual, fuse_nacc).total;
}

// ---- espnet_config.h: F_FUSE1X1 (the next block's 1x1 reduce computed in a block's epilogue), measured at batch 32
// (profiles/README.md):
//   level 2: down-sampler 0.223 -> 0.242 ms, ESP block 0.189 -> 0.21 ms (three waves per SIMD instead of four), against
//            0.063 ms per separate 1x1 launch: -0.084 ms per step.  On.
//   level 3: down-sampler (no residual: the second accumulator set fits beside four pixels per lane) 0.159 -> 0.175 ms
//            against 0.032 ms for the 1x1 launch: on.  ESP blocks: beside the residual registers the second accumulator
//            set only fits at two pixels per lane, and that form takes 0.1995 ms = exactly branch kernel + 1x1 kernel
//            (0.167 + 0.032); with the residual through a half-slot register ring it fit at four pixels per lane (24
//            registers spilled) and took 0.190-0.197 ms.  Shipped since: two pixels per lane (CFG_L3_BR_P2R, no spill):
//            0.183 ms, because half-row tasks halve the images an XCD has in flight and the reduced maps stay in its L2.
#ifndef CFG_FUSE_L3
#define CFG_FUSE_L3 2   // 0 off, 1 down-sampler only, 2 every block
#endif
#ifndef CFG_FUSE_L2
#define CFG_FUSE_L2 1
#endif

// ---- forward_plan.h: facts of the model that the packing, the workspace and the plan share
// the padded class count the decoder kernels are instantiated for (Model::cp)
constexpr int padded_classes(int classes) { return classes == 5 ? 5 : (classes + 3) / 4 * 4; }
// Lazy b2 (espnet_config.h): output1_0 is stored raw and its consumers apply b2 on load, whenever there is an ESP block
constexpr bool b2_is_lazy(int p) { return p > 0; }
// the 1x1 reduce of ESP block i is computed in the epilogue of the block before it (F_FUSE1X1; block 0: of the down-sampler)
constexpr bool l2_c1_fused(int i, int p) { return CFG_FUSE_L2 && i < p; }
constexpr bool l3_c1_fused(int i, int q) { return (CFG_FUSE_L3 == 2 || (CFG_FUSE_L3 == 1 && i == 0)) && i < q; }
// the decoder by padded class count: combine_l2_l3.1's 3x3 on the matrix cores from twelve planes on (else dec3_kernel),
// the fused tail for the five-class networks (else a conv_mfma launch + dec4_kernel); MFMA rows 16 up to sixteen planes
constexpr bool dec3_on_mfma(int cp) { return cp >= 12; }
// level3_C (the decoder's 1x1 over output1_cat) is computed by the level-3 stride-2 reduce, which has every value of that map
// in a register (F_SIDE1X1), and dec2 reads its `cp` planes instead of the 131.  Five class planes only: at four pixel runs
// per lane the side sums take 2 * cp * 4 registers, and eight planes do not fit beside the reduce's 196-207 without spilling.
constexpr bool l3c_side_sums(int cp) { return cp == 5; }
// The encoder classifier behind b3 (Model.py:368-370) is computed as side sums in the epilogues of the two launches that hold
// its input in registers -- the level-3 down-sampler's branches (output2_0) and the last ESP block (output2): F_CLS1X1,
// conv_mfma.h -- and dec1_sums_kernel adds the partial planes instead of dec1_kernel re-reading both 128-channel maps.  A fact
// of the model only: five class planes (the kernels' record and register budget), at least one ESP block (q = 0 has no
// second producer), and a down-sampler in its fused form (the forms that carry the flag).  The partial planes lie in the
// workspace's `tt`, which is free until dec2 writes it, and the records are the blob piece "b3" as packed: nothing is added.
constexpr bool cls_side_sums(int cp, int q) { return cp == 5 && q >= 1 && l3_c1_fused(0, q); }
// ... 2 producers x 2 lane halves x 5 classes planes of H3 x W3, dense, per image: at most half of tt's 2 * cp planes at 1/4 scale
constexpr int CLS_PART_PLANES = 20;
constexpr bool dec_tail_fused(int cp) { return cp == 5; }

// ---- dec_tail_args.h: the decoder tail's image (DecTailArgs::wpack)
constexpr int DT_A_FLOATS = 18 * 64;
constexpr int DT_PACK_FLOATS = DT_A_FLOATS + 16 + 100;

}  // namespace gs
