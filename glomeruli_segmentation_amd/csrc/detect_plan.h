// The host plan of the detector half: the constants of the graph, its layer table, which NHWC convolution kernel a shape
// runs (conv_nhwc_form) and, for a batch of n windows of H x W, the size chain, every layer's shape and kernel, the workspace
// carve-up and the batch limits (plan_detector).  The plan decides, the launchers execute: launch_conv2d_nhwc
// (detect_ops.hip) switches over conv_nhwc_form's answer, gs_detector_forward (detector.hip) runs plan_detector's result and
// asks nothing about sizes itself.  Host-only and free of HIP calls; gs_conv2d_nhwc_form, gs_detector_layer_info and
// gs_detector_plan (include/glomseg.h) expose it to CPU tests and to the Python package, which keeps no copy of any of this.
// A layer is added as a row of kDetLayers (and its step in plan_detector and gs_detector_forward); a convolution kernel as a
// gs_conv_form value with its name, a branch of conv_nhwc_form and a `case` of launch_conv2d_nhwc's switch.
#pragma once
#include <cstddef>
#include <cstdio>

#include "../../include/glomseg.h"

namespace gs {

constexpr int DET_A = 12;            // anchors per cell: scales {0.25,0.5,1,2} x aspect ratios {0.5,1,2}
constexpr int DET_STRIDE = 16;       // feature stride
constexpr float DET_BASE = 256.0f;   // anchor base size (TF object-detection grid_anchor_generator)
constexpr int DET_PRE_NMS = 1024;    // RPN candidates kept by score before NMS
constexpr int DET_PROPOSALS = 300;   // first_stage_max_proposals
constexpr int DET_CROP = 14;         // initial_crop_size; followed by a 2x2 max-pool
constexpr int DET_POOLED = DET_CROP / 2;
constexpr int DET_HEAD_K = 512;      // second-stage candidates sorted before NMS (the power of two above DET_PROPOSALS)
constexpr int DET_MAX_DET = 100;     // max_total_detections
constexpr int DET_CF = 256;          // feature channels
constexpr int DET_CH = 128;          // box-head channels

// ---- the graph's convolutions, in launch order; weights are [k,k,cin,cout] under name + ".weight", biases under ".bias"
enum DetLayerId { L_C1, L_C2, L_C3, L_C4, L_C5, L_C6, L_RPN, L_RPN_HEAD, L_H1, L_H2, L_FC, DET_LAYERS };
struct DetLayerRow {
    const char *name;
    int k, cin, cout, stride, pad, relu;
};
constexpr DetLayerRow kDetLayers[DET_LAYERS] = {
    {"backbone.c1", 3, 16, 64, 1, 1, 1},   // on the space-to-depth input: 12 channels padded to 16
    {"backbone.c2", 3, 64, 64, 1, 1, 1},   // after the 3x3 / stride-2 max-pool
    {"backbone.c3", 3, 64, 128, 2, 1, 1},
    {"backbone.c4", 3, 128, 128, 1, 1, 1},
    {"backbone.c5", 3, 128, DET_CF, 2, 1, 1},
    {"backbone.c6", 3, DET_CF, DET_CF, 1, 1, 1},
    {"rpn.conv", 3, DET_CF, DET_CF, 1, 1, 1},
    {"rpn.head", 1, DET_CF, 6 * DET_A, 1, 0, 0},   // 2A class logits + 4A box deltas
    {"head.h1", 1, DET_CF, DET_CH, 1, 0, 1},       // on the pooled 7x7 crops of every proposal
    {"head.h2", 3, DET_CH, DET_CH, 2, 1, 1},
    {"head.fc", 1, DET_CH, 6, 1, 0, 0},            // on the spatial mean: 2 class logits + 4 box deltas
};

// ---- which NHWC convolution kernel a shape runs
constexpr const char *kConvFormNames[] = {"generic", "smallcin", "tiled", "wide"};   // by gs_conv_form
struct ConvShape {
    int n, h, w, cin, kh, kw, cout, stride, pad;
};
// The 64 x 64 kernels address the input and the weights with 32-bit byte offsets behind buffer descriptors, and a lane with
// nothing to read uses the byte offset NHWC_OOB, which must lie beyond every descriptor to read as 0: a tensor those kernels
// take has at most NHWC_OOB bytes (conv_nhwc_form: in32, w32), so the offset is at or past the end of any of them.
constexpr int NHWC_OOB = 0x7ffffff0;
constexpr long long NHWC_MAX_BYTES = NHWC_OOB;

struct ConvPlan {
    gs_status status = GS_OK;
    const char *message = "";   // of a refusal
    gs_conv_form form = GS_CONV_GENERIC;
    int ho = 0, wo = 0;
    unsigned grid_x = 0, grid_y = 0;   // workgroups of 256 threads
};

// packed: the weights went through conv2d_nhwc_pack4, which only the tiled and wide kernels read -- a flag beside the form,
// not a form: a shape those kernels cannot take is refused.
inline ConvPlan conv_nhwc_form(const ConvShape &s, bool packed)
{
    ConvPlan p;
    p.ho = (s.h + 2 * s.pad - s.kh) / s.stride + 1;
    p.wo = (s.w + 2 * s.pad - s.kw) / s.stride + 1;
    const bool empty = p.ho <= 0 || p.wo <= 0;
    // the 64 x 64 kernels address the input and the weights with 32-bit byte offsets, NHWC_OOB being "no data"
    const bool in32 = (long long)s.n * s.h * s.w * s.cin * 4 <= NHWC_MAX_BYTES;
    const bool w32 = (long long)s.kh * s.kw * s.cin * s.cout * 4 <= NHWC_MAX_BYTES;
    const bool tiled = s.cin % 8 == 0 && in32 && w32;   // 8-channel chunks
    if (packed && (empty || !tiled)) {
        // (the message keeps the name of the entry point this check used to live in)
        p.status = GS_ERR_UNSUPPORTED, p.message = "conv2d_nhwc_packed4: shape not supported by the packed-weight kernel";
        return p;
    }
    if (empty) {
        p.status = GS_ERR_INVALID, p.message = "gs_conv2d_nhwc: empty output";
        return p;
    }
    const long long npix = (long long)s.n * p.ho * p.wo;
    if (tiled)
        // whole-line activation fetches where a pixel has at least a line of channels and the map is not a handful of pixels.
        // Measured on the detector (16 windows of 1000 x 1000): 64..256-channel backbone layers 86-90 -> 98-119 TFLOP/s; the
        // 16-channel first layer at two chunks per block 876 -> 1026 us and the box head's 7x7 -> 4x4 layer 264 -> 312 us,
        // so those stay on the chunk-at-a-time kernel.
        p.form = s.cin % 32 == 0 && p.ho * p.wo >= 64 ? GS_CONV_WIDE : GS_CONV_TILED;
    else if (s.cin < 8 && (long long)s.kh * s.kw * s.cin <= 512 && s.kh < 1024 && s.kw < 1024 && in32)
        // few input channels: flattened-K kernel (K = kh*kw*cin up to 512, channel / tap indices below 1024)
        p.form = GS_CONV_SMALLCIN;
    else
        p.form = GS_CONV_GENERIC;
    // a workgroup is four waves along the pixel axis; the generic kernel's wave tile is 32 x 32, the others' 64 x 64
    const int tile = p.form == GS_CONV_GENERIC ? 32 : 64;
    p.grid_x = (unsigned)((npix + 4 * tile - 1) / (4 * tile));
    p.grid_y = (unsigned)((s.cout + tile - 1) / tile);
    return p;
}

// ---- a forward of n windows of H x W
struct DetPiece {
    size_t off = 0, bytes = 0;
};
struct DetLayerPlan {
    long long images = 0;   // n, or n * DET_PROPOSALS in the box head
    int in_h = 0, in_w = 0;
    ConvPlan conv;          // with packed = true: the handle packs its weights
};
struct DetectorPlan {
    gs_status status = GS_OK;
    char message[160] = "";                    // of a refusal
    int h2, w2, h4, w4, h8, w8, hf, wf;        // c1's map (space-to-depth), after the max-pool, after c3, after c5
    long long cells, anchors;                  // per window
    DetLayerPlan layer[DET_LAYERS];
    // the workspace, pieces in this order, each rounded up to 256 bytes (floats unless noted)
    DetPiece A, B;                             // ping (largest: c1's output), pong
    DetPiece F, R, S;                          // features, RPN head output, objectness of every anchor
    DetPiece I1, S1, B1;                       // top DET_PRE_NMS: anchor index (int), score, box
    DetPiece M;                                // suppression masks (64-bit words), both NMS stages
    DetPiece K1, N1;                           // kept positions and their count (int)
    DetPiece P, Pn, Bi;                        // proposals in pixels, normalised, image index of every box (int)
    DetPiece C, C2;                            // box-head intermediates (the 14x14 crops are never materialised)
    DetPiece H, S2, B2;                        // head output, second-stage score and box of every proposal
    DetPiece I2, S2s, B2s;                     // top DET_HEAD_K: proposal index (int), score, box
    DetPiece K2, N2;                           // kept positions and their count (int)
    size_t total = 0;
};

inline DetectorPlan plan_detector(int n, int H, int W)
{
    DetectorPlan pl{};
    if (!(n > 0 && H >= 32 && W >= 32)) {
        pl.status = GS_ERR_INVALID;
        snprintf(pl.message, sizeof pl.message, "gs_detector_forward: windows must be at least 32x32 (got %dx%d, n=%d)", H, W, n);
        return pl;
    }
    // one layer on `images` maps of h x w; h, w become its output size
    auto layer = [&](DetLayerId id, long long images, int &h, int &w) {
        const DetLayerRow &r = kDetLayers[id];
        DetLayerPlan &l = pl.layer[id];
        l.images = images, l.in_h = h, l.in_w = w;
        l.conv = conv_nhwc_form({(int)images, h, w, r.cin, r.k, r.k, r.cout, r.stride, r.pad}, true);
        h = l.conv.ho, w = l.conv.wo;
    };
    int h = (H + 1) / 2, w = (W + 1) / 2;   // 2x2 space-to-depth, an odd edge padded
    pl.h2 = h, pl.w2 = w;
    layer(L_C1, n, h, w);
    h = (h + 2 - 3) / 2 + 1, w = (w + 2 - 3) / 2 + 1;   // max-pool 3x3 s2 p1
    pl.h4 = h, pl.w4 = w;
    layer(L_C2, n, h, w);
    layer(L_C3, n, h, w);
    pl.h8 = h, pl.w8 = w;
    layer(L_C4, n, h, w);
    layer(L_C5, n, h, w);
    pl.hf = h, pl.wf = w;
    layer(L_C6, n, h, w);
    layer(L_RPN, n, h, w);
    layer(L_RPN_HEAD, n, h, w);
    const long long nP = (long long)n * DET_PROPOSALS;
    h = w = DET_POOLED;
    layer(L_H1, nP, h, w);
    layer(L_H2, nP, h, w);
    h = w = 1;   // spatial mean
    layer(L_FC, nP, h, w);

    const int h2 = pl.h2, w2 = pl.w2, P = DET_PROPOSALS, K1 = DET_PRE_NMS, K2 = DET_HEAD_K;
    constexpr int crop_px = DET_POOLED * DET_POOLED;
    const int c1_in = kDetLayers[L_C1].cin, c1_out = kDetLayers[L_C1].cout, c2_out = kDetLayers[L_C2].cout;
    pl.cells = (long long)pl.hf * pl.wf, pl.anchors = pl.cells * DET_A;
    // (the top-k keys hold an anchor index beside the score; the tiled convolution addresses a whole input tensor with
    // 32-bit byte offsets)
    if (!(pl.anchors < (1 << 24) && (long long)n * h2 * w2 * c1_in * 4 < 0x7fffffffLL &&
          nP * crop_px * DET_CF * 4 < 0x7fffffffLL)) {
        pl.status = GS_ERR_INVALID;
        snprintf(pl.message, sizeof pl.message, "gs_detector_forward: batch too large (n=%d windows of %dx%d): split it", n, H, W);
        return pl;
    }
    auto piece = [&](size_t bytes) {
        DetPiece p{pl.total, bytes};
        pl.total += (bytes + 255) / 256 * 256;
        return p;
    };
    const size_t sn = (size_t)n, cells = (size_t)pl.cells;
    const size_t in_b = sn * h2 * w2 * c1_in * 4, pool_b = sn * pl.h4 * pl.w4 * c2_out * 4;
    pl.A = piece(sn * h2 * w2 * c1_out * 4);
    pl.B = piece(in_b > pool_b ? in_b : pool_b);
    pl.F = piece(sn * cells * DET_CF * 4);
    pl.R = piece(sn * cells * 6 * DET_A * 4);
    pl.S = piece(sn * (size_t)pl.anchors * 4);
    pl.I1 = piece(sn * K1 * 4), pl.S1 = piece(sn * K1 * 4), pl.B1 = piece(sn * K1 * 16);
    pl.M = piece(sn * K1 * (K1 / 64) * 8);
    pl.K1 = piece(sn * P * 4), pl.N1 = piece(sn * 4);
    pl.P = piece(sn * P * 16), pl.Pn = piece(sn * P * 16), pl.Bi = piece(sn * P * 4);
    pl.C = piece(sn * P * crop_px * DET_CH * 4);
    pl.C2 = piece(sn * P * crop_px * DET_CF * 4);
    pl.H = piece(sn * P * 6 * 4), pl.S2 = piece(sn * P * 4), pl.B2 = piece(sn * P * 16);
    pl.I2 = piece(sn * K2 * 4), pl.S2s = piece(sn * K2 * 4), pl.B2s = piece(sn * K2 * 16);
    pl.K2 = piece(sn * DET_MAX_DET * 4), pl.N2 = piece(sn * 4);
    return pl;
}

}  // namespace gs
