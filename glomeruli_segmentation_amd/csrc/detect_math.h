// Device arithmetic that the detector's primitives (detect_ops.hip: gs_nms, gs_roialign) and the assembled detector
// (detector.hip) must compute bit for bit alike: the IoU of two boxes and the bilinear sample of tf.image.crop_and_resize.
#pragma once
#include <hip/hip_runtime.h>

namespace gs {

// IoU of two [ymin,xmin,ymax,xmax] boxes whose corners are ordered (ymin <= ymax, xmin <= xmax); an empty box gives 0.
// The detector's kernels call this directly: decode_clip's outputs are always finite and ordered -- fmaxf(NaN, 0) = 0
// removes NaNs, the decoded sizes hh, ww are >= 0, and padded boxes are all zero.  gs_nms, whose boxes are the caller's,
// normalises the corners first (box_iou).
__device__ __forceinline__ float iou_yxyx(const float *a, const float *b)
{
    const float aa = (a[2] - a[0]) * (a[3] - a[1]), ab = (b[2] - b[0]) * (b[3] - b[1]);
    if (aa <= 0.0f || ab <= 0.0f)
        return 0.0f;
    const float ih = fmaxf(fminf(a[2], b[2]) - fmaxf(a[0], b[0]), 0.0f);
    const float iw = fmaxf(fminf(a[3], b[3]) - fmaxf(a[1], b[1]), 0.0f);
    const float inter = ih * iw;
    return inter / (aa + ab - inter);
}

// Sample (y, x) of the crop x crop grid that tf.image.crop_and_resize (bilinear, extrapolation value 0) lays over the
// normalised box [y1,x1,y2,x2] of image img (inside the batch: the caller's check) of h x w x c NHWC maps: V = float reads
// channel ch, V = float4 channels ch..ch+3 (ch and c multiples of 4).  A grid of one point samples the box's centre.
template <typename V>
__device__ __forceinline__ V crop_resize_sample(const float *feat, int img, int h, int w, int c, int ch, float y1, float x1, float y2, float x2,
                                                int crop, int y, int x)
{
    // every product and sum rounded on its own (no fused multiply-add; the pragma is lexical, so it has to stand here and not
    // in the callers): whether the last sample of a box that ends exactly on the map's border is inside (<= h-1) or
    // extrapolated (0) hangs on the last bit of in_y / in_x, and tf.image.crop_and_resize (and the oracle) round each operation
#pragma clang fp contract(off)
    const float hs = crop > 1 ? (y2 - y1) * (float)(h - 1) / (float)(crop - 1) : 0.0f;
    const float ws = crop > 1 ? (x2 - x1) * (float)(w - 1) / (float)(crop - 1) : 0.0f;
    const float in_y = crop > 1 ? y1 * (float)(h - 1) + (float)y * hs : 0.5f * (y1 + y2) * (float)(h - 1);
    const float in_x = crop > 1 ? x1 * (float)(w - 1) + (float)x * ws : 0.5f * (x1 + x2) * (float)(w - 1);
    V v{};
    if (in_y >= 0.0f && in_y <= (float)(h - 1) && in_x >= 0.0f && in_x <= (float)(w - 1)) {
        const int ty = (int)floorf(in_y), by = (int)ceilf(in_y);
        const int lx = (int)floorf(in_x), rx = (int)ceilf(in_x);
        const float fy = in_y - (float)ty, fx = in_x - (float)lx;
        const float *base = feat + (long long)img * h * w * c + ch;
        const V tl = *reinterpret_cast<const V *>(base + ((long long)ty * w + lx) * c);
        const V tr = *reinterpret_cast<const V *>(base + ((long long)ty * w + rx) * c);
        const V bl = *reinterpret_cast<const V *>(base + ((long long)by * w + lx) * c);
        const V br = *reinterpret_cast<const V *>(base + ((long long)by * w + rx) * c);
        auto lerp2 = [&](float a, float b, float cc, float d) {
            const float top = a + (b - a) * fx, bot = cc + (d - cc) * fx;
            return top + (bot - top) * fy;
        };
        if constexpr (sizeof(V) == sizeof(float))
            v = lerp2(tl, tr, bl, br);
        else
            v = make_float4(lerp2(tl.x, tr.x, bl.x, br.x), lerp2(tl.y, tr.y, bl.y, br.y), lerp2(tl.z, tr.z, bl.z, br.z),
                            lerp2(tl.w, tr.w, bl.w, br.w));
    }
    return v;
}

}  // namespace gs
