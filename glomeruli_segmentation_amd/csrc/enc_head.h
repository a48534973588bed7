// enc_head_kernel: the head of ESPNet-C (the encoder-only network, --modelType 2).  The reference upsamples the encoder's
// 1/8-scale logits x8 bilinearly and takes the per-pixel argmax (VisualizeResults_iou.py:125-128,258-261:
// torch.nn.Upsample(scale_factor=8, mode='bilinear') then img_out[0].max(0)[1]); this kernel reads the 1/8-scale logits
// [n][classes][H/8][W/8] that dec1_kernel wrote and writes the class map uint8 [n][H][W] and the per-class pixel counts
// [n][classes].  No full-resolution logits are ever written.
//
// The arithmetic, the only definition of it (tests/test_espnet_c.py restates it in numpy fp32):
//
//   s(d)  = max((d + 0.5f) * 0.125f - 0.5f, 0)      i0 = floor(s), i1 = min(i0 + 1, n_src - 1)
//   w1 = s - i0, w0 = 1 - w1                         (multiples of 1/16: exact in fp32)
//   top = fadd(fmul(wx0, L[y0][x0]), fmul(wx1, L[y0][x1]))
//   bot = fadd(fmul(wx0, L[y1][x0]), fmul(wx1, L[y1][x1]))
//   v   = fadd(fmul(wy0, top), fmul(wy1, bot))       every fmul / fadd rounded to nearest on its own, no contraction
//   class(y, x) = first maximum of v over the classes (strict >, ascending class index: torch's rule, as dec_tail's)
//
// Mapping.  Output rows 8b-4 .. 8b+3 (b = 0 .. H/8; the first and the last block hold four rows of the image) all take
// their two taps from source rows max(b-1, 0) and min(that + 1, H/8 - 1), and four consecutive output columns starting at a
// multiple of four share their two source columns.  A lane owns such a 4 x 8 block: per class it loads FOUR source values,
// forms the four `top` and four `bot` values once and the 32 results from them, and keeps a running first maximum.  A row of
// its block leaves as one dword, so a wave stores 256 contiguous bytes per row.  Every source value is read by 64 output
// pixels but loaded by two lanes only; the whole source (5 MB per 32 tiles) stays in L2.
// Counts: packed 12-bit lane counters, five classes per 64-bit word (NW words per lane).  A lane adds at most 32 and a wave at
// most 2 048 to a field, so the PACKED words are added over the wave by a butterfly (six 64-bit shuffles per word, not per
// class); lane 0 unpacks them into one LDS atomic per class per wave, then one global atomic per class per workgroup.  hist was
// zeroed by the first kernel of the forward.
#pragma once
#include <hip/hip_runtime.h>

namespace gs {

struct EncHeadArgs {
    const float *logits;        // [N][classes][H3][W3]
    unsigned char *mask;        // [N][8 * H3][8 * W3]
    unsigned long long *hist;   // [N][classes], or null
    int classes, H3, W3;
};

// hipcc compiles with -ffp-contract=fast, and the headers' __fmul_rn / __fadd_rn are inline `*` / `+` that it contracts like any
// other (the first build of this kernel held 40 v_pk_fma_f32): the products and sums below are plain operators under this
// pragma, which is what keeps them apart (no v_fma / v_pk_fma left in the ISA; the GPU test compares every pixel's bits).
#define ENC_HEAD_NO_CONTRACT _Pragma("clang fp contract(off)")

// source position of output coordinate d: the clamped s(d) above (exact in fp32 with or without contraction)
__device__ __forceinline__ float enc_head_src(int d)
{
    ENC_HEAD_NO_CONTRACT
    return fmaxf(((float)d + 0.5f) * 0.125f - 0.5f, 0.0f);
}

template <int NW>
__global__ void __launch_bounds__(256) enc_head_kernel(const EncHeadArgs a)
{
    ENC_HEAD_NO_CONTRACT
    __shared__ unsigned lh[5 * NW];
    if (threadIdx.x < 5 * NW)
        lh[threadIdx.x] = 0;
    __syncthreads();
    const int n = blockIdx.y;
    const int H3 = a.H3, W3 = a.W3, H = 8 * H3, W = 8 * W3;
    const int G = 2 * W3;                    // four-column groups per row
    const int idx = blockIdx.x * 256 + threadIdx.x;
    unsigned long long counts[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q)
        counts[q] = 0;
    if (idx < (H3 + 1) * G) {
        const int b = idx / G, x = (idx - b * G) * 4;
        const int ya = 8 * b - 4;            // first row of the block (negative in block 0: rows 0..3 of it are not stored)
        // the taps the whole block shares
        const int x0 = (int)enc_head_src(x), x1 = min(x0 + 1, W3 - 1);
        const int y0 = max(b - 1, 0), y1 = min(y0 + 1, H3 - 1);
        float wx0[4], wx1[4], wy0[8], wy1[8];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            wx1[p] = enc_head_src(x + p) - (float)x0;
            wx0[p] = 1.0f - wx1[p];
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            wy1[r] = enc_head_src(ya + r) - (float)y0;
            wy0[r] = 1.0f - wy1[r];
        }
        const long long plane = (long long)H3 * W3;
        const float *src = a.logits + (long long)n * a.classes * plane;
        const int o00 = y0 * W3 + x0, o01 = y0 * W3 + x1, o10 = y1 * W3 + x0, o11 = y1 * W3 + x1;
        float best[8][4] = {};
        unsigned cls[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // a row's four class indices, one byte each
        for (int k = 0; k < a.classes; ++k) {
            const float *pl = src + k * plane;
            const float l00 = pl[o00], l01 = pl[o01], l10 = pl[o10], l11 = pl[o11];
            float top[4], bot[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                top[p] = wx0[p] * l00 + wx1[p] * l01;
                bot[p] = wx0[p] * l10 + wx1[p] * l11;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float v = wy0[r] * top[p] + wy1[r] * bot[p];
                    const bool up = k == 0 || v > best[r][p];
                    best[r][p] = up ? v : best[r][p];
                    cls[r] = up ? (cls[r] & ~(0xffu << (8 * p))) | ((unsigned)k << (8 * p)) : cls[r];
                }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int y = ya + r;
            if (y < 0 || y >= H)
                continue;
            *reinterpret_cast<unsigned *>(a.mask + ((long long)n * H + y) * W + x) = cls[r];   // x and W are multiples of 4
            if (a.hist) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const unsigned vc = (cls[r] >> (8 * p)) & 0xffu;
                    if (NW == 1) {
                        counts[0] += 1ull << (12 * vc);
                    } else {
#pragma unroll
                        for (int q = 0; q < NW; ++q)
                            if (vc / 5 == (unsigned)q)
                                counts[q] += 1ull << (12 * (vc % 5));
                    }
                }
            }
        }
    }
    if (a.hist) {
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            unsigned long long w = counts[q];
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1)
                w += __shfl_xor(w, sh, 64);
            if ((threadIdx.x & 63) == 0) {
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const unsigned c = (unsigned)((w >> (12 * j)) & 0xfffull);
                    if (c)
                        atomicAdd(&lh[5 * q + j], c);
                }
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < a.classes && lh[threadIdx.x])
            atomicAdd(&a.hist[(long long)n * a.classes + threadIdx.x], (unsigned long long)lh[threadIdx.x]);
    }
}

inline void launch_enc_head(const EncHeadArgs &a, int n, hipStream_t s)
{
    const dim3 grid((unsigned)(((a.H3 + 1) * 2 * a.W3 + 255) / 256), (unsigned)n);
    switch ((a.classes + 4) / 5) {
    case 1: hipLaunchKernelGGL(enc_head_kernel<1>, grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL(enc_head_kernel<2>, grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL(enc_head_kernel<3>, grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL(enc_head_kernel<4>, grid, dim3(256), 0, s, a); break;
    }
}

}  // namespace gs
