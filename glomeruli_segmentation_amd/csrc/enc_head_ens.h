// enc_head_ens_kernel: the head of an ESPNet-C ENSEMBLE.  Every member's trunk has left its 1/8-scale logits
// [n][classes][H/8][W/8] in its own workspace (dec1_kernel); this one launch reads the K small maps, upsamples each x8 with the
// arithmetic of enc_head.h, forms the K softmaxes, averages them in registers and writes the class map uint8 [n][H][W] and the
// per-class pixel counts [n][classes].  No probability tensor and no full-resolution logits are ever written.
//
// The definition (tests/test_espnet_c_ensemble.py restates it in numpy).  v_k[c](y, x) is member k's
// upsampled logit, exactly enc_head.h's expression (taps, weights, every product and sum rounded on its own).  Per pixel:
//
//   m_k   = max_c v_k[c]
//   s_k   = sum_c expf(v_k[c] - m_k)                        ascending c
//   P[c]  = sum_k (expf(v_k[c] - m_k) / s_k) * (1 / K)      ascending k
//   class = first maximum of P (strict >, ascending class index)
//
// Classes (2..20) and K (1..GS_MAX_ENSEMBLE_C) are run-time values, so nothing per class is kept: pass 1 walks member by member
// over the classes twice (maximum, then sum) and keeps m_k and s_k, 2 K values per pixel; pass 2 goes class-outer and
// member-inner, recomputes v_k[c] and keeps only P[c] and the running first maximum.  v_k[c] is therefore formed three times
// (four loads that hit L2 / L1 and ~5 VALU operations per pixel) and expf twice per (member, class): cheaper than any place to
// keep classes x K values.  The member loops are unrolled to GS_MAX_ENSEMBLE_C with a uniform `k < K` test so that m_k / s_k
// are registers, not a run-time-indexed array in scratch.
//
// Mapping.  As in enc_head.h the output rows 8b-4 .. 8b+3 share their two source rows and four columns starting at a multiple
// of four share their two source columns; a lane owns EHE_ROWS = 2 rows x 4 columns of such a block (8 pixels: 16 K values of
// pass-1 state, a quarter of the single-model head's block).  Consecutive lanes own consecutive column groups of the same rows:
// a row of a lane's block leaves as one dword and a wave stores 256 contiguous bytes per row.  The table of the K members'
// pointers travels as a kernel argument: a call allocates nothing and copies nothing.
// Counts: as enc_head_kernel -- packed 12-bit lane counters (a lane adds at most 8, a wave at most 512 to a field), a butterfly
// over the wave on the packed words, one LDS atomic per class per wave, one global atomic per class per workgroup.  hist was
// zeroed by the first kernel of the first member's forward.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/glomseg.h"
#include "enc_head.h"

namespace gs {

struct EncHeadEnsArgs {
    const float *logits[GS_MAX_ENSEMBLE_C];   // member k: [N][classes][H3][W3]
    unsigned char *mask;                      // [N][8 * H3][8 * W3]
    unsigned long long *hist;                 // [N][classes], or null
    int classes, members, H3, W3;
    float inv_members;                        // 1 / K
};

constexpr int EHE_ROWS = 2;            // output rows per lane (divides 4: a lane's rows are inside the image together or not at all)
constexpr int EHE_PX = 4 * EHE_ROWS;   // pixels per lane

// the taps and weights a lane's block shares
struct EheTaps {
    unsigned o00, o01, o10, o11;   // offsets into a class plane
    float wx0[4], wx1[4], wy0[EHE_ROWS], wy1[EHE_ROWS];
};

// one class plane of one member at the lane's pixels: enc_head.h's expression.  `img` (the member's image: uniform over the
// workgroup, a scalar base) and `pc` (the plane's offset in it, uniform too) + the lane's 32-bit tap offsets: one scalar base
// and a 32-bit lane offset per load, not a 64-bit lane address per (member, tap) kept across the class loops
__device__ __forceinline__ void ehe_upsample(const float *img, unsigned pc, const EheTaps &t, float v[EHE_PX])
{
    ENC_HEAD_NO_CONTRACT
    const float l00 = img[pc + t.o00], l01 = img[pc + t.o01], l10 = img[pc + t.o10], l11 = img[pc + t.o11];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float top = t.wx0[p] * l00 + t.wx1[p] * l01;
        const float bot = t.wx0[p] * l10 + t.wx1[p] * l11;
#pragma unroll
        for (int r = 0; r < EHE_ROWS; ++r)
            v[4 * r + p] = t.wy0[r] * top + t.wy1[r] * bot;
    }
}

template <int NW>
__global__ void __launch_bounds__(256) enc_head_ens_kernel(const EncHeadEnsArgs a)
{
    ENC_HEAD_NO_CONTRACT
    __shared__ unsigned lh[5 * NW];
    if (threadIdx.x < 5 * NW)
        lh[threadIdx.x] = 0;
    __syncthreads();
    const int n = blockIdx.y;
    const int H3 = a.H3, W3 = a.W3, H = 8 * H3, W = 8 * W3;
    const int G = 2 * W3;                    // four-column groups per row
    constexpr int SUB = 8 / EHE_ROWS;        // lane blocks down one 8-row block
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int unit = idx / G;                // (b, sub-block) of the lane
    const int b = unit / SUB;
    const int x = (idx - unit * G) * 4;
    const int ya = 8 * b - 4 + EHE_ROWS * (unit - b * SUB);   // first row of the lane's block
    unsigned long long counts[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q)
        counts[q] = 0;
    // (block 0 holds rows -4..3 and block H3 rows H-4..H+3: their outer halves are not part of the image)
    if (b <= H3 && ya >= 0 && ya < H) {
        EheTaps t;
        {
            const int x0 = (int)enc_head_src(x), x1 = min(x0 + 1, W3 - 1);
            const int y0 = max(b - 1, 0), y1 = min(y0 + 1, H3 - 1);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                t.wx1[p] = enc_head_src(x + p) - (float)x0;
                t.wx0[p] = 1.0f - t.wx1[p];
            }
#pragma unroll
            for (int r = 0; r < EHE_ROWS; ++r) {
                t.wy1[r] = enc_head_src(ya + r) - (float)y0;
                t.wy0[r] = 1.0f - t.wy1[r];
            }
            t.o00 = (unsigned)(y0 * W3 + x0), t.o01 = (unsigned)(y0 * W3 + x1);
            t.o10 = (unsigned)(y1 * W3 + x0), t.o11 = (unsigned)(y1 * W3 + x1);
        }
        const int classes = a.classes, K = a.members;
        const unsigned plane = (unsigned)(H3 * W3);   // (one image's logits are classes * plane < 2^31 / 64 floats)
        const long long img = (long long)n * classes * plane;
        // ---- pass 1: m_k and s_k of every member
        float mk[GS_MAX_ENSEMBLE_C][EHE_PX], sk[GS_MAX_ENSEMBLE_C][EHE_PX];
#pragma unroll
        for (int k = 0; k < GS_MAX_ENSEMBLE_C; ++k) {
            if (k < K) {
                const float *src = a.logits[k] + img;
                float v[EHE_PX];
                for (int c = 0; c < classes; ++c) {
                    ehe_upsample(src, (unsigned)c * plane, t, v);
#pragma unroll
                    for (int i = 0; i < EHE_PX; ++i)
                        mk[k][i] = c == 0 ? v[i] : fmaxf(mk[k][i], v[i]);
                }
                for (int c = 0; c < classes; ++c) {
                    ehe_upsample(src, (unsigned)c * plane, t, v);
#pragma unroll
                    for (int i = 0; i < EHE_PX; ++i) {
                        const float e = expf(v[i] - mk[k][i]);
                        sk[k][i] = c == 0 ? e : sk[k][i] + e;
                    }
                }
            }
        }
        // ---- pass 2: P[c], class-outer, and its running first maximum
        float best[EHE_PX] = {};
        unsigned cls[EHE_ROWS];   // a row's four class indices, one byte each
#pragma unroll
        for (int r = 0; r < EHE_ROWS; ++r)
            cls[r] = 0;
        for (int c = 0; c < classes; ++c) {
            float P[EHE_PX];
#pragma unroll
            for (int k = 0; k < GS_MAX_ENSEMBLE_C; ++k) {
                if (k < K) {
                    float v[EHE_PX];
                    ehe_upsample(a.logits[k] + img, (unsigned)c * plane, t, v);
#pragma unroll
                    for (int i = 0; i < EHE_PX; ++i) {
                        const float pk = (expf(v[i] - mk[k][i]) / sk[k][i]) * a.inv_members;
                        P[i] = k == 0 ? pk : P[i] + pk;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < EHE_PX; ++i) {
                const bool up = c == 0 || P[i] > best[i];
                best[i] = up ? P[i] : best[i];
                const int sh = 8 * (i & 3);
                cls[i >> 2] = up ? (cls[i >> 2] & ~(0xffu << sh)) | ((unsigned)c << sh) : cls[i >> 2];
            }
        }
#pragma unroll
        for (int r = 0; r < EHE_ROWS; ++r) {
            *reinterpret_cast<unsigned *>(a.mask + ((long long)n * H + ya + r) * W + x) = cls[r];   // x and W are multiples of 4
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

inline void launch_ens_head(const EncHeadEnsArgs &a, int n, hipStream_t s)
{
    const dim3 grid((unsigned)(((long long)(a.H3 + 1) * (8 / EHE_ROWS) * 2 * a.W3 + 255) / 256), (unsigned)n);
    switch ((a.classes + 4) / 5) {
    case 1: hipLaunchKernelGGL(enc_head_ens_kernel<1>, grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL(enc_head_ens_kernel<2>, grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL(enc_head_ens_kernel<3>, grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL(enc_head_ens_kernel<4>, grid, dim3(256), 0, s, a); break;
    }
}

}  // namespace gs
