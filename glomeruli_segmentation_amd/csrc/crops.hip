// gs_espnet_segment_crops*: the per-patch loop of module/espnet/test/VisualizeResults_iou.py:100-156 for the crops a slide
// really produces -- every merged box at its own size (module/faster-rcnn/make_seg_data.py:357-361) -- a whole batch per
// launch.  The stages either side of the forward are descriptor-table kernels: the table (up to 64 crops) travels as a
// kernel argument, so a call allocates nothing, copies nothing and is stream-ordered like any other launch.
//
//   crops_prep_kernel    :107-116  (x - mean) / std at crop resolution -> cv2.resize INTER_LINEAR -> / 255 -> fp32 NCHW
//   (forward)            :123,128  espnet_forward: the mask comes out of the decoder tail (ESPNet-C: of enc_head_kernel; an ensemble
//                                  of ESPNet-C members: K trunks, then one enc_head_ens_kernel), no logits
//   crops_back_kernel    :129,151-155  cv2.resize INTER_NEAREST back to every crop's size + per-class counts of THAT map
//   crops_paste_kernel   eval_wsi_segmentation.py:311-312  np.max into the 1/ds slide map
//   crops_score_kernel   :195-203 (IOUEval.py:19-21), :196  a labelled batch: every crop's label nearest-resized to the network
//                                  size on the fly, its confusion matrix against the network-resolution mask and the set of
//                                  label values (np.unique), one launch per batch (gs_espnet_score_crops, glomseg_scoring.h)
//   crops_overlay_kernel :139-146, :218-222  palette colouring + addWeighted of the prediction; launched a second time over the
//                                  packed labels for the ground-truth overlay
//
// The first four are bandwidth-bound byte / fp32 streams (bound: HBM); per 1024x512 network tile and ~0.6 Mpx crop they move
// 6.3 MB (fp32 tensor out) + ~1.8 MB (crop in), 0.5 MB + 0.6 MB, and a few KB.  crops_score_kernel reads 0.5 MB of mask and the
// gathered label bytes per crop and is bound by its counters, not by HBM.
#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/glomseg_scoring.h"
#include "crop_plan.h"
#include "crop_sample.h"
#include "gs_internal.h"
#include "host_copy.h"
#include "host_pipe.h"

namespace gs {

constexpr int MAXC = GS_MAX_CROPS_PER_CALL;
struct CropTable {
    gs_crop_desc d[MAXC];
};

struct PrepArgs {
    const unsigned char *in;   // packed crops
    float *out;                // [n][3][net_h][net_w]
    int net_h, net_w;
    float mean[3], std[3];
    unsigned long long *hist_zero;   // optional: counters crops_back_kernel adds into, zeroed here
    int hist_count;
};

// one thread = four consecutive output columns of one row, all three channels: 16-byte stores
__global__ void __launch_bounds__(256) crops_prep_kernel(const CropTable t, const PrepArgs a)
{
    __shared__ float lut[3][256];
    crop_norm_table(lut, a.mean, a.std);
    const int i = blockIdx.y;
    if (a.hist_zero && blockIdx.x == 0 && i == 0)
        for (int k = threadIdx.x; k < a.hist_count; k += 256)
            a.hist_zero[k] = 0ull;
    const int w4 = a.net_w / 4;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.net_h * w4)
        return;
    const int oy = idx / w4, ox = (idx - oy * w4) * 4;
    const int h = t.d[i].h, w = t.d[i].w;
    const unsigned char *src = a.in + t.d[i].in_off;
    const double sx = cv_inv_scale(a.net_w, w), sy = cv_inv_scale(a.net_h, h);
    int y0, y1, x0[4], x1[4];
    float wy, wx[4];
    linear_tap(oy, sy, h, y0, y1, wy);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        linear_tap(ox + k, sx, w, x0[k], x1[k], wx[k]);
    float *dst = a.out + (((long long)i * 3) * a.net_h + oy) * a.net_w + ox;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float4 v;
        v.x = crop_sample(src, w, c, x0[0], x1[0], y0, y1, wx[0], wy, lut[c]);
        v.y = crop_sample(src, w, c, x0[1], x1[1], y0, y1, wx[1], wy, lut[c]);
        v.z = crop_sample(src, w, c, x0[2], x1[2], y0, y1, wx[2], wy, lut[c]);
        v.w = crop_sample(src, w, c, x0[3], x1[3], y0, y1, wx[3], wy, lut[c]);
        *reinterpret_cast<float4 *>(dst + (long long)c * a.net_h * a.net_w) = v;
    }
}

// Nearest resize of every network-resolution mask back to its crop's size, four consecutive bytes of the flat crop map per
// thread (one 32-bit store), and the per-class counts of the crop-size map: packed per-lane counters (12 bits per class, at
// most 4 added per iteration and the grid is sized for <= 512 iterations), a butterfly add over the wave, one LDS atomic per
// class per wave, one global atomic per class per workgroup.  NW = 64-bit counter words per lane, five classes each (1 for the
// five-class networks, up to 4 for GS_MAX_CLASSES = 20); hist is [n][classes].
template <int NW>
__global__ void __launch_bounds__(256)
crops_back_kernel(const CropTable t, const unsigned char *net, int net_h, int net_w, unsigned char *out, unsigned long long *hist, int classes)
{
    __shared__ unsigned lh[5 * NW];
    const int i = blockIdx.y;
    if (threadIdx.x < 5 * NW)
        lh[threadIdx.x] = 0;
    __syncthreads();
    const int h = t.d[i].h, w = t.d[i].w;
    const long long hw = (long long)h * w;
    const unsigned char *src = net + (long long)i * net_h * net_w;
    unsigned char *dst = out ? out + t.d[i].out_off : nullptr;
    const double ifx = cv_inv_scale(w, net_w), ify = cv_inv_scale(h, net_h);
    unsigned long long counts[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q)
        counts[q] = 0;
    for (long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; base < hw; base += (long long)gridDim.x * 1024) {
        int oy = (int)(base / w), ox = (int)(base - (long long)oy * w);
        unsigned packed = 0;
        int sy = nearest_src(oy, ify, net_h);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (base + k < hw) {
                const unsigned v = src[(long long)sy * net_w + nearest_src(ox, ifx, net_w)];
                packed |= v << (8 * k);
                const unsigned vc = v < (unsigned)classes ? v : 0;   // (a value no class map holds counts as background)
                if (NW == 1) {
                    counts[0] += 1ull << (12 * vc);
                } else {
#pragma unroll
                    for (int q = 0; q < NW; ++q)
                        if (vc / 5 == (unsigned)q)
                            counts[q] += 1ull << (12 * (vc % 5));
                }
            }
            if (++ox == w) {   // the four bytes may run over a row end
                ox = 0;
                ++oy;
                sy = nearest_src(oy, ify, net_h);
            }
        }
        if (dst) {
            if (base + 4 <= hw)
                *reinterpret_cast<unsigned *>(dst + base) = packed;   // out_off and base are multiples of 4
            else
                for (int k = 0; base + k < hw; ++k)
                    dst[base + k] = (unsigned char)(packed >> (8 * k));
        }
    }
    if (hist) {
#pragma unroll
        for (int k = 0; k < 5 * NW; ++k) {
            int c = (int)((counts[k / 5] >> (12 * (k % 5))) & 0xfffull);
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1)
                c += __shfl_xor(c, sh, 64);
            if ((threadIdx.x & 63) == 0 && c)
                atomicAdd(&lh[k], (unsigned)c);
        }
        __syncthreads();
        if ((int)threadIdx.x < classes && lh[threadIdx.x])
            atomicAdd(&hist[(long long)i * classes + threadIdx.x], (unsigned long long)lh[threadIdx.x]);
    }
}

// Palette colouring + cv2.addWeighted of every crop of the batch (VisualizeResults_iou.py:139-146): four pixels per thread -- one
// dword of the crop-size class map, three dwords of BGR in, three out.  The two products and their sum are rounded separately
// (no fused multiply-add), so the bytes are those of numpy's float32 arithmetic.  `fp contract(off)` over plain operators is
// what keeps them apart: __fmul_rn / __fadd_rn are inline functions whose own * and + are compiled contractible, and written
// with them nine of the twelve sums of a thread came out as v_fmac_f32 (tests/test_crop_stage.py: the 0.3 / 0.7 and 1.3 / 0.9
// weights tell the difference, 0.4 / 0.6 does not).
struct OverlayArgs {
    const unsigned char *crops;   // packed BGR crops (gs_crop_desc::in_off)
    const unsigned char *maps;    // packed crop-size class maps (out_off)
    unsigned char *out;           // packed overlays, at in_off
    float wa, wb;
    int n_colours;
    int clamp;                    // a class beyond the table: 0 = black, 1 = the table's last row (the ground-truth overlay)
    unsigned char pal[GS_MAX_PALETTE * 3];   // RGB rows
};

__global__ void __launch_bounds__(256) crops_overlay_kernel(const CropTable t, const OverlayArgs a)
{
#pragma clang fp contract(off)
    const int i = blockIdx.y;
    const long long hw = (long long)t.d[i].h * t.d[i].w;
    const unsigned char *src = a.crops + t.d[i].in_off, *cls = a.maps + t.d[i].out_off;
    unsigned char *dst = a.out + t.d[i].in_off;
    for (long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; base < hw; base += (long long)gridDim.x * 1024) {
        const int np = hw - base < 4 ? (int)(hw - base) : 4;
        unsigned cw = 0, pw[3] = {0, 0, 0}, ow[3] = {0, 0, 0};   // bytes little-endian in dwords
        if (np == 4) {   // (in_off / out_off are multiples of 256 and base of 4: aligned dwords)
            cw = *reinterpret_cast<const unsigned *>(cls + base);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                pw[k] = reinterpret_cast<const unsigned *>(src + base * 3)[k];
        } else {
            for (int k = 0; k < np; ++k)
                cw |= (unsigned)cls[base + k] << (8 * k);
            for (int k = 0; k < np * 3; ++k)
                pw[k >> 2] |= (unsigned)src[base * 3 + k] << (8 * (k & 3));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int c = (int)((cw >> (8 * k)) & 0xffu);
            if (a.clamp && c >= a.n_colours)
                c = a.n_colours - 1;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int bi = k * 3 + ch;
                const float pix = (float)((pw[bi >> 2] >> (8 * (bi & 3))) & 0xffu);
                // palette rows are RGB, the image is BGR (classMap_numpy_color[...] = [b, g, r], :143)
                const float col = c < a.n_colours ? (float)a.pal[c * 3 + (2 - ch)] : 0.0f;
                const float v = pix * a.wa + col * a.wb;   // (three roundings: contraction is off in this function)
                ow[bi >> 2] |= (unsigned)fminf(fmaxf(rintf(v), 0.0f), 255.0f) << (8 * (bi & 3));   // saturate_cast<uchar>(cvRound)
            }
        }
        if (np == 4) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                reinterpret_cast<unsigned *>(dst + base * 3)[k] = ow[k];
        } else {
            for (int k = 0; k < np * 3; ++k)
                dst[base * 3 + k] = (unsigned char)(ow[k >> 2] >> (8 * (k & 3)));
        }
    }
}

// Scoring of a labelled batch at network resolution (VisualizeResults_iou.py:195-203): for every network pixel of crop i the
// label byte g at the pixel's INTER_NEAREST source in the crop-size label (the reference resizes the label to the network size,
// :195; a label already at that size is the identity case of the same rule) and the mask byte p; conf_i[g][p] += 1 for
// g < classes (IOUEval.py:19-21; a mask byte >= classes, which no forward writes, is dropped too) and bit g of seen_i set for
// every g (np.unique of the resized label, :196).  One thread = four consecutive mask bytes of one row (one dword; net_w is a
// multiple of 8), about eight such dwords per thread.  Nearly every pixel is background on both sides, so no counter is bumped
// per pixel in memory of any kind:
//   REG (classes <= 5)  crops_back_kernel's packed counters, one 64-bit word of five 12-bit fields per ground-truth row, five
//                       words per lane (at most 4 added to a field per iteration and the grid keeps a lane under 33
//                       iterations: <= 132 of 4095), a butterfly add over the wave per field, one LDS add per wave;
//   general (6 .. 20)   80 words of registers do not fit: bin (0,0) is counted in a register per lane, every other bin is
//                       aggregated over the wave first -- the lanes that hold the leader's bin are counted with a ballot and
//                       the leader adds the count to the workgroup's LDS histogram: one LDS add per DISTINCT bin of a wave
//                       instruction (one, for a crop whose glomerulus fills the tile).
// Label values below 64 are collected in a register per lane and OR-reduced over the wave; the others (a 255 "ignore" byte) go
// to the LDS set only when the lane's value changes.  One global add per non-zero bin and one OR per non-zero word per workgroup;
// conf and seen are zeroed on the stream by the launcher.
struct ScoreArgs {
    const unsigned char *net;      // [n][net_h][net_w]
    const unsigned char *labels;   // packed crop-size labels (gs_crop_desc::out_off)
    unsigned long long *conf;      // [n][classes][classes], rows = ground truth
    unsigned long long *seen;      // [n][4]: 256-bit set, or null
    int net_h, net_w, classes;
};

// CFG_SCORE_FORM -- 0: the register form up to five classes, the ballot form above (the product); 1 / 2: the ballot form / the
// wave-private LDS histograms (one LDS add per pixel into the wave's own copy of the matrix, the copies summed at the end) for
// EVERY class count: the A/B of tools/crop_scoring_rate.py (DESIGN.md section 4 has the figures)
#ifndef CFG_SCORE_FORM
#define CFG_SCORE_FORM 0
#endif
enum { SCORE_REG = 0, SCORE_BALLOT = 1, SCORE_WAVE_HIST = 2 };

template <int FORM>
__global__ void __launch_bounds__(256) crops_score_kernel(const CropTable t, const ScoreArgs a)
{
    constexpr bool REG = FORM == SCORE_REG;
    constexpr int NBINS = GS_MAX_CLASSES * GS_MAX_CLASSES;
    constexpr int NB = REG ? 25 : FORM == SCORE_WAVE_HIST ? 4 * NBINS : NBINS;
    __shared__ unsigned lh[NB];
    __shared__ unsigned ls[8];
    const int i = blockIdx.y, lane = threadIdx.x & 63, cl = a.classes;
    for (int k = threadIdx.x; k < NB; k += 256)
        lh[k] = 0;
    if (threadIdx.x < 8)
        ls[threadIdx.x] = 0;
    __syncthreads();
    const int h = t.d[i].h, w = t.d[i].w;
    const unsigned char *msk = a.net + (long long)i * a.net_h * a.net_w;
    const unsigned char *lab = a.labels + t.d[i].out_off;
    const double sfy = cv_inv_scale(a.net_h, h), sfx = cv_inv_scale(a.net_w, w);
    const int w4 = a.net_w / 4, quads = a.net_h * w4;
    unsigned long long rows[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    unsigned long long lo = 0ull;   // label values 0 .. 63 this lane has met
    int n00 = 0, last = -1;
    // (the loop bound is the wave's, not the lane's: the ballots below see whole waves)
    for (int q0 = blockIdx.x * 256 + (threadIdx.x - lane); q0 < quads; q0 += gridDim.x * 256) {
        const int q = q0 + lane;
        const bool valid = q < quads;
        const int oy = valid ? q / w4 : 0, ox = valid ? (q - oy * w4) * 4 : 0;
        const unsigned mw = valid ? *reinterpret_cast<const unsigned *>(msk + (long long)oy * a.net_w + ox) : 0u;
        const unsigned char *lrow = lab + (long long)nearest_src(oy, sfy, h) * w;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int g = lrow[nearest_src(ox + k, sfx, w)], p = (int)((mw >> (8 * k)) & 0xffu);
            if (valid) {
                if (g < 64) {
                    lo |= 1ull << g;
                } else if (g != last) {
                    atomicOr(&ls[g >> 5], 1u << (g & 31));
                    last = g;
                }
            }
            const bool counted = valid && g < cl && p < cl;
            if (REG) {
                const unsigned long long inc = counted ? 1ull << (12 * p) : 0ull;
#pragma unroll
                for (int r = 0; r < 5; ++r)
                    rows[r] += g == r ? inc : 0ull;
            } else if (FORM == SCORE_WAVE_HIST) {
                if (counted)
                    atomicAdd(&lh[(threadIdx.x >> 6) * NBINS + g * cl + p], 1u);
            } else {
                const int bin = g * cl + p;
                n00 += counted && bin == 0 ? 1 : 0;
                const bool active = counted && bin != 0;
                unsigned long long todo = __ballot(active);
                while (todo) {
                    const int leader = __ffsll((long long)todo) - 1;
                    const int lb = __shfl(bin, leader, 64);
                    const unsigned long long m = __ballot(active && bin == lb);
                    if (lane == leader)
                        atomicAdd(&lh[lb], (unsigned)__popcll(m));
                    todo &= ~m;
                }
            }
        }
    }
    if (REG) {
#pragma unroll
        for (int k = 0; k < 25; ++k) {
            int c = (int)((rows[k / 5] >> (12 * (k % 5))) & 0xfffull);
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1)
                c += __shfl_xor(c, sh, 64);
            if (lane == 0 && c)
                atomicAdd(&lh[k], (unsigned)c);
        }
    } else if (FORM == SCORE_BALLOT) {
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1)
            n00 += __shfl_xor(n00, sh, 64);
        if (lane == 0 && n00)
            atomicAdd(&lh[0], (unsigned)n00);
    }
    unsigned lo0 = (unsigned)lo, lo1 = (unsigned)(lo >> 32);
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        lo0 |= __shfl_xor(lo0, sh, 64);
        lo1 |= __shfl_xor(lo1, sh, 64);
    }
    if (lane == 0) {
        if (lo0) atomicOr(&ls[0], lo0);
        if (lo1) atomicOr(&ls[1], lo1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < cl * cl; b += 256) {
        const unsigned v = REG ? lh[(b / cl) * 5 + b % cl]
                           : FORM == SCORE_WAVE_HIST ? lh[b] + lh[NBINS + b] + lh[2 * NBINS + b] + lh[3 * NBINS + b] : lh[b];
        if (v)
            atomicAdd(&a.conf[(long long)i * cl * cl + b], (unsigned long long)v);
    }
    if (a.seen && threadIdx.x < 4) {
        const unsigned long long v = (unsigned long long)ls[2 * threadIdx.x] | ((unsigned long long)ls[2 * threadIdx.x + 1] << 32);
        if (v)
            atomicOr(&a.seen[(long long)i * 4 + threadIdx.x], v);
    }
}

// per-byte maximum into a map that other crops of the same launch (or of the other compute stream) may be writing
__device__ __forceinline__ void byte_max(unsigned char *p, unsigned v)
{
    if (v == 0)
        return;   // the map starts at zero: a background pixel never changes it
    unsigned *wp = reinterpret_cast<unsigned *>(reinterpret_cast<unsigned long long>(p) & ~3ull);
    const int sh = (int)(reinterpret_cast<unsigned long long>(p) & 3ull) * 8;
    unsigned old = __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (((old >> sh) & 0xffu) < v) {
        const unsigned nv = (old & ~(0xffu << sh)) | (v << sh);
        const unsigned prev = atomicCAS(wp, old, nv);
        if (prev == old)
            break;
        old = prev;
    }
}

// Max-composite of every crop's class map into the 1/ds slide map.  Map cell (X, Y) shows level-0 pixel (ds*X, ds*Y) --
// or (sx[X], sy[Y]) under the reference's window walk (gs_wsi_paste_max_lut) -- i.e. crop pixel (px - x1, py - y1), whose
// class is the network-resolution mask at that pixel's INTER_NEAREST source: the crop-size map need not exist.
__global__ void __launch_bounds__(256)
crops_paste_kernel(const CropTable t, const unsigned char *net, int net_h, int net_w, const gs_paste_target p)
{
    const int i = blockIdx.y;
    const int h = t.d[i].h, w = t.d[i].w, x1 = t.d[i].x1, y1 = t.d[i].y1;
    const unsigned char *src = net + (long long)i * net_h * net_w;
    const int ds = p.ds;
    // candidate cells: within one cell of the crop's footprint on the regular grid (the tables are monotone with steps >= ds)
    const int X0 = x1 / ds - 1, Y0 = y1 / ds - 1;
    const int nx = (x1 + w) / ds + 2 - X0, ny = (y1 + h) / ds + 2 - Y0;
    const double ifx = cv_inv_scale(w, net_w), ify = cv_inv_scale(h, net_h);
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < nx * ny; idx += gridDim.x * 256) {
        const int X = X0 + idx % nx, Y = Y0 + idx / nx;
        if (X < 0 || Y < 0 || X >= p.map_w || Y >= p.map_h)
            continue;
        const int px = p.sx_lut ? p.sx_lut[X] : X * ds, py = p.sy_lut ? p.sy_lut[Y] : Y * ds;
        if (px < 0 || py < 0)
            continue;
        const int cx = px - x1, cy = py - y1;
        if (cx < 0 || cy < 0 || cx >= w || cy >= h)
            continue;
        const unsigned v = src[(long long)nearest_src(cy, ify, net_h) * net_w + nearest_src(cx, ifx, net_w)];
        byte_max(p.slide_map + (long long)Y * p.map_w + X, v);
    }
}

// ---------------------------------------------------------------------------------------------
// staging state, owned by the (first) model handle
struct CropPipe {
    int device = 0;
    struct LaneScratch {
        float *f32 = nullptr;           // the network input [n,3,net_h,net_w]
        size_t f32_bytes = 0;
        unsigned char *net = nullptr;   // network-resolution masks when the caller keeps none
        size_t net_bytes = 0;
    } lane[4];
    // host pipeline (host_pipe.h): four slots
    struct Slot : PipeSlot {
        Staging<unsigned char> in, out, net;   // packed crops, packed crop-size maps, network-resolution maps
        Staging<unsigned char> ov;             // overlays (allocated on first use, sized like the packed input)
        Staging<unsigned long long> hist;
        Staging<unsigned char> lab, gov;       // a scored call: packed labels (laid out like `out`), ground-truth overlays (like `ov`)
        Staging<unsigned long long> score;     // its results: conf [count][classes][classes], then seen [count][4]
        bool out_direct = false, ov_direct = false;
        std::vector<gs_crop_desc> descs;
        size_t in_bytes = 0, out_bytes = 0;    // packed sizes of the batch (fill_crop_descs)
        void free_staging() { in.free(), out.free(), net.free(), ov.free(), hist.free(), lab.free(), gov.free(), score.free(); }
    };
    HostPipe<Slot, 4> host;
};

void crop_pipe_destroy(CropPipe *p)
{
    if (!p)
        return;
    p->host.destroy();
    for (auto &l : p->lane) {
        if (l.f32) hipFree(l.f32);
        if (l.net) hipFree(l.net);
    }
    delete p;
}

static CropPipe *pipe_of(gs_espnet *h)
{
    CropPipe *&p = espnet_crop_pipe(h);
    if (!p) {
        p = new (std::nothrow) CropPipe();
        if (p)
            p->device = espnet_device(h);
    }
    return p;
}

static gs_status check_common(gs_espnet *const *models, int n_models, const float *means, const float *stds, int net_h, int net_w)
{
    GS_REQUIRE(models && n_models > 0 && means && stds, "segment_crops: null argument");
    GS_REQUIRE(net_h >= 8 && net_w >= 8 && net_h % 8 == 0 && net_w % 8 == 0,
               "network size must be a positive multiple of 8 in both dimensions (got %dx%d)", net_h, net_w);
    for (int k = 0; k < n_models; ++k)
        GS_REQUIRE(models[k], "model %d is null", k);
    if (n_models > 1) {
        // all full networks, or all ESPNet-C handles (at most GS_MAX_ENSEMBLE_C, run_ensemble: one head over their logits).
        // A mixed list is refused HERE, in the crop entries' own words; ensemble_kind below (shared with
        // gs_espnet_ensemble_forward) would refuse it too, with that entry's text, and is never reached with one: what it
        // adds for the crop entries is the class counts, the member limit and the repeated handle.
        bool any_full = false, enc_only = false;
        for (int k = 0; k < n_models; ++k)
            any_full = any_full || espnet_is_full_net(models[k]);
        for (int k = 0; k < n_models; ++k)
            GS_REQUIRE(!any_full || espnet_is_full_net(models[k]),
                       "ensemble member %d is an ESPNet-C handle in a list with full networks: mixed ensembles need full ESPNet members", k);
        const gs_status st = ensemble_kind(models, n_models, &enc_only);   // class counts, the member limit, repeated handles
        if (st != GS_OK) return st;
    }
    for (int k = 0; k < n_models; ++k)
        for (int i = 0; i < 3; ++i)
            GS_REQUIRE(stds[3 * k + i] != 0.0f, "model %d: std[%d] is zero", k, i);
    return GS_OK;
}

// crops_score_kernel over a complete table: zeroes conf / seen on the stream, then one launch
static gs_status launch_score(const CropTable &tab, int n, const unsigned char *net_masks, const unsigned char *labels, int net_h,
                              int net_w, int classes, unsigned long long *conf, unsigned long long *seen, hipStream_t s)
{
    const size_t conf_words = (size_t)n * classes * classes;
    const bool joined = seen == conf + conf_words;   // the host pipeline's layout: one fill
    GS_HIP(hipMemsetAsync(conf, 0, (conf_words + (joined ? (size_t)n * 4 : 0)) * sizeof(unsigned long long), s));
    if (seen && !joined)
        GS_HIP(hipMemsetAsync(seen, 0, (size_t)n * 4 * sizeof(unsigned long long), s));
    ScoreArgs a{};
    a.net = net_masks;
    a.labels = labels;
    a.conf = conf;
    a.seen = seen;
    a.net_h = net_h;
    a.net_w = net_w;
    a.classes = classes;
    // about eight dwords of mask per thread; at the grid limit a lane makes 2^29 / (65535 * 256) < 33 iterations
    const long long quads = (long long)net_h * net_w / 4;
    const long long gx = std::min(std::max((quads + 8 * 256 - 1) / (8 * 256), 1ll), 65535ll);
    const dim3 grid((unsigned)gx, (unsigned)n);
    if (CFG_SCORE_FORM == 0 && classes <= 5)
        hipLaunchKernelGGL(crops_score_kernel<SCORE_REG>, grid, dim3(256), 0, s, tab, a);
    else if (CFG_SCORE_FORM == 2)
        hipLaunchKernelGGL(crops_score_kernel<SCORE_WAVE_HIST>, grid, dim3(256), 0, s, tab, a);
    else
        hipLaunchKernelGGL(crops_score_kernel<SCORE_BALLOT>, grid, dim3(256), 0, s, tab, a);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// the device side of a gs_crop_scoring block for one batch
struct BatchScoring {
    const unsigned char *labels;   // packed at out_off
    unsigned long long *conf, *seen;
    unsigned char *gt_overlay;     // packed at in_off, or null
    int gt_clamp;
};

// An overlay request of after_masks: crops_overlay_kernel over the crop-size maps (packed_out) into `out`
struct BatchOverlay {
    const unsigned char *crops;         // packed BGR crops at in_off
    const unsigned char *palette_rgb;   // host, n_colours rows
    int n_colours;
    float wa, wb;
    unsigned char *out;                 // packed at in_off, or null (only a ground-truth overlay is wanted)
    int clamp;                          // of the launch into `out`; the ground-truth launch takes BatchScoring::gt_clamp
};

// Everything that follows the network-resolution masks of one batch, on stream s: the resize back with the counts, the scoring,
// the overlays (prediction and ground truth) and the paste, each with its grid.  The table is complete.  hist is added into: the
// caller has zeroed it on the stream (crops_prep_kernel in run_batch, a fill in gs_crops_from_masks).
static gs_status after_masks(const CropTable &tab, int n, const unsigned char *net_masks, int net_h, int net_w, int classes,
                             unsigned char *packed_out, unsigned long long *hist, const gs_paste_target *paste,
                             const BatchOverlay *overlay, const BatchScoring *score, hipStream_t s)
{
    long long max_hw = 1, max_cells = 1;
    for (int i = 0; i < n; ++i) {
        max_hw = std::max(max_hw, (long long)tab.d[i].h * tab.d[i].w);
        if (paste)
            max_cells = std::max(max_cells, (long long)(tab.d[i].w / paste->ds + 3) * (tab.d[i].h / paste->ds + 3));
    }
    if (packed_out || hist) {
        long long gx = (max_hw + 8 * 1024 - 1) / (8 * 1024);   // about eight iterations per workgroup, never more than 512
        gx = std::max(gx, (max_hw + 512 * 1024 - 1) / (512 * 1024));
        gx = std::min(std::max(gx, 1ll), 65535ll);
        const dim3 grid((unsigned)gx, (unsigned)n);
        switch ((classes + 4) / 5) {
        case 1: hipLaunchKernelGGL(crops_back_kernel<1>, grid, dim3(256), 0, s, tab, net_masks, net_h, net_w, packed_out, hist, classes); break;
        case 2: hipLaunchKernelGGL(crops_back_kernel<2>, grid, dim3(256), 0, s, tab, net_masks, net_h, net_w, packed_out, hist, classes); break;
        case 3: hipLaunchKernelGGL(crops_back_kernel<3>, grid, dim3(256), 0, s, tab, net_masks, net_h, net_w, packed_out, hist, classes); break;
        default: hipLaunchKernelGGL(crops_back_kernel<4>, grid, dim3(256), 0, s, tab, net_masks, net_h, net_w, packed_out, hist, classes); break;
        }
        GS_HIP(hipGetLastError());
    }
    if (score) {   // reads the network-resolution masks only
        const gs_status st = launch_score(tab, n, net_masks, score->labels, net_h, net_w, classes, score->conf, score->seen, s);
        if (st != GS_OK) return st;
    }
    const bool gt_overlay = score && score->gt_overlay && overlay;
    if ((overlay && overlay->out) || gt_overlay) {   // needs the crop-size maps: the caller passes packed_out with it
        OverlayArgs oa{};
        oa.crops = overlay->crops;
        oa.wa = overlay->wa;
        oa.wb = overlay->wb;
        oa.n_colours = overlay->n_colours;
        std::memcpy(oa.pal, overlay->palette_rgb, (size_t)overlay->n_colours * 3);
        const long long gx = std::min(std::max((max_hw + 8 * 1024 - 1) / (8 * 1024), 1ll), 65535ll);
        if (overlay->out) {
            oa.maps = packed_out;
            oa.out = overlay->out;
            oa.clamp = overlay->clamp ? 1 : 0;
            hipLaunchKernelGGL(crops_overlay_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, s, tab, oa);
            GS_HIP(hipGetLastError());
        }
        if (gt_overlay) {   // the same kernel over the packed labels (VisualizeResults_iou.py:218-222)
            oa.maps = score->labels;
            oa.out = score->gt_overlay;
            oa.clamp = score->gt_clamp ? 1 : 0;
            hipLaunchKernelGGL(crops_overlay_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, s, tab, oa);
            GS_HIP(hipGetLastError());
        }
    }
    if (paste) {
        const unsigned gx = (unsigned)std::min<long long>((max_cells + 255) / 256, 4096);
        hipLaunchKernelGGL(crops_paste_kernel, dim3(gx, (unsigned)n), dim3(256), 0, s, tab, net_masks, net_h, net_w, *paste);
        GS_HIP(hipGetLastError());
    }
    return GS_OK;
}

// One batch, everything on stream s: the table is complete (offsets within packed_in / packed_out).
static gs_status run_batch(gs_espnet *const *models, int n_models, int lane, const unsigned char *packed_in, const gs_crop_desc *descs,
                           int n, const float *means, const float *stds, int net_h, int net_w, unsigned char *net_masks,
                           unsigned char *packed_out, unsigned long long *hist, const gs_paste_target *paste, hipStream_t s,
                           const gs_crop_overlay *overlay = nullptr, unsigned char *overlay_out = nullptr,
                           const BatchScoring *score = nullptr)
{
    CropPipe *pipe = pipe_of(models[0]);
    GS_REQUIRE(pipe, "out of host memory");
    GS_REQUIRE(n >= 1 && n <= MAXC, "internal: a batch of %d crops does not fit the %d-entry descriptor table", n, MAXC);
    GS_REQUIRE(lane >= 0 && lane < 4, "lane %d out of range", lane);
    for (int k = 0; k < n_models; ++k)
        GS_REQUIRE(lane < espnet_lanes(models[k]), "model %d has no lane %d (gs_espnet_set_lanes)", k, lane);
    CropPipe::LaneScratch &ls = pipe->lane[lane];
    const size_t npx = (size_t)net_h * net_w;
    const int classes = espnet_classes(models[0]);
    gs_status st = grow(ls.f32, ls.f32_bytes, (size_t)n * 3 * npx * sizeof(float), "crop tensor");
    if (st != GS_OK) return st;
    if (!net_masks) {
        st = grow(ls.net, ls.net_bytes, (size_t)n * npx, "network-resolution mask");
        if (st != GS_OK) return st;
        net_masks = ls.net;
    }
    CropTable tab;
    std::memset(&tab, 0, sizeof tab);
    std::copy(descs, descs + n, tab.d);
    const dim3 prep_grid((unsigned)((net_h * (net_w / 4) + 255) / 256), (unsigned)n);
    // member k resamples the crops with its own mean / std into the lane's tensor; the first launch also zeroes the counts
    auto prepare = [&](int k) -> gs_status {
        PrepArgs a{};
        a.in = packed_in;
        a.out = ls.f32;
        a.net_h = net_h;
        a.net_w = net_w;
        for (int c = 0; c < 3; ++c) {
            a.mean[c] = means[3 * k + c];
            a.std[c] = stds[3 * k + c];
        }
        if (hist && k == 0) {
            a.hist_zero = hist;
            a.hist_count = n * classes;
        }
        hipLaunchKernelGGL(crops_prep_kernel, prep_grid, dim3(256), 0, s, tab, a);
        GS_HIP(hipGetLastError());
        return GS_OK;
    };
    ForwardReq r;   // the network-resolution masks only: the counts are those of the crop-size maps (crops_back_kernel)
    r.in = ls.f32, r.n = n, r.H = net_h, r.W = net_w, r.mask = net_masks, r.s = s;
    if (n_models > 1) {
        st = run_ensemble(models, n_models, lane, r, nullptr, nullptr, prepare);
    } else {
        // NOT the runner's one-member ensemble (role SOLE): a single crop model takes the argmax of its logits (role NONE, as
        // gs_espnet_forward does), a one-member ensemble takes the argmax of its softmax, and the two can differ where fp32
        // rounds two close logits to equal probabilities.
        st = prepare(0);
        if (st == GS_OK) st = espnet_forward(models[0], lane, r);
    }
    if (st != GS_OK) return st;
    BatchOverlay bo{};
    if (overlay) {
        bo.crops = packed_in;
        bo.palette_rgb = overlay->palette_rgb;
        bo.n_colours = overlay->n_colours;
        bo.wa = overlay->wa;
        bo.wb = overlay->wb;
        bo.out = overlay_out;
    }
    return after_masks(tab, n, net_masks, net_h, net_w, classes, packed_out, hist, paste, overlay ? &bo : nullptr, score, s);
}

static gs_status check_descs(const gs_crop_desc *descs, int n, bool need_out)
{
    GS_REQUIRE(descs && n > 0 && n <= MAXC, "1 to %d crops per call (got %d)", MAXC, n);
    for (int i = 0; i < n; ++i) {
        GS_REQUIRE(descs[i].h > 0 && descs[i].w > 0 && (long long)descs[i].h * descs[i].w < (1ll << 31), "crop %d has a bad size %dx%d", i,
                   descs[i].h, descs[i].w);
        GS_REQUIRE(descs[i].in_off >= 0 && (!need_out || (descs[i].out_off >= 0 && descs[i].out_off % 4 == 0)),
                   "crop %d: offsets must be non-negative and out_off a multiple of 4", i);
    }
    return GS_OK;
}

static gs_status check_paste(const gs_paste_target *p)
{
    if (!p)
        return GS_OK;
    GS_REQUIRE(p->slide_map && p->map_h > 0 && p->map_w > 0 && p->ds > 0, "paste target: null map or bad size");
    GS_REQUIRE((p->sx_lut == nullptr) == (p->sy_lut == nullptr), "paste target: give both tables or neither");
    // crops of one launch (or of the other stream) that overlap meet through a 32-bit compare-and-swap on the aligned word that
    // holds the byte: the map must start on a 4-byte boundary and its allocation must cover whole words
    GS_REQUIRE((reinterpret_cast<uintptr_t>(p->slide_map) & 3u) == 0,
               "paste target: slide_map must be 4-byte aligned (and its allocation padded to a multiple of 4 bytes)");
    return GS_OK;
}

}  // namespace gs

using namespace gs;

extern "C" {

gs_status gs_espnet_ensemble_segment_crops(gs_espnet *const *models, int n_models, const uint8_t *packed_in, const gs_crop_desc *descs,
                                           int n, const float *means, const float *stds, int net_h, int net_w, uint8_t *net_masks,
                                           uint8_t *packed_out, unsigned long long *hist, const gs_paste_target *paste, void *hip_stream)
{
    gs_status st = check_common(models, n_models, means, stds, net_h, net_w);
    if (st != GS_OK) return st;
    GS_REQUIRE(packed_in, "segment_crops: null input");
    GS_REQUIRE(net_masks || packed_out || hist || paste, "nothing to compute: every output is NULL");
    st = check_descs(descs, n, packed_out != nullptr);
    if (st != GS_OK) return st;
    st = check_paste(paste);
    if (st != GS_OK) return st;
    return run_batch(models, n_models, 0, packed_in, descs, n, means, stds, net_h, net_w, net_masks, packed_out, hist, paste,
                     static_cast<hipStream_t>(hip_stream));
}

gs_status gs_espnet_segment_crops(gs_espnet *h, int lane, const uint8_t *packed_in, const gs_crop_desc *descs, int n, const float mean[3],
                                  const float std[3], int net_h, int net_w, uint8_t *net_masks, uint8_t *packed_out,
                                  unsigned long long *hist, const gs_paste_target *paste, void *hip_stream)
{
    gs_espnet *models[1] = {h};
    gs_status st = check_common(models, h ? 1 : 0, mean, std, net_h, net_w);
    if (st != GS_OK) return st;
    GS_REQUIRE(packed_in, "segment_crops: null input");
    GS_REQUIRE(net_masks || packed_out || hist || paste, "nothing to compute: every output is NULL");
    st = check_descs(descs, n, packed_out != nullptr);
    if (st != GS_OK) return st;
    st = check_paste(paste);
    if (st != GS_OK) return st;
    return run_batch(models, 1, lane, packed_in, descs, n, mean, std, net_h, net_w, net_masks, packed_out, hist, paste,
                     static_cast<hipStream_t>(hip_stream));
}

gs_status gs_espnet_score_crops(const uint8_t *net_masks, const uint8_t *packed_labels, const gs_crop_desc *descs, int n, int net_h,
                                int net_w, int classes, unsigned long long *conf, unsigned long long *seen, void *hip_stream)
{
    GS_REQUIRE(n >= 1 && n <= MAXC, "score_crops: 1 to %d crops per call (got %d)", MAXC, n);
    GS_REQUIRE(classes >= 2 && classes <= GS_MAX_CLASSES, "score_crops: 2 to %d classes (got %d)", GS_MAX_CLASSES, classes);
    GS_REQUIRE(packed_labels, "score_crops: null label buffer");
    GS_REQUIRE(conf, "score_crops: null conf");
    GS_REQUIRE(net_masks && (reinterpret_cast<uintptr_t>(net_masks) & 3u) == 0, "score_crops: net_masks is null or not 4-byte aligned");
    GS_REQUIRE(net_h >= 8 && net_w >= 8 && net_h % 8 == 0 && net_w % 8 == 0 && (long long)net_h * net_w < (1ll << 29),
               "network size must be a positive multiple of 8 in both dimensions (got %dx%d)", net_h, net_w);
    const gs_status st = check_descs(descs, n, true);
    if (st != GS_OK) return st;
    CropTable tab;
    std::memset(&tab, 0, sizeof tab);
    std::copy(descs, descs + n, tab.d);
    return launch_score(tab, n, net_masks, packed_labels, net_h, net_w, classes, conf, seen, static_cast<hipStream_t>(hip_stream));
}

gs_status gs_crops_from_masks(const uint8_t *net_masks, const gs_crop_desc *descs, int n, int net_h, int net_w, int classes,
                              uint8_t *packed_out, unsigned long long *hist, const gs_paste_target *paste, const uint8_t *overlay_crops,
                              const uint8_t *palette_rgb, int n_colours, float wa, float wb, int clamp, uint8_t *overlay_out,
                              void *hip_stream)
{
    GS_REQUIRE(classes >= 2 && classes <= GS_MAX_CLASSES, "crops_from_masks: 2 to %d classes (got %d)", GS_MAX_CLASSES, classes);
    GS_REQUIRE(net_masks && (reinterpret_cast<uintptr_t>(net_masks) & 3u) == 0, "crops_from_masks: net_masks is null or not 4-byte aligned");
    GS_REQUIRE(net_h >= 8 && net_w >= 8 && net_h % 8 == 0 && net_w % 8 == 0 && (long long)net_h * net_w < (1ll << 29),
               "network size must be a positive multiple of 8 in both dimensions (got %dx%d)", net_h, net_w);
    GS_REQUIRE(packed_out || hist || paste, "nothing to compute: every output is NULL");
    GS_REQUIRE((reinterpret_cast<uintptr_t>(packed_out) & 3u) == 0, "crops_from_masks: packed_out is not 4-byte aligned");
    gs_status st = check_descs(descs, n, packed_out != nullptr);
    if (st != GS_OK) return st;
    st = check_paste(paste);
    if (st != GS_OK) return st;
    BatchOverlay bo{};
    if (overlay_out) {
        GS_REQUIRE(packed_out, "crops_from_masks: an overlay needs packed_out (it colours the crop-size maps)");
        GS_REQUIRE(overlay_crops && palette_rgb && n_colours >= 1 && n_colours <= GS_MAX_PALETTE,
                   "overlay: null crops / palette or a table of %d colours (1 .. %d)", n_colours, GS_MAX_PALETTE);
        GS_REQUIRE(((reinterpret_cast<uintptr_t>(overlay_crops) | reinterpret_cast<uintptr_t>(overlay_out)) & 3u) == 0,
                   "overlay: the packed crops and the output must be 4-byte aligned");
        for (int i = 0; i < n; ++i)
            GS_REQUIRE(descs[i].in_off % 4 == 0, "overlay: crop %d: in_off must be a multiple of 4", i);
        bo.crops = overlay_crops;
        bo.palette_rgb = palette_rgb;
        bo.n_colours = n_colours;
        bo.wa = wa;
        bo.wb = wb;
        bo.out = overlay_out;
        bo.clamp = clamp;
    }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (hist)   // (in the crop entries the resampling kernel zeroes the counts)
        GS_HIP(hipMemsetAsync(hist, 0, (size_t)n * classes * sizeof(unsigned long long), s));
    CropTable tab;
    std::memset(&tab, 0, sizeof tab);
    std::copy(descs, descs + n, tab.d);
    return after_masks(tab, n, net_masks, net_h, net_w, classes, packed_out, hist, paste, overlay_out ? &bo : nullptr, nullptr, s);
}

gs_status gs_plan_crop_batches(const int *heights, const int *widths, int n_crops, int batch, int *starts, int cap, int *n_batches)
{
    GS_REQUIRE(heights && widths && n_batches, "gs_plan_crop_batches: null argument");
    GS_REQUIRE(n_crops > 0 && batch > 0, "gs_plan_crop_batches: n_crops and batch must be positive");
    for (int i = 0; i < n_crops; ++i)
        GS_REQUIRE(heights[i] > 0 && widths[i] > 0 && (long long)heights[i] * widths[i] < (1ll << 29), "crop %d has a bad size %dx%d", i,
                   heights[i], widths[i]);
    const CropBatchPlan plan = plan_crop_batches(heights, widths, n_crops, batch, MAXC);
    *n_batches = (int)plan.starts.size() - 1;
    if (!starts)
        return GS_OK;
    GS_REQUIRE(cap >= (int)plan.starts.size(), "gs_plan_crop_batches: %d entries needed, room for %d", (int)plan.starts.size(), cap);
    std::copy(plan.starts.begin(), plan.starts.end(), starts);
    return GS_OK;
}

int gs_host_block_is_pinned(const void *p, size_t bytes) { return p && host_block_is_pinned(p, bytes) ? 1 : 0; }

gs_status gs_espnet_segment_crops_host(gs_espnet *const *models, int n_models, const uint8_t *const *crops, const int *heights,
                                       const int *widths, int n_crops, const float *means, const float *stds, int net_h, int net_w,
                                       int batch, uint8_t *const *masks, uint8_t *net_masks, unsigned long long *hist,
                                       const gs_paste_target *paste, const int *x1, const int *y1, const gs_crop_overlay *overlay)
{
    return gs_espnet_segment_crops_host_scored(models, n_models, crops, heights, widths, n_crops, means, stds, net_h, net_w, batch, masks,
                                               net_masks, hist, paste, x1, y1, overlay, nullptr);
}

gs_status gs_espnet_segment_crops_host_scored(gs_espnet *const *models, int n_models, const uint8_t *const *crops, const int *heights,
                                              const int *widths, int n_crops, const float *means, const float *stds, int net_h,
                                              int net_w, int batch, uint8_t *const *masks, uint8_t *net_masks,
                                              unsigned long long *hist, const gs_paste_target *paste, const int *x1, const int *y1,
                                              const gs_crop_overlay *overlay, const gs_crop_scoring *scoring)
{
    if (scoring) {   // (its own refusals first: they need no handle)
        GS_REQUIRE(scoring->labels, "scoring: null label list");
        GS_REQUIRE(scoring->conf, "scoring: null conf");
        for (int i = 0; i < n_crops; ++i)
            GS_REQUIRE(scoring->labels[i] && (!scoring->gt_overlay_bgr || scoring->gt_overlay_bgr[i]),
                       "scoring: crop %d has a null label or no ground-truth overlay buffer", i);
        GS_REQUIRE(!scoring->gt_overlay_bgr || overlay, "scoring: a ground-truth overlay needs the overlay argument's palette and weights");
    }
    gs_status st = check_common(models, n_models, means, stds, net_h, net_w);
    if (st != GS_OK) return st;
    GS_REQUIRE(crops && heights && widths && n_crops > 0, "segment_crops_host: null crop list");
    GS_REQUIRE(batch > 0, "batch must be positive");
    GS_REQUIRE(masks || net_masks || hist || paste || overlay || scoring, "nothing to compute: every output is NULL");
    GS_REQUIRE(!paste || (x1 && y1), "a paste target needs the crops' level-0 origins");
    if (overlay) {
        GS_REQUIRE(overlay->palette_rgb && overlay->out_bgr && overlay->n_colours >= 1 && overlay->n_colours <= GS_MAX_PALETTE,
                   "overlay: null palette / outputs or a table of %d colours (1 .. %d)", overlay->n_colours, GS_MAX_PALETTE);
        for (int i = 0; i < n_crops; ++i)
            GS_REQUIRE(overlay->out_bgr[i], "overlay: crop %d has no output buffer", i);
    }
    st = check_paste(paste);
    if (st != GS_OK) return st;
    for (int i = 0; i < n_crops; ++i) {
        GS_REQUIRE(crops[i] && (!masks || masks[i]), "crop %d: null pointer", i);
        GS_REQUIRE(heights[i] > 0 && widths[i] > 0 && (long long)heights[i] * widths[i] < (1ll << 29), "crop %d has a bad size %dx%d", i,
                   heights[i], widths[i]);
    }
    CropPipe *pp = pipe_of(models[0]);
    GS_REQUIRE(pp, "out of host memory");
    CropPipe &p = *pp;
    int nl = 2;   // batches alternate between two lanes when every member has them
    for (int k = 0; k < n_models; ++k)
        if (espnet_lanes(models[k]) < 2) nl = 1;
    const size_t npx = (size_t)net_h * net_w;
    const size_t ncl = (size_t)espnet_classes(models[0]);   // hist is [n_crops][classes]
    const size_t ncc = ncl * ncl;                           // conf is [n_crops][classes][classes]
    uint8_t *const *gt_ov = scoring ? scoring->gt_overlay_bgr : nullptr;
    // which crops go into which batch, and the staging a batch needs (csrc/crop_plan.h: host-only, sanitised on its own)
    const CropBatchPlan plan = plan_crop_batches(heights, widths, n_crops, batch, MAXC);
    const std::vector<int> &starts = plan.starts;
    const size_t need_in = plan.need_in, need_out = plan.need_out;
    batch = plan.max_count;
    GS_REQUIRE(batch >= 1 && batch <= MAXC, "internal: planned a batch of %d crops", batch);
    using Slot = CropPipe::Slot;
    HipLatch fail;
    if (!p.host.ensure(2, true, fail, [&](Slot &s) {
            s.in.grow(need_in, fail);
            s.out.grow(need_out, fail);
            s.net.grow(npx * batch, fail);
            s.hist.grow(sizeof(unsigned long long) * GS_MAX_CLASSES * batch, fail);
            if (overlay) s.ov.grow(s.in.bytes, fail);
            if (scoring) {
                s.lab.grow(s.out.bytes, fail);
                s.score.grow(sizeof(unsigned long long) * (GS_MAX_CLASSES * GS_MAX_CLASSES + 4) * batch, fail);
                if (gt_ov) s.gov.grow(s.in.bytes, fail);
            }
        }))
        return fail.rc;
    const bool net_pinned = net_masks && host_is_pinned(net_masks), hist_pinned = hist && host_is_pinned(hist);
    // One DMA for a batch of page-locked destinations laid out like the packed device buffer (every one at its 256-byte-aligned
    // offset behind the batch's first: what engine.segment_crops_host allocates) -- 32 separate DMA commands per batch sat in
    // the compute stream between two forwards -- and only when the whole range is ONE page-locked allocation: separately
    // pinned buffers that happen to be neighbours in virtual memory are written one by one.  off / bytes: crop j's place.
    auto download_direct = [&](uint8_t *const *dst, const unsigned char *dev, int cnt, hipStream_t compute, auto off, auto bytes) {
        bool packed = true;
        for (int j = 0; j < cnt; ++j)
            packed = packed && dst[j] == dst[0] + off(j);
        const size_t b = off(cnt - 1) + bytes(cnt - 1);
        packed = packed && host_block_is_pinned(dst[0], b);
        if (packed) {
            fail(hipMemcpy2DAsync(dst[0], b, dev, b, b, 1, hipMemcpyDeviceToHost, compute), "D2H copy");
            return;
        }
        for (int j = 0; j < cnt && fail.ok(); ++j)
            fail(hipMemcpy2DAsync(dst[j], bytes(j), dev + off(j), bytes(j), bytes(j), 1, hipMemcpyDeviceToHost, compute), "D2H copy");
    };
    const gs_status rc = p.host.run(
        (int)starts.size() - 1, nl == 1, fail,
        [&](int bi, Slot &s, hipStream_t h2d) {
            const int first = s.first = starts[bi], cnt = s.count = starts[bi + 1] - first;
            s.descs.assign(cnt, gs_crop_desc{});
            fill_crop_descs(heights, widths, x1, y1, first, cnt, s.descs.data(), &s.in_bytes, &s.out_bytes);
            bool in_direct = true;
            s.out_direct = masks != nullptr;
            s.ov_direct = overlay != nullptr;
            for (int j = 0; j < cnt; ++j) {
                in_direct = in_direct && host_is_pinned(crops[first + j]);
                if (masks)
                    s.out_direct = s.out_direct && host_is_pinned(masks[first + j]);
                if (overlay)
                    s.ov_direct = s.ov_direct && host_is_pinned(overlay->out_bgr[first + j]);
            }
            // uploads: page-locked crops are DMA'd in place, pageable ones are packed into the slot's pinned buffer by a few
            // threads (one core copies ~10 GB/s) and leave as one copy
            if (in_direct) {
                for (int j = 0; j < cnt && fail.ok(); ++j)
                    fail(hipMemcpyAsync(s.in.d + s.descs[j].in_off, crops[first + j], (size_t)s.descs[j].h * s.descs[j].w * 3,
                                        hipMemcpyHostToDevice, h2d), "H2D copy");
            } else {
                parallel_jobs(cnt, bi == 0 ? 8 : 4, [&](int j) {   // (the first batch's staging is exposed: more threads)
                    std::memcpy(s.in.h + s.descs[j].in_off, crops[first + j], (size_t)s.descs[j].h * s.descs[j].w * 3);
                });
                fail(hipMemcpyAsync(s.in.d, s.in.h, s.in_bytes, hipMemcpyHostToDevice, h2d), "H2D copy");
            }
            if (scoring) {   // the labels ride with the crops: packed like the crop-size maps, one copy
                parallel_jobs(cnt, 4, [&](int j) {
                    std::memcpy(s.lab.h + s.descs[j].out_off, scoring->labels[first + j], (size_t)s.descs[j].h * s.descs[j].w);
                });
                fail(hipMemcpyAsync(s.lab.d, s.lab.h, s.out_bytes, hipMemcpyHostToDevice, h2d), "H2D copy");
            }
        },
        [&](int bi, Slot &s, hipStream_t compute) {
            BatchScoring bs{};
            if (scoring) {
                bs.labels = s.lab.d;
                bs.conf = s.score.d;
                bs.seen = s.score.d + (size_t)s.count * ncc;
                bs.gt_overlay = gt_ov ? s.gov.d : nullptr;
                bs.gt_clamp = scoring->gt_clamp;
            }
            return run_batch(models, n_models, bi % nl, s.in.d, s.descs.data(), s.count, means, stds, net_h, net_w, s.net.d,
                             (masks || overlay) ? s.out.d : nullptr, hist ? s.hist.d : nullptr, paste, compute, overlay,
                             overlay ? s.ov.d : nullptr, scoring ? &bs : nullptr);
        },
        [&](int, Slot &s, hipStream_t compute) {
            const int first = s.first, cnt = s.count;
            auto map_off = [&](int j) { return (size_t)s.descs[j].out_off; };
            auto map_bytes = [&](int j) { return (size_t)s.descs[j].h * s.descs[j].w; };
            auto bgr_off = [&](int j) { return (size_t)s.descs[j].in_off; };
            auto bgr_bytes = [&](int j) { return (size_t)s.descs[j].h * s.descs[j].w * 3; };
            const size_t oi = s.in_bytes, oo = s.out_bytes;
            if (masks) {
                if (s.out_direct)
                    download_direct(masks + first, s.out.d, cnt, compute, map_off, map_bytes);
                else
                    fail(hipMemcpy2DAsync(s.out.h, oo, s.out.d, oo, oo, 1, hipMemcpyDeviceToHost, compute), "D2H copy");
            }
            if (overlay) {
                if (s.ov_direct)
                    download_direct(overlay->out_bgr + first, s.ov.d, cnt, compute, bgr_off, bgr_bytes);
                else
                    fail(hipMemcpy2DAsync(s.ov.h, oi, s.ov.d, oi, oi, 1, hipMemcpyDeviceToHost, compute), "D2H copy");
            }
            if (net_masks)
                fail(hipMemcpy2DAsync(net_pinned ? net_masks + (size_t)first * npx : s.net.h, npx, s.net.d, npx, npx, cnt,
                                      hipMemcpyDeviceToHost, compute), "D2H copy");
            if (gt_ov)
                fail(hipMemcpy2DAsync(s.gov.h, oi, s.gov.d, oi, oi, 1, hipMemcpyDeviceToHost, compute), "D2H copy");
            if (scoring) {
                const size_t b = sizeof(unsigned long long) * (ncc + 4) * cnt;
                fail(hipMemcpy2DAsync(s.score.h, b, s.score.d, b, b, 1, hipMemcpyDeviceToHost, compute), "D2H copy");
            }
            if (hist) {
                const size_t b = sizeof(unsigned long long) * ncl * cnt;
                fail(hipMemcpy2DAsync(hist_pinned ? hist + (size_t)first * ncl : s.hist.h, b, s.hist.d, b, b, 1, hipMemcpyDeviceToHost,
                                      compute), "D2H copy");
            }
        },
        [&](Slot &s) {
            if (masks && !s.out_direct)
                parallel_jobs(s.count, 4, [&](int j) {
                    std::memcpy(masks[s.first + j], s.out.h + s.descs[j].out_off, (size_t)s.descs[j].h * s.descs[j].w);
                });
            if (overlay && !s.ov_direct)
                parallel_jobs(s.count, 4, [&](int j) {
                    std::memcpy(overlay->out_bgr[s.first + j], s.ov.h + s.descs[j].in_off, (size_t)s.descs[j].h * s.descs[j].w * 3);
                });
            if (net_masks && !net_pinned)
                parallel_memcpy(net_masks + (size_t)s.first * npx, s.net.h, npx * s.count);
            if (hist && !hist_pinned)
                std::memcpy(hist + (size_t)s.first * ncl, s.hist.h, sizeof(unsigned long long) * ncl * s.count);
            if (gt_ov)
                parallel_jobs(s.count, 4, [&](int j) {
                    std::memcpy(gt_ov[s.first + j], s.gov.h + s.descs[j].in_off, (size_t)s.descs[j].h * s.descs[j].w * 3);
                });
            if (scoring) {
                std::memcpy(scoring->conf + (size_t)s.first * ncc, s.score.h, sizeof(unsigned long long) * ncc * s.count);
                if (scoring->seen)
                    std::memcpy(scoring->seen + (size_t)s.first * 4, s.score.h + (size_t)s.count * ncc,
                                sizeof(unsigned long long) * 4 * s.count);
            }
        });
    return rc != GS_OK ? rc : gs_device_fault_check();
}

}  // extern "C"
