// WSI-level evaluation against ground truth (eval_wsi_segmentation.py:162-213, the scan_files branch): for every window of
// the reference's window walk, the ground-truth and prediction label maps of that window are composited from their crop
// rasters (np.max of the member boxes, :301-312), scored into a per-window fast_hist (IOUEval.py:19-21) and sampled into the
// two 1/8 class maps (generate_whole_img, :215-241) -- in one launch, without materialising any level-0 map.
//
// One workgroup per 64 x 64 tile of one window.  The workgroup collects the member boxes of its window that touch the tile
// (in LDS); a tile no box touches returns at once -- most of a slide -- and its pixels are added to cell (0,0) by the
// per-window fill-in pass (window area minus the pixels counted).  Counting is run-length per thread, then an LDS
// histogram, then one global integer atomic per non-zero cell: bit-reproducible.
#include <climits>

#include "gs_internal.h"

namespace gs {

namespace {

constexpr int kTile = 64;         // tile edge, level-0 pixels
constexpr int kThreads = 256;     // 4 rows of 64 columns per pass, 16 passes per tile
constexpr int kLdsBoxes = 128;    // candidate boxes per set held in LDS; beyond that the tile reads its window's list in place

enum : int { kErrLabel = 1, kErrBox = 2, kErrList = 4 };

struct EvalSet {
    const unsigned char *rasters;
    long long raster_bytes;
    const gs_eval_box *boxes;
    int n_boxes;
    const int *win_ptr;
    const int *win_idx;
    int n_idx;
    unsigned char *small_map;
};

struct EvalArgs {
    int W, H, ws, classes, nwx, nwy, tiles_x, tiles_y;
    EvalSet set[2];                 // 0 = ground truth, 1 = prediction
    const int *sx, *sy;
    int map_h, map_w;
    unsigned long long *hist;       // [nwx*nwy][classes*classes]
    int *err;                       // [0] flags, [1] largest label >= classes, [2] / [3] lowest bad box index of set 0 / 1
};

struct Rect {
    int x0, y0, x1, y1;
    long long off;
};

// window (xi, yi) of the walk (:180-195); false when the reference skips it or it is empty
__device__ inline bool window_rect(const EvalArgs &a, int xi, int yi, int &xmin, int &ymin, int &xmax, int &ymax)
{
    xmin = xi * a.ws;
    xmax = xi == a.W / a.ws ? a.W : (xi + 1) * a.ws;
    ymin = yi * a.ws;
    ymax = yi == a.H / a.ws ? a.H : (yi + 1) * a.ws;
    if (xmax > a.W || ymax > a.W)   // :186 and :194 (slide_width for slide_height: the reference's typo, kept)
        return false;
    return xmax > xmin && ymax > ymin;
}

// the box record of a member, checked: its raster must be exactly its placement rectangle and lie inside the set's buffer
__device__ inline bool load_box(const EvalArgs &a, int s, int j, Rect &r)
{
    const EvalSet &S = a.set[s];
    const int b = S.win_idx[j];
    if (b < 0 || b >= S.n_boxes) {
        atomicOr(&a.err[0], kErrList);
        return false;
    }
    const gs_eval_box e = S.boxes[b];
    const long long w = (long long)e.x1 - e.x0, h = (long long)e.y1 - e.y0;
    if (w <= 0 || h <= 0 || e.raster_w != w || e.raster_h != h || e.offset < 0 || e.offset + w * h > S.raster_bytes) {
        atomicOr(&a.err[0], kErrBox);
        atomicMin(&a.err[2 + s], b);
        return false;
    }
    r = Rect{e.x0, e.y0, e.x1, e.y1, e.offset};
    return true;
}

// label of level-0 pixel (x, y) in set s: 0, or the max over the candidate boxes that contain it (:311-312)
__device__ inline int label_at(const EvalArgs &a, int s, const Rect *lds, int n, bool in_place, int p0, int p1, int x, int y)
{
    const unsigned char *R = a.set[s].rasters;
    int v = 0;
    if (!in_place) {
        for (int i = 0; i < n; ++i) {
            const Rect r = lds[i];
            if (x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1) {
                const int t = R[r.off + (long long)(y - r.y0) * (r.x1 - r.x0) + (x - r.x0)];
                v = t > v ? t : v;
            }
        }
    } else {
        for (int j = p0; j < p1; ++j) {
            Rect r;
            if (!load_box(a, s, j, r))
                continue;
            if (x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1) {
                const int t = R[r.off + (long long)(y - r.y0) * (r.x1 - r.x0) + (x - r.x0)];
                v = t > v ? t : v;
            }
        }
    }
    return v;
}

__global__ void __launch_bounds__(kThreads) wsi_eval_tile_kernel(const EvalArgs a)
{
    extern __shared__ unsigned int lh[];                // classes*classes counters
    __shared__ Rect cand[2][kLdsBoxes];
    __shared__ int n_cand[2];
    __shared__ int span[2][2];

    const int w = blockIdx.y;
    const int xi = w % a.nwx, yi = w / a.nwx;
    int xmin, ymin, xmax, ymax;
    if (!window_rect(a, xi, yi, xmin, ymin, xmax, ymax))
        return;
    const int tx0 = xmin + (int)(blockIdx.x % a.tiles_x) * kTile, ty0 = ymin + (int)(blockIdx.x / a.tiles_x) * kTile;
    if (tx0 >= xmax || ty0 >= ymax)
        return;
    const int tx1 = min(tx0 + kTile, xmax), ty1 = min(ty0 + kTile, ymax);
    const int tid = threadIdx.x;

    if (tid < 2) {
        n_cand[tid] = 0;
        const EvalSet &S = a.set[tid];
        int p0 = S.win_ptr[w], p1 = S.win_ptr[w + 1];
        if (p0 < 0 || p1 < p0 || p1 > S.n_idx) {
            atomicOr(&a.err[0], kErrList);
            p0 = p1 = 0;
        }
        span[tid][0] = p0;
        span[tid][1] = p1;
    }
    __syncthreads();
    // member boxes of the window that touch the tile (every member is checked, as the reference pastes every member)
    for (int s = 0; s < 2; ++s) {
        for (int j = span[s][0] + tid; j < span[s][1]; j += kThreads) {
            Rect r;
            if (!load_box(a, s, j, r))
                continue;
            if (r.x0 < tx1 && r.x1 > tx0 && r.y0 < ty1 && r.y1 > ty0) {
                const int k = atomicAdd(&n_cand[s], 1);
                if (k < kLdsBoxes)
                    cand[s][k] = r;
            }
        }
    }
    __syncthreads();
    const int ng = n_cand[0], np = n_cand[1];
    if (ng == 0 && np == 0)
        return;                                          // box-free tile: all (0,0), added by the fill-in pass
    const bool gin = ng > kLdsBoxes, pin = np > kLdsBoxes;
    const int cells = a.classes * a.classes;
    for (int i = tid; i < cells; i += kThreads)
        lh[i] = 0;
    __syncthreads();

    const int x = tx0 + (tid & (kTile - 1));
    int cur = -1;
    unsigned int run = 0;
    if (x < tx1) {
        for (int y = ty0 + (tid >> 6); y < ty1; y += kThreads / kTile) {
            const int g = ng ? label_at(a, 0, cand[0], ng, gin, span[0][0], span[0][1], x, y) : 0;
            const int p = np ? label_at(a, 1, cand[1], np, pin, span[1][0], span[1][1], x, y) : 0;
            if (g >= a.classes || p >= a.classes) {      // :315
                atomicOr(&a.err[0], kErrLabel);
                atomicMax(&a.err[1], g > p ? g : p);
                continue;
            }
            const int cell = g * a.classes + p;
            if (cell != cur) {
                if (run)
                    atomicAdd(&lh[cur], run);
                cur = cell;
                run = 0;
            }
            ++run;
        }
    }
    if (run)
        atomicAdd(&lh[cur], run);

    // 1/8 maps: the cells whose level-0 sample point lies in this tile (each such cell lies in exactly one tile)
    const int X0 = max(tx0 / 8 - 1, 0), X1 = min(tx1 / 8 + 2, a.map_w);
    const int Y0 = max(ty0 / 8 - 1, 0), Y1 = min(ty1 / 8 + 2, a.map_h);
    const int nx = X1 - X0, ny = Y1 - Y0;
    if (nx > 0 && ny > 0 && (a.set[0].small_map || a.set[1].small_map)) {
        for (int i = tid; i < nx * ny; i += kThreads) {
            const int X = X0 + i % nx, Y = Y0 + i / nx;
            const int px = a.sx[X], py = a.sy[Y];
            if (px < tx0 || px >= tx1 || py < ty0 || py >= ty1)
                continue;
            if (a.set[0].small_map && ng)
                a.set[0].small_map[(long long)Y * a.map_w + X] =
                    (unsigned char)label_at(a, 0, cand[0], ng, gin, span[0][0], span[0][1], px, py);
            if (a.set[1].small_map && np)
                a.set[1].small_map[(long long)Y * a.map_w + X] =
                    (unsigned char)label_at(a, 1, cand[1], np, pin, span[1][0], span[1][1], px, py);
        }
    }
    __syncthreads();
    unsigned long long *hw = a.hist + (long long)w * cells;
    for (int i = tid; i < cells; i += kThreads)
        if (lh[i])
            atomicAdd(&hw[i], (unsigned long long)lh[i]);
}

// cell (0,0) of every walked window gets the pixels no tile counted: window area minus the window's counted pixels
__global__ void __launch_bounds__(64) wsi_eval_fill_kernel(const EvalArgs a)
{
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= a.nwx * a.nwy)
        return;
    int xmin, ymin, xmax, ymax;
    if (!window_rect(a, w % a.nwx, w / a.nwx, xmin, ymin, xmax, ymax))
        return;
    const int cells = a.classes * a.classes;
    unsigned long long *hw = a.hist + (long long)w * cells;
    unsigned long long counted = 0;
    for (int i = 0; i < cells; ++i)
        counted += hw[i];
    hw[0] += (unsigned long long)(xmax - xmin) * (unsigned long long)(ymax - ymin) - counted;
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" {

gs_status gs_wsi_eval_windows(int slide_w, int slide_h, int window, int classes, const gs_eval_set *gt, const gs_eval_set *pred,
                              const int *sx_lut, const int *sy_lut, int map_h, int map_w, unsigned long long *hist_win, int *err_word,
                              void *hip_stream)
{
    GS_REQUIRE(gt && pred && hist_win && err_word, "gs_wsi_eval_windows: null pointer");
    GS_REQUIRE(slide_w > 0 && slide_h > 0 && window > 0, "gs_wsi_eval_windows: bad slide %d x %d / window %d", slide_w, slide_h, window);
    GS_REQUIRE(classes > 0 && classes <= 64, "gs_wsi_eval_windows: classes %d outside 1..64", classes);
    GS_REQUIRE(map_h >= 0 && map_w >= 0, "gs_wsi_eval_windows: bad map size");
    const bool maps = gt->small_map || pred->small_map;
    GS_REQUIRE(!maps || (sx_lut && sy_lut), "gs_wsi_eval_windows: 1/8 maps need both sample tables");
    const gs_eval_set *sets[2] = {gt, pred};
    EvalArgs a{};
    a.W = slide_w;
    a.H = slide_h;
    a.ws = window;
    a.classes = classes;
    a.nwx = slide_w / window + 1;
    a.nwy = slide_h / window + 1;
    a.tiles_x = (window + kTile - 1) / kTile;
    a.tiles_y = a.tiles_x;
    GS_REQUIRE((long long)a.nwx * a.nwy < 65536 && (long long)a.tiles_x * a.tiles_y < (1LL << 24),
               "gs_wsi_eval_windows: %d x %d windows exceed the launch grid", a.nwx, a.nwy);
    for (int s = 0; s < 2; ++s) {
        const gs_eval_set &S = *sets[s];
        GS_REQUIRE(S.win_ptr && S.n_boxes >= 0 && S.n_idx >= 0 && S.raster_bytes >= 0, "gs_wsi_eval_windows: bad %s set",
                   s ? "prediction" : "ground-truth");
        GS_REQUIRE(S.n_idx == 0 || (S.win_idx && S.boxes && (S.rasters || S.raster_bytes == 0)),
                   "gs_wsi_eval_windows: %s set has members but no boxes / rasters", s ? "prediction" : "ground-truth");
        a.set[s] = EvalSet{S.rasters, S.raster_bytes, S.boxes, S.n_boxes, S.win_ptr, S.win_idx, S.n_idx, S.small_map};
    }
    a.sx = sx_lut;
    a.sy = sy_lut;
    a.map_h = maps ? map_h : 0;
    a.map_w = maps ? map_w : 0;
    a.hist = hist_win;
    a.err = err_word;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int nw = a.nwx * a.nwy;
    const size_t cells = (size_t)classes * classes;
    GS_HIP(hipMemsetAsync(hist_win, 0, (size_t)nw * cells * sizeof(unsigned long long), st));
    GS_HIP(hipMemsetAsync(err_word, 0, 2 * sizeof(int), st));
    GS_HIP(hipMemsetAsync(err_word + 2, 0x7f, 2 * sizeof(int), st));      // 0x7f7f7f7f: no bad box yet
    for (int s = 0; s < 2; ++s)
        if (sets[s]->small_map && map_h > 0 && map_w > 0)
            GS_HIP(hipMemsetAsync(sets[s]->small_map, 0, (size_t)map_h * map_w, st));
    hipLaunchKernelGGL(wsi_eval_tile_kernel, dim3((unsigned)(a.tiles_x * a.tiles_y), (unsigned)nw), dim3(kThreads),
                       cells * sizeof(unsigned int), st, a);
    GS_HIP(hipGetLastError());
    hipLaunchKernelGGL(wsi_eval_fill_kernel, dim3((unsigned)((nw + 63) / 64)), dim3(64), 0, st, a);
    GS_HIP(hipGetLastError());
    // the range and record checks are reported like any argument error: this entry waits for its launch
    int err[4];
    GS_HIP(hipMemcpyAsync(err, err_word, sizeof(err), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    if (err[0] & kErrBox) {
        const bool g = err[2] != 0x7f7f7f7f;
        set_error("gs_wsi_eval_windows: %s box %d: its raster is not the size of its placement rectangle or lies outside the "
                  "set's raster buffer", g ? "ground-truth" : "prediction", g ? err[2] : err[3]);
        return GS_ERR_INVALID;
    }
    if (err[0] & kErrList) {
        set_error("gs_wsi_eval_windows: a window membership list is malformed (row pointers or box indices out of range)");
        return GS_ERR_INVALID;
    }
    if (err[0] & kErrLabel) {
        set_error("gs_wsi_eval_windows: label %d >= classes %d in a window", err[1], classes);
        return GS_ERR_INVALID;
    }
    return GS_OK;
}

}  // extern "C"
