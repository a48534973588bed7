// Boundary distances of matched glomeruli (include/glomseg_boundary_dist.h): for every boundary pixel of a paired instance the
// exact squared distance to the boundary of its partner, in both directions, and per ground-truth instance and direction the
// number of such pixels, the largest d2 and the sum of d2.
//
// gs_instance_boundary_dist keeps four uint16 link tables in the caller's workspace (boundary_dist_plan.h), in four launches:
//   1 bdist_zero_kernel    stats = 0
//   2 bdist_rows_kernel    one wave per (row, side): the row in chunks of 64 pixels left to right, then right to left, four
//                          chunks' tests ahead of their links so that the loads overlap.  A lane
//                          tests its pixel (boundary_links.h's boundary_pixel), the wave's ballot of the tests gives every lane
//                          the nearest set bit at or below / at or above its own, and the nearest column of the chunks already
//                          done is carried in a register: a segmented scan in the wave, no atomics, no LDS.  It writes, per
//                          side, the column of the nearest boundary pixel OF ANY VALID INSTANCE at or left of x and at or right
//                          of x, kLinkNone for none.
//   3 bdist_query_kernel   direction 0: one lane per pixel of LG.  A boundary pixel of a paired g reads its partner id once and
//                          walks the rows y, y-1, y+1, y-2, ... of LP's tables while k*k < best; in a row it hops from x to the
//                          left and to the right along the links, skips boundary pixels of other instances and stops at the
//                          first pixel of the partner or when dx*dx + k*k >= best.  Every lane stores its d2 or -1 into the map;
//                          the lanes of a wave that share g are combined and the group's first lane adds to stats.
//   4 bdist_query_kernel   direction 1: the same from LP into LG's tables.
// With n_gt == 0 or n_pred == 0 nothing can be paired: launch 1 and bdist_fill_kernel (both maps = -1) only.
//
// Why the result is exact: the nearest partner pixel in a row, left of x, is the first partner pixel the left links reach, since
// the links visit every boundary pixel of the row in order of distance; pixels beyond dx*dx + k*k >= best cannot improve best,
// and neither can a row with k*k >= best.  Rows are visited in order of k, so nothing nearer is skipped.
//
// Why the output does not depend on the run: the tables and both maps are pure functions of the inputs, every element written by
// exactly one lane.  stats is written with integer add and max only, which commute: the bytes do not depend on the order in
// which waves arrive, nor on how a wave's lanes happen to be grouped.
//
// Visibility.  Per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores.  Across
// launches visibility comes from the kernel boundary alone: the tables of launch 2 are read plainly in launches 3 and 4 and
// never inside launch 2; the zeroes of launch 1 are in memory before the first atomic of launch 3.  Inside launches 3 and 4 stats
// is touched only through agent-scope 64-bit atomics (add, max), which execute at the memory side: no lane reads stats at all.
//
// Rules: those of wave_block.h, whose grouping loop ends launches 3 and 4.  The loops of this file's own --
//   the row pass      x0 rises (falls) by 256 per round until it leaves [0, width)
//   the row walk      k rises by one per round and stops at k*k >= best, at height, or when both rows y-k and y+k lie outside
//   a hop sequence    the column strictly falls (left) or rises (right) with every hop: a link at c-1 is at most c-1, one at
//                     c+1 at least c+1; it ends at none, at the row's end, at the partner or at dx*dx + k*k >= best: at most
//                     width hops
// A link is a column the row pass itself stored (< width) or kLinkNone, so no link leads out of its row, and an id is used as an
// index only after its range test.
//
// Inconsistent match arrays.  A pair is believed only when both arrays agree and both ids are in range; a partner that owns no
// boundary pixel makes the search walk every link of the map once (bounded by height * width) and end with no d2: -1, no stats.
#include "gs_internal.h"
#include "boundary_dist_plan.h"
#include "wave_block.h"
#include "boundary_links.h"
#include "../../include/glomseg_boundary_dist.h"

#include <climits>

namespace gs {

namespace {

typedef unsigned long long u64;
typedef unsigned short u16;

constexpr int kThreads = kBdistThreads;
static_assert(kThreads == 256, "four waves per workgroup: the row pass's wave index");
constexpr int kBatch = 4, kSpan = 64 * kBatch;     // the row pass tests this many chunks of 64 pixels before it links them

// 1 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void bdist_zero_kernel(u64 *__restrict__ stats, long long words)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < words)
        stats[i] = 0;
}

__global__ __launch_bounds__(kThreads) void bdist_fill_kernel(int *__restrict__ dist_gt, int *__restrict__ dist_pred, long long pixels)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < pixels) {
        if (dist_gt)
            dist_gt[i] = -1;
        if (dist_pred)
            dist_pred[i] = -1;
    }
}

// 2 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void bdist_rows_kernel(const int *__restrict__ lg, int n_gt, const int *__restrict__ lp, int n_pred,
                                                               int H, int W, u16 *__restrict__ left_gt, u16 *__restrict__ right_gt,
                                                               u16 *__restrict__ left_pred, u16 *__restrict__ right_pred)
{
    const int lane = threadIdx.x & 63;
    const int task = (int)blockIdx.x * (kThreads / 64) + (int)(threadIdx.x >> 6);      // < 2 * 32768 + 4
    if (task >= 2 * H)                             // the whole wave
        return;
    const bool pred = task >= H;
    const int y = pred ? task - H : task;
    const int *__restrict__ L = pred ? lp : lg;
    const int n = pred ? n_pred : n_gt;
    u16 *__restrict__ left = (pred ? left_pred : left_gt) + (size_t)y * W;
    u16 *__restrict__ right = (pred ? right_pred : right_gt) + (size_t)y * W;
    int id;
    int carry = kLinkNone;
    for (int x0 = 0; x0 < W; x0 += kSpan) {        // wave-uniform
        u64 m[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {         // the tests of kBatch chunks first: their loads are in flight together
            const int x = x0 + 64 * b + lane;
            m[b] = __ballot((x < W) & boundary_pixel(L, n, H, W, y, x < W ? x : W - 1, id));
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int xb = x0 + 64 * b, x = xb + lane;
            const u64 le = m[b] & (~0ull >> (63 - lane));              // bits 0..lane
            if (x < W)
                left[x] = (u16)(le ? xb + 63 - __clzll((long long)le) : carry);
            if (m[b])
                carry = xb + 63 - __clzll((long long)m[b]);
        }
    }
    carry = kLinkNone;
    for (int x0 = (W - 1) / kSpan * kSpan; x0 >= 0; x0 -= kSpan) {
        u64 m[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int x = x0 + 64 * b + lane;
            m[b] = __ballot((x < W) & boundary_pixel(L, n, H, W, y, x < W ? x : W - 1, id));
        }
#pragma unroll
        for (int b = kBatch - 1; b >= 0; --b) {
            const int xb = x0 + 64 * b, x = xb + lane;
            const u64 ge = m[b] & (~0ull << lane);                     // bits lane..63
            if (x < W)
                right[x] = (u16)(ge ? xb + __ffsll((long long)ge) - 1 : carry);
            if (m[b])
                carry = xb + __ffsll((long long)m[b]) - 1;
        }
    }
}

// 3, 4 ---------------------------------------------------------------------------------------------------------------------
// The squared distance from (x, y) to the nearest pixel of T's tables that carries the label t, or -1.
__device__ inline int nearest_of_partner(const int *__restrict__ T, const u16 *__restrict__ left, const u16 *__restrict__ right, int t, int H,
                                         int W, int y, int x)
{
    int best = INT_MAX;                            // every d2 is at most 2 * 32767^2 < INT_MAX
    for (int k = 0; k < H; ++k) {
        const int kk = k * k;                      // k <= 32767
        if (kk >= best)
            break;
        const bool above = y - k >= 0, below = y + k < H;
        if (!above && !below)
            break;
        for (int s = 0; s < (k ? 2 : 1); ++s) {
            if (s == 0 ? !above : !below)
                continue;
            const size_t row = (size_t)(s == 0 ? y - k : y + k) * W;
            int c = left[row + x];
            while (c != kLinkNone) {              // c falls with every hop
                const int d = (x - c) * (x - c) + kk;
                if (d >= best)
                    break;
                if (T[row + c] == t) {
                    best = d;
                    break;
                }
                if (c == 0)
                    break;
                c = left[row + c - 1];
            }
            c = right[row + x];
            while (c != kLinkNone) {              // c rises with every hop
                const int d = (c - x) * (c - x) + kk;
                if (d >= best)
                    break;
                if (T[row + c] == t) {
                    best = d;
                    break;
                }
                if (c == W - 1)
                    break;
                c = right[row + c + 1];
            }
        }
    }
    return best == INT_MAX ? -1 : best;
}

// S, match_s, n_s: the side the pixels come from; T, match_t, n_t and the tables: the side searched.  dir 0: S is the ground
// truth and stats' row is the pixel's own id; dir 1: S is the prediction and the row is its partner's.
__global__ __launch_bounds__(kThreads) void bdist_query_kernel(const int *__restrict__ S, const int *__restrict__ match_s, int n_s,
                                                                const int *__restrict__ T, const int *__restrict__ match_t, int n_t,
                                                                const u16 *__restrict__ left, const u16 *__restrict__ right, int H, int W, int dir,
                                                                int *__restrict__ dist, u64 *stats)
{
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x, pixels = (long long)H * W;
    int d2 = -1, g = 0;
    if (i < pixels) {
        const int y = (int)(i / W), x = (int)(i - (long long)y * W);
        int a;
        if (boundary_pixel(S, n_s, H, W, y, x, a)) {
            const int t = match_s[a - 1];                              // 1 <= a <= n_s
            if (t >= 1 && t <= n_t && match_t[t - 1] == a) {           // a pair: both arrays agree
                d2 = nearest_of_partner(T, left, right, t, H, W, y, x);
                g = dir == 0 ? a : t;
            }
        }
        if (dist)
            dist[i] = d2;
    }
    // every lane of the wave gets here.  Lanes that share g are retired together; a slide-map wave holds one or two glomeruli.
    for_each_wave_group(d2 >= 0, g, [&](int first, u64 grp, bool mine) {
        const int g0 = __shfl(g, first);
        u64 sum = mine ? (u64)d2 : 0;
        unsigned mx = mine ? (unsigned)d2 : 0;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            sum += __shfl_xor(sum, off);
            const unsigned o = __shfl_xor(mx, off);
            mx = o > mx ? o : mx;
        }
        if (lane == first) {
            u64 *row = stats + ((size_t)(g0 - 1) * 2 + dir) * 3;       // 1 <= g0 <= n_gt
            __hip_atomic_fetch_add(row, (u64)__popcll(grp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (mx)
                __hip_atomic_fetch_max(row + 1, (u64)mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (sum)
                __hip_atomic_fetch_add(row + 2, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    });
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" gs_status gs_boundary_dist_plan(int height, int width, size_t *workspace_bytes)
{
    GS_REQUIRE(workspace_bytes, "gs_boundary_dist_plan: null argument");
    BoundaryDistPlan plan;
    const gs_status st = plan_boundary_dist(height, width, plan);
    *workspace_bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_instance_boundary_dist(const int32_t *labels_gt, const int32_t *labels_pred, const int32_t *match_gt, int n_gt,
                                               const int32_t *match_pred, int n_pred, int height, int width, void *workspace,
                                               size_t workspace_bytes, int32_t *dist_gt, int32_t *dist_pred, unsigned long long *stats,
                                               void *hip_stream)
{
    BoundaryDistPlan plan;
    gs_status st = plan_boundary_dist(height, width, plan);
    if (st != GS_OK)
        return st;
    st = check_instance_counts("gs_instance_boundary_dist", n_gt, n_pred);
    if (st != GS_OK)
        return st;
    GS_REQUIRE(aligned(labels_gt, 4) && aligned(labels_pred, 4),
               "gs_instance_boundary_dist: labels_gt / labels_pred is NULL or not 4-byte aligned");
    GS_REQUIRE(n_gt == 0 || aligned(match_gt, 4), "gs_instance_boundary_dist: match_gt is NULL or not 4-byte aligned");
    GS_REQUIRE(n_pred == 0 || aligned(match_pred, 4), "gs_instance_boundary_dist: match_pred is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 8), "gs_instance_boundary_dist: workspace is NULL or not 8-byte aligned");
    GS_REQUIRE((!dist_gt || aligned(dist_gt, 4)) && (!dist_pred || aligned(dist_pred, 4)),
               "gs_instance_boundary_dist: dist_gt / dist_pred is not 4-byte aligned");
    GS_REQUIRE(n_gt == 0 || aligned(stats, 8), "gs_instance_boundary_dist: stats is NULL or not 8-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_instance_boundary_dist: %d x %d maps need %zu bytes of workspace (got %zu)", height, width,
               plan.bytes, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char *ws = static_cast<char *>(workspace);
    u16 *left_gt = reinterpret_cast<u16 *>(ws + plan.left_gt_off), *right_gt = reinterpret_cast<u16 *>(ws + plan.right_gt_off);
    u16 *left_pred = reinterpret_cast<u16 *>(ws + plan.left_pred_off), *right_pred = reinterpret_cast<u16 *>(ws + plan.right_pred_off);
    const unsigned pixel_blocks = (unsigned)plan.pixel_blocks;

    if (n_gt > 0) {
        const long long words = 6ll * n_gt;
        hipLaunchKernelGGL(bdist_zero_kernel, dim3((unsigned)((words - 1) / kThreads + 1)), dim3(kThreads), 0, s, stats, words);
    }
    if (n_gt == 0 || n_pred == 0) {                // nothing can be paired
        if (dist_gt || dist_pred)
            hipLaunchKernelGGL(bdist_fill_kernel, dim3(pixel_blocks), dim3(kThreads), 0, s, dist_gt, dist_pred, (long long)plan.n_pixels);
        GS_HIP(hipGetLastError());
        return GS_OK;
    }
    hipLaunchKernelGGL(bdist_rows_kernel, dim3((unsigned)plan.row_blocks), dim3(kThreads), 0, s, labels_gt, n_gt, labels_pred, n_pred, height,
                       width, left_gt, right_gt, left_pred, right_pred);
    hipLaunchKernelGGL(bdist_query_kernel, dim3(pixel_blocks), dim3(kThreads), 0, s, labels_gt, match_gt, n_gt, labels_pred, match_pred, n_pred,
                       left_pred, right_pred, height, width, 0, dist_gt, stats);
    hipLaunchKernelGGL(bdist_query_kernel, dim3(pixel_blocks), dim3(kThreads), 0, s, labels_pred, match_pred, n_pred, labels_gt, match_gt, n_gt,
                       left_gt, right_gt, height, width, 1, dist_pred, stats);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
