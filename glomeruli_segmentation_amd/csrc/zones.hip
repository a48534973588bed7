// Influence zones and neighbour gaps of a slide map (csrc/zones_abi.h, which has the definitions): for every pixel the nearest
// instance, exactly, and for every boundary pixel of an instance the nearest pixel of any other instance.  Workspaces: zones_plan.h.
//
// gs_instance_zones, four launches.  g(x, y) is the vertical distance from (x, y) to the nearest instance pixel of column x, 0 on an
// instance pixel and kZoneNone where the column holds none within R = floor(sqrt(max_d2)) rows; clab(x, y) is that pixel's label,
// the lower of the two where the one above and the one below are equally far.  The outside of the map holds no site.
//   1 zone_count_kernel   a workgroup per band of kZoneBand rows and 256 columns, a lane per column: the band's first and last
//                         instance pixel of the column, as rows from the band's first row down (top) and from its last row up
//                         (bot), with their labels.
//   2 zone_carry_kernel   a lane per column walks the bands down and then up: down[b] = rows from band b's first row up to the
//                         nearest instance pixel above the band, up[b] = rows from its last row down to the nearest one below, with
//                         their labels.  The carry across bands is this launch of its own: no workgroup waits for another.
//   3 zone_apply_kernel   the grid of launch 1: the lane walks its kZoneBand rows down from down[b], keeps distance and label in
//                         registers, walks back up from up[b] and stores the nearer of the two, the lower label at a tie.
//   4 zone_row_kernel     a workgroup per row stages the row of g in LDS (maps wider than kZoneLdsCols read it from global memory:
//                         the same kernel, the other template argument) and learns from the staging whether the row holds a finite
//                         g at all; without one no pixel of the row has a site within max_d2 and the row is filled with (0, -1).
//                         Otherwise a lane per pixel starts at (g^2, clab) of its own column and walks dx = 1, 2, ... while
//                         dx^2 <= min(best, max_d2), taking the smaller (dx^2 + g^2, clab) of the columns x - dx and x + dx.  The
//                         bound is <=, not <: a column at dx^2 == best with g == 0 ties the distance and may hold a lower label.
//                         clab is read (from global memory) only for a column whose distance is at most the best so far.
// Exact: dx^2 is constant within a column, so the minimum over all sites is the minimum over the columns of dx^2 plus the column's
// own minimum, which its nearest site above or below attains (the lower label at a tie, by launch 3); every column with dx^2 <= the
// final d2 has been looked at, and a column beyond cannot hold a pixel as near.  A g above R is dropped by launch 3: its g^2 alone
// is beyond max_d2.
// gs_foreign_dist, two launches.
//   1 foreign_rows_kernel   one wave per row: the row in chunks of 64 pixels left to right, then right to left.  A lane tests its
//                           pixel (boundary_links.h's boundary_pixel), the wave's ballot of the tests gives every lane the nearest
//                           set bit at or below / at or above its own, and the nearest column of the chunks already done is carried
//                           in a register: a segmented scan in the wave.  It writes the column of the nearest boundary pixel of any
//                           instance at or left of x and at or right of x, kLinkNone for none.
//   2 foreign_query_kernel  one lane per pixel.  A boundary pixel of instance a walks the rows y, y-1, y+1, y-2, ... while
//                           k^2 <= min(best, max_d2); in a row it hops from x to the left and to the right along the links, skips
//                           the pixels of a and takes the first pixel of another instance on each side; a hop sequence ends at
//                           dx^2 + k^2 > min(best, max_d2), at none or at the row's end.  Every other lane stores (-1, 0).
// Exact: the nearest pixel of an instance seen from outside it is a boundary pixel of it (an inner pixel has a 4-neighbour of its
// instance that is nearer), so the minimum and every tie lie on the links; in a row the first foreign pixel the links reach on a
// side is the nearest on that side; rows are visited in order of k, and a row with k^2 > best cannot hold a pixel as near.  The
// bounds are <= for the id tie, as above.
// With n == 0 every pixel is background: zone_fill_kernel alone writes both outputs.
//
// Why the output does not depend on the run: every table and every output element is a pure function of the inputs and is written
// by exactly one lane; there are no atomics.
//
// Visibility.  Per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores.  Across
// launches visibility comes from the kernel boundary alone: what a launch stores plainly is read plainly only by later launches,
// and never inside the launch that stores it.  The row pass's LDS is written and read by one workgroup, behind its one barrier.
//
// Rules: those of wave_block.h.  No kernel waits on another workgroup; an entry allocates nothing, waits for nothing on the host
// and writes every byte of workspace that it later reads, so the workspace contents on entry do not matter.  The loops --
//   the band walks        i rises (falls) by one over the kZoneBand rows of the band, fully unrolled
//   the carry walks       b rises by one to `bands`, then falls by one to 0: at most 1024 rounds each
//   staging, row sweep    x rises by 256 until it passes `width`
//   the dx search         dx rises by one while dx * dx <= min(best, max_d2); best never grows: dx <= 32768.  It ends at the
//                         latest when both x - dx and x + dx lie outside the map: dx < width
//   the row pass          x0 rises (falls) by 256 per round until it leaves [0, width)
//   the row walk          k rises by one per round and stops at k * k > min(best, max_d2), at height, or when both rows y - k and
//                         y + k lie outside the map
//   a hop sequence        the column strictly falls (left) or rises (right) with every hop: a link at c - 1 is at most c - 1, one
//                         at c + 1 at least c + 1: at most width hops
// A link is a column the row pass itself stored (< width) or kLinkNone, so no link leads out of its row.  Nothing is indexed by a
// label: a label is only compared, after its range test.
#include "gs_internal.h"
#include "zones_plan.h"
#include "zones_abi.h"
#include "boundary_links.h"

namespace gs {

namespace {

typedef unsigned long long u64;
typedef unsigned short u16;

constexpr int kThreads = kZoneThreads;
static_assert(kThreads == 256, "four waves per workgroup: the row pass's wave index");
constexpr int kFar = 1 << 20;                      // a distance in rows beyond every map: "no instance pixel on this side"
constexpr int kBatch = 4, kSpan = 64 * kBatch;     // the row pass tests this many chunks of 64 pixels before it links them

__device__ inline bool in_range(int v, int n) { return v >= 1 && v <= n; }

__global__ __launch_bounds__(kThreads) void zone_fill_kernel(int *__restrict__ a, int va, int *__restrict__ b, int vb, long long pixels)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < pixels) {
        a[i] = va;
        b[i] = vb;
    }
}

// ------------------------------------------------------------------------------------------------------------------- the zones
__global__ __launch_bounds__(kThreads) void zone_count_kernel(const int *__restrict__ L, int n, int H, int W, int col_tiles,
                                                              u16 *__restrict__ top_d, u16 *__restrict__ bot_d, int *__restrict__ top_l,
                                                              int *__restrict__ bot_l)
{
    const int b = (int)blockIdx.x / col_tiles, x = ((int)blockIdx.x - b * col_tiles) * kThreads + (int)threadIdx.x;
    if (x >= W)
        return;
    const int y0 = b * kZoneBand, rows = H - y0 < kZoneBand ? H - y0 : kZoneBand;
    int first = kZoneNone, last = kZoneNone, first_l = 0, last_l = 0;
#pragma unroll
    for (int i = 0; i < kZoneBand; ++i)
        if (i < rows) {
            const int v = L[(size_t)(y0 + i) * W + x];
            if (in_range(v, n)) {
                if (first == kZoneNone) {
                    first = i;
                    first_l = v;
                }
                last = rows - 1 - i;
                last_l = v;
            }
        }
    const size_t at = (size_t)b * W + x;
    top_d[at] = (u16)first;
    top_l[at] = first_l;
    bot_d[at] = (u16)last;
    bot_l[at] = last_l;
}

__global__ __launch_bounds__(kThreads) void zone_carry_kernel(const u16 *__restrict__ top_d, const u16 *__restrict__ bot_d,
                                                              const int *__restrict__ top_l, const int *__restrict__ bot_l, int H, int W,
                                                              int bands, u16 *__restrict__ down_d, u16 *__restrict__ up_d,
                                                              int *__restrict__ down_l, int *__restrict__ up_l)
{
    const int x = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (x >= W)
        return;
    int carry = kZoneNone, label = 0;              // a distance is at most H - 1 <= 32767: 16 bits, kZoneNone apart
    for (int b = 0; b < bands; ++b) {
        const int rows = H - b * kZoneBand < kZoneBand ? H - b * kZoneBand : kZoneBand;
        const size_t at = (size_t)b * W + x;
        down_d[at] = (u16)carry;
        down_l[at] = label;
        const int bd = bot_d[at];
        if (bd != kZoneNone) {
            carry = bd + 1;
            label = bot_l[at];
        } else if (carry != kZoneNone)
            carry += rows;
    }
    carry = kZoneNone;
    label = 0;
    for (int b = bands - 1; b >= 0; --b) {
        const int rows = H - b * kZoneBand < kZoneBand ? H - b * kZoneBand : kZoneBand;
        const size_t at = (size_t)b * W + x;
        up_d[at] = (u16)carry;
        up_l[at] = label;
        const int td = top_d[at];
        if (td != kZoneNone) {
            carry = td + 1;
            label = top_l[at];
        } else if (carry != kZoneNone)
            carry += rows;
    }
}

__global__ __launch_bounds__(kThreads) void zone_apply_kernel(const int *__restrict__ L, int n, int H, int W, int col_tiles, int reach,
                                                              const u16 *__restrict__ down_d, const u16 *__restrict__ up_d,
                                                              const int *__restrict__ down_l, const int *__restrict__ up_l,
                                                              u16 *__restrict__ g, int *__restrict__ clab)
{
    const int b = (int)blockIdx.x / col_tiles, x = ((int)blockIdx.x - b * col_tiles) * kThreads + (int)threadIdx.x;
    if (x >= W)
        return;
    const int y0 = b * kZoneBand, rows = H - y0 < kZoneBand ? H - y0 : kZoneBand;
    const size_t at = (size_t)b * W + x;
    int dn[kZoneBand], dl[kZoneBand];
    int d = down_d[at], lab = down_l[at];
    d = d == kZoneNone ? kFar : d - 1;             // the distance at the row above the band; kFar + 32 per band never overflows
#pragma unroll
    for (int i = 0; i < kZoneBand; ++i) {
        dn[i] = kFar;
        dl[i] = 0;
        if (i < rows) {
            const int v = L[(size_t)(y0 + i) * W + x];
            const bool site = in_range(v, n);
            d = site ? 0 : d < kFar ? d + 1 : kFar;
            lab = site ? v : lab;
            dn[i] = d;
            dl[i] = lab;
        }
    }
    int u = up_d[at], ul = up_l[at];
    u = u == kZoneNone ? kFar : u - 1;
#pragma unroll
    for (int i = kZoneBand - 1; i >= 0; --i)
        if (i < rows) {
            const bool site = dn[i] == 0;
            u = site ? 0 : u < kFar ? u + 1 : kFar;
            ul = site ? dl[i] : ul;
            int best = dn[i], bl = dl[i];
            if (u < best || (u == best && ul < bl)) {
                best = u;
                bl = ul;
            }
            const bool none = best > reach;        // kFar too: reach <= 32768
            g[(size_t)(y0 + i) * W + x] = (u16)(none ? kZoneNone : best);      // <= 32767
            clab[(size_t)(y0 + i) * W + x] = none ? 0 : bl;
        }
}

// column c at squared horizontal distance dd: (dd + g^2, clab) replaces (best, lab) where it is lexicographically smaller and
// within max_d2.  clab is read only where the distance is at most the best so far.
__device__ inline void zone_take(const u16 *row, const int *__restrict__ clab, int c, int dd, int max_d2, int &best, int &lab)
{
    const int gv = row[c];
    if (gv == kZoneNone)
        return;
    const int v = dd + gv * gv;                    // dd <= 2^30, gv <= 32767: < 2^31
    if (v > best || v > max_d2)
        return;
    const int l = clab[c];
    if (v < best || l < lab) {
        best = v;
        lab = l;
    }
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void zone_row_kernel(const u16 *__restrict__ g, const int *__restrict__ clab, int W, int max_d2,
                                                            int *__restrict__ zone, int *__restrict__ zone_d2)
{
    extern __shared__ __attribute__((aligned(16))) u16 s_zone_row[];               // [width] where kLds
    const u16 *grow = g + (size_t)blockIdx.x * W;
    const int *lrow = clab + (size_t)blockIdx.x * W;
    int *out_zone = zone + (size_t)blockIdx.x * W, *out_d2 = zone_d2 + (size_t)blockIdx.x * W;
    int any = 0;
    for (int x = (int)threadIdx.x; x < W; x += kThreads) {
        const u16 v = grow[x];
        if (kLds)
            s_zone_row[x] = v;
        any |= v != kZoneNone;
    }
    any = __syncthreads_or(any);                   // every thread of the workgroup: the loop above holds no barrier
    if (!any) {                                    // the whole workgroup: no column of this row has a site within reach
        for (int x = (int)threadIdx.x; x < W; x += kThreads) {
            out_zone[x] = 0;
            out_d2[x] = -1;
        }
        return;
    }
    const u16 *row = kLds ? s_zone_row : grow;
    const int none = max_d2 + 1;                   // <= 2^30 + 1
    for (int x = (int)threadIdx.x; x < W; x += kThreads) {
        const int gv = row[x];
        int best = none, lab = 0;
        if (gv != kZoneNone) {
            best = gv * gv;                        // gv <= floor(sqrt(max_d2)): within max_d2
            lab = lrow[x];
        }
        for (int dx = 1; dx < W; ++dx) {           // beyond W - 1 both columns lie outside
            const int dd = dx * dx;                // dx <= 32767
            if (dd > best || dd > max_d2)
                break;
            if (x - dx >= 0)
                zone_take(row, lrow, x - dx, dd, max_d2, best, lab);
            if (x + dx < W)
                zone_take(row, lrow, x + dx, dd, max_d2, best, lab);
            if (x - dx < 0 && x + dx >= W)
                break;
        }
        out_zone[x] = best == none ? 0 : lab;
        out_d2[x] = best == none ? -1 : best;
    }
}

// ------------------------------------------------------------------------------------------------------------------- the gaps
__global__ __launch_bounds__(kThreads) void foreign_rows_kernel(const int *__restrict__ L, int n, int H, int W, u16 *__restrict__ left_all,
                                                                u16 *__restrict__ right_all)
{
    const int lane = threadIdx.x & 63;
    const int y = (int)blockIdx.x * (kThreads / 64) + (int)(threadIdx.x >> 6);         // < 32768 + 4
    if (y >= H)                                    // the whole wave
        return;
    u16 *__restrict__ left = left_all + (size_t)y * W;
    u16 *__restrict__ right = right_all + (size_t)y * W;
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

// The lexicographic minimum of (d2, label) over the pixels of instances other than a within max_d2 of (x, y); best = max_d2 + 1
// where there is none.  Every column the links give holds a boundary pixel of an instance: its label is in 1..n.
__device__ inline void nearest_foreign(const int *__restrict__ L, const u16 *__restrict__ left, const u16 *__restrict__ right, int a, int H,
                                       int W, int y, int x, int max_d2, int &best, int &id)
{
    best = max_d2 + 1;                             // <= 2^30 + 1
    id = 0;
    for (int k = 0; k < H; ++k) {
        const int kk = k * k;                      // k <= 32767
        if (kk > best || kk > max_d2)
            break;
        const bool above = y - k >= 0, below = y + k < H;
        if (!above && !below)
            break;
        for (int s = 0; s < (k ? 2 : 1); ++s) {
            if (s == 0 ? !above : !below)
                continue;
            const size_t row = (size_t)(s == 0 ? y - k : y + k) * W;
            int c = left[row + x];
            while (c != kLinkNone) {               // c falls with every hop
                const int d = (x - c) * (x - c) + kk;                  // < 2^31
                if (d > best || d > max_d2)
                    break;
                const int t = L[row + c];
                if (t != a) {
                    if (d < best || t < id) {
                        best = d;
                        id = t;
                    }
                    break;
                }
                if (c == 0)
                    break;
                c = left[row + c - 1];
            }
            c = right[row + x];
            while (c != kLinkNone) {               // c rises with every hop
                const int d = (c - x) * (c - x) + kk;
                if (d > best || d > max_d2)
                    break;
                const int t = L[row + c];
                if (t != a) {
                    if (d < best || t < id) {
                        best = d;
                        id = t;
                    }
                    break;
                }
                if (c == W - 1)
                    break;
                c = right[row + c + 1];
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void foreign_query_kernel(const int *__restrict__ L, int n, const u16 *__restrict__ left,
                                                                 const u16 *__restrict__ right, int H, int W, int max_d2,
                                                                 int *__restrict__ near_d2, int *__restrict__ near_id)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x, pixels = (long long)H * W;
    if (i >= pixels)
        return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    int a, d2 = -1, id = 0;
    if (boundary_pixel(L, n, H, W, y, x, a)) {
        int best;
        nearest_foreign(L, left, right, a, H, W, y, x, max_d2, best, id);
        d2 = best > max_d2 ? -1 : best;
    }
    near_d2[i] = d2;
    near_id[i] = id;
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" gs_status gs_instance_zones_plan(int height, int width, size_t *workspace_bytes)
{
    GS_REQUIRE(workspace_bytes, "gs_instance_zones_plan: null argument");
    ZonePlan plan;
    const gs_status st = plan_zones(height, width, plan);
    *workspace_bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_foreign_dist_plan(int height, int width, size_t *workspace_bytes)
{
    GS_REQUIRE(workspace_bytes, "gs_foreign_dist_plan: null argument");
    ForeignPlan plan;
    const gs_status st = plan_foreign(height, width, plan);
    *workspace_bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_instance_zones(const int32_t *labels, int n, int height, int width, int max_d2, void *workspace,
                                       size_t workspace_bytes, int32_t *zone, int32_t *zone_d2, void *hip_stream)
{
    ZonePlan plan;
    gs_status st = plan_zones(height, width, plan);
    if (st != GS_OK)
        return st;
    if ((st = check_zone_count("gs_instance_zones", n)) != GS_OK || (st = check_zone_cap("gs_instance_zones", max_d2)) != GS_OK)
        return st;
    GS_REQUIRE(aligned(labels, 4), "gs_instance_zones: labels is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 8), "gs_instance_zones: workspace is NULL or not 8-byte aligned");
    GS_REQUIRE(aligned(zone, 4), "gs_instance_zones: zone is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(zone_d2, 4), "gs_instance_zones: zone_d2 is NULL or not 4-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_instance_zones: a map of %d x %d needs %zu bytes of workspace (got %zu)", height, width,
               plan.bytes, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (n == 0) {
        hipLaunchKernelGGL(zone_fill_kernel, dim3((unsigned)plan.pixel_blocks), dim3(kThreads), 0, s, zone, 0, zone_d2, -1,
                           (long long)height * width);
        GS_HIP(hipGetLastError());
        return GS_OK;
    }
    char *ws = static_cast<char *>(workspace);
    u16 *g = reinterpret_cast<u16 *>(ws + plan.g_off);
    int *clab = reinterpret_cast<int *>(ws + plan.clab_off);
    u16 *top_d = reinterpret_cast<u16 *>(ws + plan.top_d_off), *bot_d = reinterpret_cast<u16 *>(ws + plan.bot_d_off);
    u16 *down_d = reinterpret_cast<u16 *>(ws + plan.down_d_off), *up_d = reinterpret_cast<u16 *>(ws + plan.up_d_off);
    int *top_l = reinterpret_cast<int *>(ws + plan.top_l_off), *bot_l = reinterpret_cast<int *>(ws + plan.bot_l_off);
    int *down_l = reinterpret_cast<int *>(ws + plan.down_l_off), *up_l = reinterpret_cast<int *>(ws + plan.up_l_off);
    const int reach = zone_isqrt(max_d2);          // <= 32768

    hipLaunchKernelGGL(zone_count_kernel, dim3((unsigned)plan.band_blocks), dim3(kThreads), 0, s, labels, n, height, width, plan.col_tiles,
                       top_d, bot_d, top_l, bot_l);
    hipLaunchKernelGGL(zone_carry_kernel, dim3((unsigned)plan.carry_blocks), dim3(kThreads), 0, s, top_d, bot_d, top_l, bot_l, height, width,
                       plan.bands, down_d, up_d, down_l, up_l);
    hipLaunchKernelGGL(zone_apply_kernel, dim3((unsigned)plan.band_blocks), dim3(kThreads), 0, s, labels, n, height, width, plan.col_tiles,
                       reach, down_d, up_d, down_l, up_l, g, clab);
    if (plan.row_lds_bytes > 0)
        hipLaunchKernelGGL(zone_row_kernel<true>, dim3((unsigned)height), dim3(kThreads), (size_t)plan.row_lds_bytes, s, g, clab, width,
                           max_d2, zone, zone_d2);
    else
        hipLaunchKernelGGL(zone_row_kernel<false>, dim3((unsigned)height), dim3(kThreads), 0, s, g, clab, width, max_d2, zone, zone_d2);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

extern "C" gs_status gs_foreign_dist(const int32_t *labels, int n, int height, int width, int max_d2, void *workspace, size_t workspace_bytes,
                                     int32_t *near_d2, int32_t *near_id, void *hip_stream)
{
    ForeignPlan plan;
    gs_status st = plan_foreign(height, width, plan);
    if (st != GS_OK)
        return st;
    if ((st = check_zone_count("gs_foreign_dist", n)) != GS_OK || (st = check_zone_cap("gs_foreign_dist", max_d2)) != GS_OK)
        return st;
    GS_REQUIRE(aligned(labels, 4), "gs_foreign_dist: labels is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 8), "gs_foreign_dist: workspace is NULL or not 8-byte aligned");
    GS_REQUIRE(aligned(near_d2, 4), "gs_foreign_dist: near_d2 is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(near_id, 4), "gs_foreign_dist: near_id is NULL or not 4-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_foreign_dist: a map of %d x %d needs %zu bytes of workspace (got %zu)", height, width,
               plan.bytes, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (n == 0) {
        hipLaunchKernelGGL(zone_fill_kernel, dim3((unsigned)plan.pixel_blocks), dim3(kThreads), 0, s, near_d2, -1, near_id, 0,
                           (long long)height * width);
        GS_HIP(hipGetLastError());
        return GS_OK;
    }
    char *ws = static_cast<char *>(workspace);
    u16 *left = reinterpret_cast<u16 *>(ws + plan.left_off), *right = reinterpret_cast<u16 *>(ws + plan.right_off);
    hipLaunchKernelGGL(foreign_rows_kernel, dim3((unsigned)plan.row_blocks), dim3(kThreads), 0, s, labels, n, height, width, left, right);
    hipLaunchKernelGGL(foreign_query_kernel, dim3((unsigned)plan.pixel_blocks), dim3(kThreads), 0, s, labels, n, left, right, height, width,
                       max_d2, near_d2, near_id);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
