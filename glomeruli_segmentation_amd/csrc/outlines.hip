// Per-glomerulus outlines (csrc/outlines_abi.h, gs_instance_outlines): for every instance of a label map the closed loops of its
// crack edges -- one for its outer boundary, one for each hole -- as lists of lattice corner points in a fixed order.  The
// definitions (lattice, edges, successor, loops, points) are the header's; everything is integer.
//
// gs_instance_outlines keeps a head, a word per pixel and 53 bytes per edge in the caller's workspace (outlines_plan.h), in
// 12 + rounds launches, none of which needs a sort:
//   1 out_count_kernel        one lane per pixel: the crack edges of the pixel (its sides whose neighbour is not in its instance),
//                             summed per workgroup of 256 pixels.
//   2 out_scan_pixels_kernel  one workgroup of 1024: the block sums become the edges in front of each block (wave_block.h's scan,
//                             with 64-bit sums: a map can hold more than 2^31 edges); the total is edges_needed and decides whether
//                             the result fits.  Writes the head and counts[0]; counts[1] = counts[2] = -1 where it does not fit.
//   3 out_number_kernel       per pixel again: the pixel's base = the block's + the edges of the pixels in front of it in the
//                             block (a shuffle scan per wave, the waves' sums in LDS).  An edge's dense index is its pixel's base
//                             plus the pixel's edges of lower side, so dense order is key order (key = 4 * pixel + side).  Writes
//                             the base of every pixel and the pixel and side of every edge.
//   4 out_succ_kernel         one lane per edge: the successor by the header's rule, as a dense index (the target pixel's base plus
//                             its edges of lower side, recomputed from the labels), and the first jumping state: the window is the
//                             edge itself.
//   5 out_jump_kernel         `rounds` launches, ping-pong between two state buffers: an edge whose state covers its next 2^k
//                             edges takes the state of the edge 2^k ahead and covers 2^(k+1).  A state holds the smallest dense
//                             index of the window and the steps to its first occurrence; the combine is strict (<), so of equal
//                             minima (a window that has gone round the loop) the nearer stays.  rounds is the plan's, from
//                             edges_cap alone: 2^rounds >= edges_cap >= the edges of any loop, so at the end every edge knows its
//                             loop's key edge (the smallest index) and its distance forward to it.
//   6 out_loop_count_kernel   per edge: a key edge is its own minimum; its loop's length is the distance of its successor to it,
//                             plus one.  Key edges and their lengths are summed per workgroup.
//   7 out_scan_loops_kernel   both block sums scanned; the total of the first is n_loops.
//   8 out_loop_rank_kernel    a key edge's rank among the key edges is its loop's number (key order), the lengths in front of it
//                             are its loop's first row of the edges in loop order.  Writes loop_label, loop_first, loop_edges,
//                             loop_area2 = 0, and number, first row and length into the key edge's row of the state buffer that the
//                             last round did not write.
//   9 out_order_kernel        per edge: rank = (length - distance to the key edge) mod length, row = the loop's first + rank.  The
//                             row takes the edge's end vertex where the successor's side differs (a corner; x = -1 where not) and
//                             the loop's number where rank = 0.  The area term goes to loop_area2: the lanes of a wave are grouped
//                             by loop (for_each_wave_group), reduced by shuffles, one 64-bit atomic add per group.
//  10 out_corner_count_kernel per row: corners per workgroup.
//  11 out_scan_points_kernel  scanned; the total is n_points = loop_offsets[n_loops].
//  12 out_points_kernel       a corner's rank among the corners is its place in `points`; the row where a loop begins writes the
//                             corners in front of it to loop_offsets.
// Launches 1..3 are sized by the map, the others by edges_cap: a lane beyond edges_needed, and every lane where the result does
// not fit, does nothing but take its workgroup's barriers.  The entry reads no device value: the round count, the grids and the
// buffer that holds the final states follow from edges_cap on the host.
//
// Why the result is exact: the successor maps the edges of an instance onto themselves one to one (the header), so following
// `jump` never leaves the loop and the window of round k is the next 2^k edges, with repetition once it is longer than the loop.
// The first occurrence of the minimum in a window that covers the loop lies less than one loop length ahead.
//
// Why the bytes do not depend on the run: everything but loop_area2 is a pure function of the labels, written by one thread;
// loop_area2 is zeroed in launch 8 and then only added to, with integers, in launch 9.
//
// Visibility: across launches the kernel boundary alone; a launch never reads what it writes (the jumping rounds read one state
// buffer and write the other).  loop_area2 in launch 9 is touched only through agent-scope atomics.
//
// Rules: those of wave_block.h.  The loops of this file's own --
//   the four sides           s rises from 0 to 3
//   the wave scan            off doubles up to 64; the LDS sums are read behind the workgroup's one barrier, reached by all
//   the block scan           wave_block.h's, b rises by one over the thread's run of blocks, d doubles up to 1024
//   the shuffle reduction    off halves from 32
// An index is used only where it is known to lie in range: a pixel index comes from the lane's own position or is a neighbour
// inside the map; a dense index is below edges_needed <= edges_cap by construction and is tested once more where it is made
// (launches 4 and 9); a loop number is tested against the rows of the loop tables (edges_cap / 4) before it is written through.
#include "gs_internal.h"
#include "outlines_abi.h"
#include "outlines_plan.h"
#include "wave_block.h"

namespace gs {

namespace {

typedef unsigned long long u64;

constexpr int kThreads = kOutThreads;
static_assert(kThreads == 256 && kThreads == kFlagThreads, "four waves a workgroup");

// the heading of an edge of side s (0 top: east, 1 right: south, 2 bottom: west, 3 left: north); y grows downwards
__device__ inline int head_dx(int s) { return s == 0 ? 1 : s == 2 ? -1 : 0; }
__device__ inline int head_dy(int s) { return s == 1 ? 1 : s == 3 ? -1 : 0; }

__device__ inline bool in_instance(const int *__restrict__ L, int H, int W, int x, int y, int i)
{
    return x >= 0 && y >= 0 && x < W && y < H && L[(size_t)y * W + x] == i;
}

// bit s: side s of pixel (x, y) of instance i is a crack edge.  The neighbour across side s lies to the left of its heading.
__device__ inline int edge_mask(const int *__restrict__ L, int H, int W, int x, int y, int i)
{
    int m = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (!in_instance(L, H, W, x + head_dx((s + 3) & 3), y + head_dy((s + 3) & 3), i))
            m |= 1 << s;
    return m;
}

// the edges of pixel p (0 for a pixel of no instance, and beyond the map)
__device__ inline int pixel_edges(const int *__restrict__ L, int n, int H, int W, long long p, int n_pixels)
{
    if (p >= n_pixels)
        return 0;
    const int i = L[p];
    if (i < 1 || i > n)
        return 0;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    return edge_mask(L, H, W, x, y, i);
}

// For each of N values of a workgroup of kThreads: before = the sum over the threads in front of this one, total = over all.
// Every thread of the workgroup calls it, once per kernel (the LDS words are the instantiation's own).
template <int N>
__device__ inline void block_prefix(const int (&v)[N], int (&before)[N], int (&total)[N])
{
    __shared__ int wave_sum[N][kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc[N];
#pragma unroll
    for (int j = 0; j < N; ++j)
        inc[j] = v[j];
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int o = __shfl_up(inc[j], off);
            if (lane >= off)
                inc[j] += o;
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int j = 0; j < N; ++j)
            wave_sum[j][wave] = inc[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int b = 0, t = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int s = wave_sum[j][w];
            b += w < wave ? s : 0;
            t += s;
        }
        before[j] = b + inc[j] - v[j];
        total[j] = t;
    }
}

// 1 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void out_count_kernel(const int *__restrict__ L, int n, int H, int W, int n_pixels,
                                                             int *__restrict__ pixel_count)
{
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int v[1] = {(int)__popc(pixel_edges(L, n, H, W, p, n_pixels))};
    int before[1], total[1];
    block_prefix<1>(v, before, total);
    if (threadIdx.x == 0)
        pixel_count[blockIdx.x] = total[0];        // at most 1024
}

// 2 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void out_scan_pixels_kernel(int *__restrict__ pixel_count, int n_blocks, int edges_cap,
                                                                       OutHead *__restrict__ head, long long *__restrict__ counts)
{
    __shared__ long long s[kScanThreads];
    const int t = (int)threadIdx.x, run = (n_blocks + kScanThreads - 1) / kScanThreads;
    const long long lo = (long long)t * run, hi = lo + run < n_blocks ? lo + run : n_blocks;
    long long sum = 0;
    for (long long b = lo; b < hi; ++b)
        sum += pixel_count[b];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const long long v = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    const long long total = s[kScanThreads - 1];   // at most 4 * n_pixels < 2^33
    const bool fits = total <= edges_cap;
    long long base = s[t] - sum;
    for (long long b = lo; b < hi; ++b) {
        const int c = pixel_count[b];
        pixel_count[b] = fits ? (int)base : 0;     // read only where the result fits: then every base is below 2^31
        base += c;
    }
    if (t == 0) {
        head->edges_needed = total;
        head->fits = fits ? 1 : 0;
        head->n_loops = 0;
        head->n_points = 0;
        head->pad = 0;
        counts[0] = total;
        if (!fits)
            counts[1] = counts[2] = -1;
    }
}

// 3 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void out_number_kernel(const int *__restrict__ L, int n, int H, int W, int n_pixels,
                                                              const OutHead *__restrict__ head, const int *__restrict__ pixel_count,
                                                              int *__restrict__ pixel_base, int *__restrict__ edge_pixel,
                                                              unsigned char *__restrict__ edge_side)
{
    if (!head->fits)                               // the whole workgroup
        return;
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int m = pixel_edges(L, n, H, W, p, n_pixels);
    const int v[1] = {(int)__popc(m)};
    int before[1], total[1];
    block_prefix<1>(v, before, total);
    if (p >= n_pixels)
        return;
    int k = pixel_count[blockIdx.x] + before[0];   // k + popc(m) <= edges_needed <= edges_cap
    pixel_base[p] = k;
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (m >> s & 1) {
            edge_pixel[k] = (int)p;
            edge_side[k] = (unsigned char)s;
            ++k;
        }
}

// 4 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void out_succ_kernel(const int *__restrict__ L, int H, int W, int connectivity,
                                                            const OutHead *__restrict__ head, const int *__restrict__ pixel_base,
                                                            const int *__restrict__ edge_pixel, const unsigned char *__restrict__ edge_side,
                                                            OutState *__restrict__ state)
{
    const long long d = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (!head->fits || d >= head->edges_needed)
        return;
    const int needed = (int)head->edges_needed;
    const int p = edge_pixel[d], s = edge_side[d];
    const int y = p / W, x = p - y * W;
    const int i = L[p];                            // launch 3 numbered the edges of instance pixels only: 1 <= i <= n
    const int left = (s + 3) & 3;
    const int arx = x + head_dx(s), ary = y + head_dy(s);             // ahead and to the right of the heading
    const int alx = arx + head_dx(left), aly = ary + head_dy(left);   // ahead and to the left
    const bool ar = in_instance(L, H, W, arx, ary, i), al = in_instance(L, H, W, alx, aly, i);
    const int turn = connectivity == 8 ? (al ? 0 : ar ? 1 : 2) : (!ar ? 2 : al ? 0 : 1);      // 0 left, 1 straight, 2 right
    const int qx = turn == 0 ? alx : turn == 1 ? arx : x, qy = turn == 0 ? aly : turn == 1 ? ary : y;
    const int qs = turn == 0 ? left : turn == 1 ? s : (s + 1) & 3;
    const int qm = edge_mask(L, H, W, qx, qy, i);  // (qx, qy) is in i, and its side qs is an edge (the header's rule)
    int succ = pixel_base[(size_t)qy * W + qx] + __popc(qm & ((1 << qs) - 1));
    if (succ < 0 || succ >= needed)
        succ = (int)d;
    OutState o;
    o.min = (int)d;
    o.off = 0;
    o.jump = succ;
    o.succ = succ;
    state[d] = o;
}

// 5 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void out_jump_kernel(const OutHead *__restrict__ head, const OutState *__restrict__ src,
                                                            OutState *__restrict__ dst, unsigned step)
{
    const long long d = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (!head->fits || d >= head->edges_needed)
        return;
    OutState a = src[d];
    const OutState b = src[a.jump];                // a dense index of the same loop: below edges_needed
    if (b.min < a.min) {
        a.min = b.min;
        a.off = (int)((unsigned)b.off + step);     // a first occurrence: less than the loop's length
    }
    a.jump = b.jump;
    dst[d] = a;
}

// 6, 8 ---------------------------------------------------------------------------------------------------------------------
// whether edge d is its loop's key edge, and then the loop's edges
__device__ inline bool key_edge(const OutHead *__restrict__ head, const OutState *__restrict__ fin, long long d, int &len)
{
    len = 0;
    if (!head->fits || d >= head->edges_needed)
        return false;
    const OutState a = fin[d];
    if (a.min != (int)d)
        return false;
    len = fin[a.succ].off + 1;                     // the successor of the key edge is the farthest from it
    return true;
}

__global__ __launch_bounds__(kThreads) void out_loop_count_kernel(const OutHead *__restrict__ head, const OutState *__restrict__ fin,
                                                                  int *__restrict__ count_a, int *__restrict__ count_b)
{
    const long long d = (long long)blockIdx.x * kThreads + threadIdx.x;
    int len;
    const bool key = key_edge(head, fin, d, len);
    const int v[2] = {key ? 1 : 0, len};           // the lengths of distinct loops sum to at most edges_needed
    int before[2], total[2];
    block_prefix<2>(v, before, total);
    if (threadIdx.x == 0) {
        count_a[blockIdx.x] = total[0];
        count_b[blockIdx.x] = total[1];
    }
}

// 7 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void out_scan_loops_kernel(int *__restrict__ count_a, int *__restrict__ count_b, int n_blocks,
                                                                      OutHead *__restrict__ head, long long *__restrict__ counts)
{
    const int n_loops = block_scan_exclusive(count_a, n_blocks);
    __syncthreads();                               // the scan's LDS is read to the end before the next one fills it
    block_scan_exclusive(count_b, n_blocks);
    if (threadIdx.x == 0 && head->fits) {
        head->n_loops = n_loops;
        counts[1] = n_loops;
    }
}

__global__ __launch_bounds__(kThreads) void out_loop_rank_kernel(const int *__restrict__ L, const OutHead *__restrict__ head,
                                                                 const OutState *__restrict__ fin, OutLoop *__restrict__ loops,
                                                                 const int *__restrict__ count_a, const int *__restrict__ count_b,
                                                                 const int *__restrict__ edge_pixel, int loop_rows,
                                                                 int *__restrict__ loop_label, int *__restrict__ loop_first,
                                                                 int *__restrict__ loop_edges, long long *__restrict__ loop_area2)
{
    const long long d = (long long)blockIdx.x * kThreads + threadIdx.x;
    int len;
    const bool key = key_edge(head, fin, d, len);
    const int v[2] = {key ? 1 : 0, len};
    int before[2], total[2];
    block_prefix<2>(v, before, total);
    if (!key)
        return;
    OutLoop o;
    o.loop = count_a[blockIdx.x] + before[0];
    o.base = count_b[blockIdx.x] + before[1];
    o.len = len;
    o.pad = 0;
    loops[d] = o;
    if (o.loop < loop_rows) {                      // a loop has at least four edges: always
        const int p = edge_pixel[d];
        loop_label[o.loop] = L[p];
        loop_first[o.loop] = p;
        loop_edges[o.loop] = len;
        loop_area2[o.loop] = 0;
    }
}

// 9 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void out_order_kernel(int W, const OutHead *__restrict__ head, const OutState *__restrict__ fin,
                                                             const OutLoop *__restrict__ loops, const int *__restrict__ edge_pixel,
                                                             const unsigned char *__restrict__ edge_side, int loop_rows,
                                                             OutRow *__restrict__ rows, long long *loop_area2)
{
    const int lane = threadIdx.x & 63;
    const long long d = (long long)blockIdx.x * kThreads + threadIdx.x;
    bool todo = false;
    int loop = 0;
    long long term = 0;
    if (head->fits && d < head->edges_needed) {
        const int needed = (int)head->edges_needed;
        const OutState a = fin[d];
        const OutLoop lp = loops[a.min];           // written by launch 8 for every key edge
        const int rank = a.off ? lp.len - a.off : 0;
        const long long row = (long long)lp.base + rank;
        const int p = edge_pixel[d], s = edge_side[d];
        const int y = p / W, x = p - y * W;
        const long long sx = x + (s == 1 || s == 2), sy = y + (s >= 2), ex = x + (s < 2), ey = y + (s == 1 || s == 2);
        term = sx * ey - ex * sy;
        if (rank >= 0 && row >= 0 && row < needed) {
            OutRow o;
            o.x = edge_side[a.succ] != s ? (int)ex : -1;
            o.y = (int)ey;
            o.loop = rank == 0 ? lp.loop : -1;
            o.pad = 0;
            rows[row] = o;
        }
        loop = lp.loop;
        todo = loop >= 0 && loop < loop_rows && term != 0;
    }
    // every lane of the wave gets here
    for_each_wave_group(todo, loop, [&](int first, u64 group, bool mine) {
        long long v = mine ? term : 0;             // 64 terms below 2^31 each
#pragma unroll
        for (int off = 32; off; off >>= 1)
            v += __shfl_xor(v, off);
        if (lane == first && v)
            __hip_atomic_fetch_add(reinterpret_cast<u64 *>(loop_area2 + loop), (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    });
}

// 10, 12 -------------------------------------------------------------------------------------------------------------------
__device__ inline OutRow row_at(const OutHead *__restrict__ head, const OutRow *__restrict__ rows, long long r)
{
    OutRow o;
    o.x = o.loop = -1;
    o.y = o.pad = 0;
    if (head->fits && r < head->edges_needed)
        o = rows[r];
    return o;
}

__global__ __launch_bounds__(kThreads) void out_corner_count_kernel(const OutHead *__restrict__ head, const OutRow *__restrict__ rows,
                                                                    int *__restrict__ count_a)
{
    const OutRow r = row_at(head, rows, (long long)blockIdx.x * kThreads + threadIdx.x);
    const int v[1] = {r.x >= 0 ? 1 : 0};
    int before[1], total[1];
    block_prefix<1>(v, before, total);
    if (threadIdx.x == 0)
        count_a[blockIdx.x] = total[0];
}

// 11 -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void out_scan_points_kernel(int *__restrict__ count_a, int n_blocks, int loop_rows,
                                                                       OutHead *__restrict__ head, int *__restrict__ loop_offsets,
                                                                       long long *__restrict__ counts)
{
    const int n_points = block_scan_exclusive(count_a, n_blocks);
    if (threadIdx.x == 0 && head->fits) {
        head->n_points = n_points;
        counts[2] = n_points;
        if (head->n_loops <= loop_rows)            // loop_offsets has loop_rows + 1 rows
            loop_offsets[head->n_loops] = n_points;
    }
}

__global__ __launch_bounds__(kThreads) void out_points_kernel(const OutHead *__restrict__ head, const OutRow *__restrict__ rows,
                                                              const int *__restrict__ count_a, int loop_rows, int edges_cap,
                                                              int *__restrict__ loop_offsets, int *__restrict__ points)
{
    const OutRow r = row_at(head, rows, (long long)blockIdx.x * kThreads + threadIdx.x);
    const int v[1] = {r.x >= 0 ? 1 : 0};
    int before[1], total[1];
    block_prefix<1>(v, before, total);
    const int at = count_a[blockIdx.x] + before[0];                   // the corners in front of this row: at most its number
    if (r.x >= 0 && at < edges_cap) {
        points[2 * (size_t)at] = r.x;
        points[2 * (size_t)at + 1] = r.y;
    }
    if (r.loop >= 0 && r.loop < loop_rows)
        loop_offsets[r.loop] = at;
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" gs_status gs_outlines_plan(int height, int width, long long edges_cap, size_t *workspace_bytes)
{
    GS_REQUIRE(workspace_bytes, "gs_outlines_plan: null argument");
    OutlinesPlan plan;
    const gs_status st = plan_outlines(height, width, edges_cap, plan);
    *workspace_bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_instance_outlines(const int32_t *labels, int n, int height, int width, int connectivity, void *workspace,
                                          size_t workspace_bytes, long long edges_cap, int32_t *loop_label, int32_t *loop_first,
                                          int32_t *loop_edges, long long *loop_area2, int32_t *loop_offsets, int32_t *points,
                                          long long *counts, void *hip_stream)
{
    OutlinesPlan plan;
    const gs_status st = plan_outlines(height, width, edges_cap, plan);
    if (st != GS_OK)
        return st;
    const int loop_rows = plan.edges_cap / 4;
    GS_REQUIRE(n >= 0, "gs_instance_outlines: n must not be negative (got %d)", n);
    GS_REQUIRE(connectivity == 4 || connectivity == 8, "gs_instance_outlines: connectivity must be 4 or 8 (got %d)", connectivity);
    GS_REQUIRE(aligned(labels, 4), "gs_instance_outlines: labels is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 16), "gs_instance_outlines: workspace is NULL or not 16-byte aligned");
    GS_REQUIRE(loop_rows == 0 || aligned(loop_label, 4), "gs_instance_outlines: loop_label is NULL or not 4-byte aligned");
    GS_REQUIRE(loop_rows == 0 || aligned(loop_first, 4), "gs_instance_outlines: loop_first is NULL or not 4-byte aligned");
    GS_REQUIRE(loop_rows == 0 || aligned(loop_edges, 4), "gs_instance_outlines: loop_edges is NULL or not 4-byte aligned");
    GS_REQUIRE(loop_rows == 0 || aligned(loop_area2, 8), "gs_instance_outlines: loop_area2 is NULL or not 8-byte aligned");
    GS_REQUIRE(aligned(loop_offsets, 4), "gs_instance_outlines: loop_offsets is NULL or not 4-byte aligned");
    GS_REQUIRE(plan.edges_cap == 0 || aligned(points, 4), "gs_instance_outlines: points is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(counts, 8), "gs_instance_outlines: counts is NULL or not 8-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_instance_outlines: edges_cap %lld needs %zu bytes of workspace (got %zu)", edges_cap,
               plan.bytes, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char *ws = static_cast<char *>(workspace);
    OutHead *head = reinterpret_cast<OutHead *>(ws + plan.head_off);
    int *pixel_count = reinterpret_cast<int *>(ws + plan.pixel_count_off), *pixel_base = reinterpret_cast<int *>(ws + plan.pixel_base_off);
    int *edge_pixel = reinterpret_cast<int *>(ws + plan.edge_pixel_off);
    unsigned char *edge_side = reinterpret_cast<unsigned char *>(ws + plan.edge_side_off);
    int *count_a = reinterpret_cast<int *>(ws + plan.count_a_off), *count_b = reinterpret_cast<int *>(ws + plan.count_b_off);
    OutState *state[2] = {reinterpret_cast<OutState *>(ws + plan.state_off[0]), reinterpret_cast<OutState *>(ws + plan.state_off[1])};
    OutRow *rows = reinterpret_cast<OutRow *>(ws + plan.row_off);
    const dim3 pixel_grid((unsigned)plan.pixel_blocks), edge_grid((unsigned)plan.edge_blocks), block(kThreads), scan(kScanThreads);

    hipLaunchKernelGGL(out_count_kernel, pixel_grid, block, 0, s, labels, n, height, width, plan.n_pixels, pixel_count);
    hipLaunchKernelGGL(out_scan_pixels_kernel, dim3(1), scan, 0, s, pixel_count, plan.pixel_blocks, plan.edges_cap, head, counts);
    hipLaunchKernelGGL(out_number_kernel, pixel_grid, block, 0, s, labels, n, height, width, plan.n_pixels, head, pixel_count, pixel_base,
                       edge_pixel, edge_side);
    hipLaunchKernelGGL(out_succ_kernel, edge_grid, block, 0, s, labels, height, width, connectivity, head, pixel_base, edge_pixel, edge_side,
                       state[0]);
    for (int k = 0; k < plan.rounds; ++k)          // round k reads buffer k & 1 and writes the other
        hipLaunchKernelGGL(out_jump_kernel, edge_grid, block, 0, s, head, state[k & 1], state[(k & 1) ^ 1], 1u << k);
    const OutState *fin = state[plan.rounds & 1];
    OutLoop *loops = reinterpret_cast<OutLoop *>(state[(plan.rounds & 1) ^ 1]);
    hipLaunchKernelGGL(out_loop_count_kernel, edge_grid, block, 0, s, head, fin, count_a, count_b);
    hipLaunchKernelGGL(out_scan_loops_kernel, dim3(1), scan, 0, s, count_a, count_b, plan.edge_blocks, head, counts);
    hipLaunchKernelGGL(out_loop_rank_kernel, edge_grid, block, 0, s, labels, head, fin, loops, count_a, count_b, edge_pixel, loop_rows,
                       loop_label, loop_first, loop_edges, loop_area2);
    hipLaunchKernelGGL(out_order_kernel, edge_grid, block, 0, s, width, head, fin, loops, edge_pixel, edge_side, loop_rows, rows,
                       loop_area2);
    hipLaunchKernelGGL(out_corner_count_kernel, edge_grid, block, 0, s, head, rows, count_a);
    hipLaunchKernelGGL(out_scan_points_kernel, dim3(1), scan, 0, s, count_a, plan.edge_blocks, loop_rows, head, loop_offsets, counts);
    hipLaunchKernelGGL(out_points_kernel, edge_grid, block, 0, s, head, rows, count_a, loop_rows, plan.edges_cap, loop_offsets, points);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
