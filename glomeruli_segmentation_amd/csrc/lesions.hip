// Which classes line which part of a glomerulus' outline (csrc/lesions_abi.h, which has the definitions): for every boundary pixel
// of an instance the classes within reach inside that instance, and for every loop of gs_instance_outlines and every bit of such a
// map the covered unit edges, the arcs they form on the cycle and the longest arc.  Plans: lesions_plan.h.
//
// gs_rim_classes, one launch.
//   rim_kernel   a workgroup per tile of 64 x 16 pixels, four pixels a thread.  Every thread tests its pixels (boundary_links.h's
//                boundary_pixel, from global memory); a tile without a boundary pixel writes its zeros and leaves.  Otherwise the
//                boundary pixels go into a list in LDS (an LDS counter hands out the places; the order does not matter, every
//                pixel's word is a function of the inputs alone), every other pixel gets its 0, and the workgroup stages the tile
//                with a halo of R = floor(sqrt(max_d2)) cells: the label and the class of every cell, label 0 outside the map, and
//                the OR of the class bits of all staged instance pixels.  Behind the one barrier a lane per listed pixel walks the
//                rows dy = -R..R of its disc; in a row it takes the cells |dx| <= floor(sqrt(max_d2 - dy^2)), a table of R + 1
//                words in LDS, ORs the class bit of every cell that carries the pixel's own label, and stops after a row once it
//                holds every bit that occurs in the staged cells.
// Exact: the disc is enumerated cell by cell; a cell outside the map holds label 0, which no instance has.  The search never
// leaves the staged cells: |dy| <= R and |dx| <= R.
//
// gs_loop_arcs, ten launches.  The unit edges of all loops lie one behind the other, loop by loop in walking order, in two arrays
// of the workspace: position e holds the mask word of the edge's pixel and the loop's number.
//   1 arc_fill_kernel      three launches: the edge arrays (word 0, loop -1), arcs and the wrap sums (0), the loops' bases (-1).
//   2 arc_segment_kernel   a lane per corner: its loop by bisection of loop_offsets (31 rounds at the most), the next corner on
//                          the cycle, and the length |dx| + |dy| of the segment between them, cut at `edges`; the lengths are
//                          summed per workgroup in 64 bits.
//   3 arc_scan_kernel      one workgroup of 1024: the sums become the edges in front of each workgroup (wave_block.h's scan, in
//                          64 bits: 2^31 corners of 2^31 edges each stay below 2^62).
//   4 arc_edges_kernel     per corner again: the segment's base = the workgroup's + the lengths in front of it in the workgroup.
//                          A loop's base is its first segment's.  A segment of 64 edges or more is written by the whole wave, a
//                          lane per unit edge and round (the lanes that hold one are taken in turn from a ballot); a shorter one by
//                          its own lane.  Every unit edge reads the mask at its pixel (the header's rule for its heading).
//   5 arc_last_kernel      a lane per position, every bit in turn: the wave's ballot of the uncovered lanes gives the wave's last
//                          uncovered position, the four waves' give the workgroup's: carry[bit][workgroup], -1 for none.
//   6 arc_carry_kernel     a workgroup of 1024 per bit: carry becomes the last uncovered position in front of each workgroup (an
//                          exclusive max-scan, the kernel boundary on either side as in every two-level scan here).
//   7 arc_runs_kernel      per position and bit: last = the last uncovered position at or in front of e (the lane's part of the
//                          ballot, else the waves in front, else carry), cut at the loop's base - 1.  Uncovered positions are their
//                          own index and indices grow along the array, so the plain max-scan cut at the base IS the scan segmented
//                          by loop.  A covered edge's run so far is e - last.  Per loop and bit, grouped per wave by loop
//                          (for_each_wave_group) and reduced by shuffles, then one atomic per group:
//                            covered  += the covered edges
//                            n_arcs   += the covered edges whose predecessor on the cycle is uncovered, and 1 from the loop's last
//                                        edge where no edge of the loop is uncovered
//                            longest   = max of the runs so far
//                            wrap     += the run that begins at the sequence's start (from the edge where it ends) and the run
//                                        that ends at the sequence's end (from the last edge), where the loop has an uncovered edge
//   8 arc_finish_kernel    per loop and bit: longest = max(longest, wrap): the two runs are one run on the cycle.
// Exact: sums and maxima of integers; with all edges covered the last edge's run so far is the loop, n_arcs is 1 and wrap 0; with
// none covered everything stays 0.
//
// Why the bytes do not depend on the run: near_classes, the edge arrays and the carries are pure functions of the inputs, written
// by one lane each; arcs and wrap are zeroed by launch 1 and then only added to or raised, with integers.
//
// Visibility.  Across launches the kernel boundary alone: what a launch stores plainly is read plainly only by later launches.
// arcs and wrap are touched in launch 7 only through agent-scope atomics.  LDS is written and read by one workgroup, on either
// side of a barrier that every thread of the workgroup reaches.
//
// Safety rule of gs_loop_arcs.  points, loop_offsets and loop_edges are device data.  For the contents gs_instance_outlines writes
// the results are as defined.  For any other contents the entry terminates, and reads and writes only inside its arrays and its
// workspace: a corner belongs to loop l only where 0 <= loop_offsets[l] <= corner < loop_offsets[l + 1] <= n_points, else its
// segment is empty; a length is cut at `edges` and a position at or beyond `edges` is not written; a pixel outside the map reads
// as mask 0; a segment that is not axis-parallel counts as |dx| + |dy| uncovered positions; a position is analysed only where its
// loop number lies in 0..n_loops - 1 and the position inside [base, base + loop_edges) inside [0, edges).
//
// Rules: those of wave_block.h.  The loops of this file's own --
//   the reach table      dx rises by one to R <= 32
//   staging, the list    c (k) rises by 256 until it passes the cells (the listed pixels)
//   the disc             dy rises from -R to R, dx from -span to span
//   the bisection        hi - lo falls to half, rounded up, every round: at most 31 rounds
//   the long segments    the ballot loses its lowest bit every round; t rises by 64 to the segment's length <= edges
//   a short segment      t rises by one to less than 64
//   the bits             b rises by one to bits <= 31
//   the scans            wave_block.h's: b rises by one over the thread's run of workgroups, d doubles up to 1024
//   the reductions       off halves from 32
#include "gs_internal.h"
#include "lesions_abi.h"
#include "lesions_plan.h"
#include "wave_block.h"
#include "boundary_links.h"

namespace gs {

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kThreads = kLesionThreads;
static_assert(kThreads == 256 && kRimTileW * kRimTileH == 4 * kThreads, "four waves a workgroup, four pixels a thread");
static_assert(kRimTileW == 64, "a tile pixel's index is row * 64 + column");

// ------------------------------------------------------------------------------------------------------------------- the rim
__global__ __launch_bounds__(kThreads) void rim_kernel(const int *__restrict__ L, const unsigned char *__restrict__ C, int n, int classes,
                                                       int H, int W, int max_d2, int reach, int tiles_x, int cw, int ch,
                                                       int *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) int s_rim[];        // int [ch * cw] labels, then unsigned char [ch * cw] classes
    __shared__ int s_span[kRimMaxReach + 1];
    __shared__ unsigned short s_list[kRimTileW * kRimTileH];
    __shared__ int s_count, s_all;
    const int tid = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int x0 = tx * kRimTileW, y0 = ty * kRimTileH;
    int *s_lab = s_rim;
    unsigned char *s_cls = reinterpret_cast<unsigned char *>(s_rim + cw * ch);
    if (tid == 0) {
        s_count = 0;
        s_all = 0;
    }
    if (tid <= reach) {                            // the half width of the disc's row |dy| = tid: tid <= R, so rem >= 0
        const int rem = max_d2 - tid * tid;
        int dx = 0;
        while (dx < reach && (dx + 1) * (dx + 1) <= rem)
            ++dx;
        s_span[tid] = dx;
    }
    bool rim[4], inside[4];
    int any = 0, id;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx = tid + kThreads * j, x = x0 + (idx & 63), y = y0 + (idx >> 6);
        inside[j] = x < W && y < H;
        rim[j] = inside[j] & boundary_pixel(L, n, H, W, y < H ? y : H - 1, x < W ? x : W - 1, id);
        any |= rim[j];
    }
    any = __syncthreads_or(any);                   // every thread of the workgroup; s_count and s_all are set behind it
    if (!any) {                                    // the whole workgroup
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (inside[j]) {
                const int idx = tid + kThreads * j;
                out[(size_t)(y0 + (idx >> 6)) * W + x0 + (idx & 63)] = 0;
            }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx = tid + kThreads * j;
        if (rim[j])
            s_list[atomicAdd(&s_count, 1)] = (unsigned short)idx;      // at most 1024 places are handed out
        else if (inside[j])
            out[(size_t)(y0 + (idx >> 6)) * W + x0 + (idx & 63)] = 0;
    }
    const int cells = cw * ch;
    int seen = 0;
    for (int c = tid; c < cells; c += kThreads) {
        const int cy = c / cw, cx = c - cy * cw, y = y0 - reach + cy, x = x0 - reach + cx;
        int lab = 0;
        unsigned char cl = 255;
        if (x >= 0 && y >= 0 && x < W && y < H) {
            lab = L[(size_t)y * W + x];
            cl = C[(size_t)y * W + x];
            if (lab >= 1 && lab <= n && cl < classes)
                seen |= 1 << cl;                   // classes <= 20
        }
        s_lab[c] = lab;
        s_cls[c] = cl;
    }
    if (seen)
        atomicOr(&s_all, seen);
    __syncthreads();
    const int count = s_count, all = s_all;
    for (int k = tid; k < count; k += kThreads) {
        const int idx = s_list[k], lx = idx & 63, ly = idx >> 6;
        const int a = s_lab[(ly + reach) * cw + lx + reach];           // a boundary pixel: 1 <= a <= n
        int acc = 0;
        for (int dy = -reach; dy <= reach; ++dy) {
            const int span = s_span[dy < 0 ? -dy : dy];                // <= R: the row stays inside the staged cells
            const int at = (ly + reach + dy) * cw + lx + reach;
            for (int dx = -span; dx <= span; ++dx)
                if (s_lab[at + dx] == a) {
                    const int cl = s_cls[at + dx];
                    if (cl < classes)
                        acc |= 1 << cl;
                }
            if (acc == all)                        // every bit that occurs in the staged cells
                break;
        }
        out[(size_t)(y0 + ly) * W + x0 + lx] = acc;
    }
}

// ------------------------------------------------------------------------------------------------------------------- the arcs
__global__ __launch_bounds__(kThreads) void arc_fill_kernel(int *a, int va, i64 na, int *b, int vb, i64 nb)
{
    const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
    if (i < na)
        a[i] = va;
    if (i < nb)
        b[i] = vb;
}

// before = the sum of v over the threads of the workgroup in front of this one, total = over all.  Every thread of the workgroup
// calls it, once per kernel.
__device__ inline void block_prefix64(i64 v, i64 &before, i64 &total)
{
    __shared__ i64 wave_sum[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    i64 inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const i64 o = __shfl_up(inc, off);
        if (lane >= off)
            inc += o;
    }
    if (lane == 63)
        wave_sum[wave] = inc;
    __syncthreads();
    i64 b = 0, t = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const i64 s = wave_sum[w];
        b += w < wave ? s : 0;
        t += s;
    }
    before = b + inc - v;
    total = t;
}

// 2 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void arc_segment_kernel(const int *__restrict__ loop_offsets, const int *__restrict__ points,
                                                               int n_loops, int n_points, int edges, int *__restrict__ seg_len,
                                                               int *__restrict__ seg_loop, i64 *__restrict__ seg_sum)
{
    const i64 c = (i64)blockIdx.x * kThreads + threadIdx.x;
    int len = 0, loop = -1;
    if (c < n_points) {
        int lo = 0, hi = n_loops;                  // the last l in [0, n_loops) with loop_offsets[l] <= c, or 0
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (loop_offsets[mid] <= c)
                lo = mid;
            else
                hi = mid;
        }
        const int first = loop_offsets[lo], end = loop_offsets[lo + 1];           // loop_offsets has n_loops + 1 words
        if (first >= 0 && first <= c && c < end && end <= n_points) {
            loop = lo;
            const i64 nx = c + 1 < end ? c + 1 : first;                           // in [0, n_points)
            const i64 dx = (i64)points[2 * nx] - points[2 * c], dy = (i64)points[2 * nx + 1] - points[2 * c + 1];
            const i64 l = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);              // < 2^33
            len = l > edges ? edges : (int)l;
        }
        seg_len[c] = len;
        seg_loop[c] = loop;
    }
    i64 before, total;
    block_prefix64(len, before, total);
    if (threadIdx.x == 0)
        seg_sum[blockIdx.x] = total;
}

// 3 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void arc_scan_kernel(i64 *__restrict__ seg_sum, int n_blocks)
{
    __shared__ i64 s[kScanThreads];
    const int t = (int)threadIdx.x, run = (n_blocks + kScanThreads - 1) / kScanThreads;
    const i64 lo = (i64)t * run, hi = lo + run < n_blocks ? lo + run : n_blocks;
    i64 sum = 0;
    for (i64 b = lo; b < hi; ++b)
        sum += seg_sum[b];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const i64 v = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    i64 base = s[t] - sum;
    for (i64 b = lo; b < hi; ++b) {
        const i64 c = seg_sum[b];
        seg_sum[b] = base;
        base += c;
    }
}

// 4 ------------------------------------------------------------------------------------------------------------------------
// the mask word at the pixel of the unit edge with start vertex (X, Y) and heading (dx, dy); 0 for a pixel outside the map and for
// a heading that is not one of the four
__device__ inline int edge_word(const int *__restrict__ mask, int H, int W, i64 X, i64 Y, int dx, int dy)
{
    i64 px, py;
    if (dx == 1 && dy == 0) {                      // east: the top side of (X, Y)
        px = X;
        py = Y;
    } else if (dx == 0 && dy == 1) {               // south: the right side of (X - 1, Y)
        px = X - 1;
        py = Y;
    } else if (dx == -1 && dy == 0) {              // west: the bottom side of (X - 1, Y - 1)
        px = X - 1;
        py = Y - 1;
    } else if (dx == 0 && dy == -1) {              // north: the left side of (X, Y - 1)
        px = X;
        py = Y - 1;
    } else
        return 0;
    if (px < 0 || py < 0 || px >= W || py >= H)
        return 0;
    return mask[(size_t)py * W + (size_t)px];
}

__global__ __launch_bounds__(kThreads) void arc_edges_kernel(const int *__restrict__ mask, int H, int W, const int *__restrict__ loop_offsets,
                                                             const int *__restrict__ points, int n_points, int edges,
                                                             const int *__restrict__ seg_len, const int *__restrict__ seg_loop,
                                                             const i64 *__restrict__ seg_sum, int *__restrict__ loop_base,
                                                             int *__restrict__ edge_mask, int *__restrict__ edge_loop)
{
    const int lane = threadIdx.x & 63;
    const i64 c = (i64)blockIdx.x * kThreads + threadIdx.x;
    int len = 0, loop = -1;
    if (c < n_points) {
        len = seg_len[c];
        loop = seg_loop[c];
    }
    i64 before, total;
    block_prefix64(len, before, total);
    const i64 base = seg_sum[blockIdx.x] + before;
    int x = 0, y = 0, dx = 0, dy = 0;
    if (loop >= 0) {                               // launch 2 found the corner inside its loop: first <= c < end <= n_points
        const int first = loop_offsets[loop], end = loop_offsets[loop + 1];
        const i64 nx = c + 1 < end ? c + 1 : first;
        x = points[2 * c];
        y = points[2 * c + 1];
        const i64 ddx = (i64)points[2 * nx] - x, ddy = (i64)points[2 * nx + 1] - y;
        dx = ddx > 0 ? 1 : ddx < 0 ? -1 : 0;
        dy = ddy > 0 ? 1 : ddy < 0 ? -1 : 0;
        if (c == first)
            loop_base[loop] = base < edges ? (int)base : edges;
    }
    const i64 room = base < edges ? edges - base : 0;                  // a position at or beyond `edges` is not written
    const int todo = loop >= 0 ? (len < room ? len : (int)room) : 0;
    // every lane of the wave gets here
    u64 rem = __ballot(todo >= 64);
    while (rem) {                                  // wave-uniform: the long segments in turn, the whole wave on each
        const int f = __ffsll((long long)rem) - 1;
        const int bx = __shfl(x, f), by = __shfl(y, f), bdx = __shfl(dx, f), bdy = __shfl(dy, f), bl = __shfl(loop, f), bt = __shfl(todo, f);
        const i64 bb = __shfl(base, f);
        for (i64 t = lane; t < bt; t += 64) {
            edge_mask[bb + t] = edge_word(mask, H, W, bx + t * bdx, by + t * bdy, bdx, bdy);
            edge_loop[bb + t] = bl;
        }
        rem &= rem - 1;
    }
    if (todo < 64)
        for (int t = 0; t < todo; ++t) {
            edge_mask[base + t] = edge_word(mask, H, W, (i64)x + t * dx, (i64)y + t * dy, dx, dy);
            edge_loop[base + t] = loop;
        }
}

// 5, 7 ---------------------------------------------------------------------------------------------------------------------
// the last position of the wave at which bit b of `word` is clear, -1 for none; u: the ballot of those lanes
__device__ inline int wave_last(int word, int b, i64 wave_base, u64 &u)
{
    u = __ballot(!(word >> b & 1));
    return u ? (int)(wave_base + 63 - __clzll((long long)u)) : -1;
}

__global__ __launch_bounds__(kThreads) void arc_last_kernel(const int *__restrict__ edge_mask, int edges, int bits, int edge_blocks,
                                                            int *__restrict__ carry)
{
    __shared__ int s_last[kArcMaxBits][kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 e = (i64)blockIdx.x * kThreads + threadIdx.x;
    const int word = e < edges ? edge_mask[e] : -1;                    // beyond the array: covered, never the last uncovered
    for (int b = 0; b < bits; ++b) {
        u64 u;
        const int last = wave_last(word, b, e - lane, u);
        if (lane == 0)
            s_last[b][wave] = last;
    }
    __syncthreads();
    if ((int)threadIdx.x < bits) {
        int m = -1;
        for (int w = 0; w < kThreads / 64; ++w)
            m = s_last[threadIdx.x][w] > m ? s_last[threadIdx.x][w] : m;
        carry[(size_t)threadIdx.x * edge_blocks + blockIdx.x] = m;
    }
}

// 6 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void arc_carry_kernel(int *__restrict__ carry, int edge_blocks)
{
    __shared__ int s[kScanThreads];
    int *__restrict__ row = carry + (size_t)blockIdx.x * edge_blocks;
    const int t = (int)threadIdx.x, run = (edge_blocks + kScanThreads - 1) / kScanThreads;
    const i64 lo = (i64)t * run, hi = lo + run < edge_blocks ? lo + run : edge_blocks;
    int m = -1;
    for (i64 b = lo; b < hi; ++b)
        m = row[b] > m ? row[b] : m;
    s[t] = m;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const int v = t >= d ? s[t - d] : -1;
        __syncthreads();
        s[t] = v > s[t] ? v : s[t];
        __syncthreads();
    }
    int base = t ? s[t - 1] : -1;                  // the threads in front: exclusive
    for (i64 b = lo; b < hi; ++b) {
        const int c = row[b];
        row[b] = base;
        base = c > base ? c : base;
    }
}

// 7 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void arc_runs_kernel(const int *__restrict__ edge_mask, const int *__restrict__ edge_loop,
                                                            const int *__restrict__ loop_edges, const int *__restrict__ loop_base,
                                                            const int *__restrict__ carry, int edges, int n_loops, int bits,
                                                            int edge_blocks, int *arcs, int *wrap)
{
    __shared__ int s_last[kArcMaxBits][kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 e = (i64)blockIdx.x * kThreads + threadIdx.x;
    const int word = e < edges ? edge_mask[e] : -1;
    bool ok = false;
    int loop = -1, B = 0, E = 0, t = 0, prev = 0, next = 0;
    if (e < edges) {
        loop = edge_loop[e];
        if (loop >= 0 && loop < n_loops) {
            B = loop_base[loop];
            E = loop_edges[loop];
            if (B >= 0 && E >= 1 && (i64)B + E <= edges && e >= B && e < (i64)B + E) {
                ok = true;
                t = (int)(e - B);
                prev = edge_mask[t ? e - 1 : (i64)B + E - 1];          // the predecessor on the cycle
                next = t + 1 < E ? edge_mask[e + 1] : 0;
            }
        }
    }
    for (int b = 0; b < bits; ++b) {
        u64 u;
        const int last = wave_last(word, b, e - lane, u);
        if (lane == 0)
            s_last[b][wave] = last;
    }
    __syncthreads();
    // every lane of the wave gets here
    for_each_wave_group(ok, loop, [&](int first, u64 group, bool mine) {
        for (int b = 0; b < bits; ++b) {           // wave-uniform
            u64 u;
            wave_last(word, b, e - lane, u);
            const u64 le = u & (~0ull >> (63 - lane));                 // the uncovered lanes at or in front of this one
            int last = le ? (int)(e - lane + 63 - __clzll((long long)le)) : -1;
            for (int w = 0; w < wave; ++w)         // positions grow with the wave: the maximum is the latest
                last = s_last[b][w] > last ? s_last[b][w] : last;
            const int c = carry[(size_t)b * edge_blocks + blockIdx.x];
            last = c > last ? c : last;
            last = last < B - 1 ? B - 1 : last;    // cut at the loop's base: nothing uncovered in this loop so far
            const bool cov = mine && (word >> b & 1);
            const bool whole = cov && t == E - 1 && last == B - 1;     // the last edge, and no edge of the loop is uncovered
            const bool start = cov && !(prev >> b & 1);
            const int head = cov && last == B - 1 && t + 1 < E && !(next >> b & 1) ? t + 1 : 0;
            const int tail = cov && t == E - 1 && last >= B ? (int)(e - last) : 0;
            int counts = (cov ? 1 : 0) | ((start || whole ? 1 : 0) << 16);        // two sums of at most 64
            int run = cov ? (int)(e - last) : 0;
            int ends = head + tail;                // both at most the loop's edges, and together: there is an uncovered one
#pragma unroll
            for (int off = 32; off; off >>= 1) {
                counts += __shfl_xor(counts, off);
                ends += __shfl_xor(ends, off);
                const int o = __shfl_xor(run, off);
                run = o > run ? o : run;
            }
            if (lane == first) {
                int *row = arcs + ((size_t)loop * bits + b) * 3;
                if (counts & 0xFFFF)
                    __hip_atomic_fetch_add(row, counts & 0xFFFF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (counts >> 16)
                    __hip_atomic_fetch_add(row + 1, counts >> 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (run)
                    __hip_atomic_fetch_max(row + 2, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (ends)
                    __hip_atomic_fetch_add(wrap + (size_t)loop * bits + b, ends, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    });
}

// 8 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void arc_finish_kernel(const int *__restrict__ wrap, i64 loop_bits, int *__restrict__ arcs)
{
    const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
    if (i >= loop_bits)
        return;
    const int w = wrap[i];
    if (w > arcs[3 * i + 2])
        arcs[3 * i + 2] = w;
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" gs_status gs_rim_classes(const int32_t *labels, const uint8_t *class_map, int n, int classes, int height, int width, int max_d2,
                                    int32_t *near_classes, void *hip_stream)
{
    RimPlan plan;
    const gs_status st = plan_rim(n, classes, height, width, max_d2, plan);
    if (st != GS_OK)
        return st;
    GS_REQUIRE(aligned(labels, 4), "gs_rim_classes: labels is NULL or not 4-byte aligned");
    GS_REQUIRE(class_map, "gs_rim_classes: class_map is NULL");
    GS_REQUIRE(aligned(near_classes, 4), "gs_rim_classes: near_classes is NULL or not 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(rim_kernel, dim3((unsigned)plan.blocks), dim3(kThreads), (size_t)plan.lds_bytes, s, labels, class_map, n, classes,
                       height, width, max_d2, plan.reach, plan.tiles_x, plan.cell_w, plan.cell_h, near_classes);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

extern "C" gs_status gs_loop_arcs_plan(long long edges, long long n_points, long long n_loops, int bits, size_t *workspace_bytes)
{
    GS_REQUIRE(workspace_bytes, "gs_loop_arcs_plan: null argument");
    ArcsPlan plan;
    const gs_status st = plan_arcs(edges, n_points, n_loops, bits, plan);
    *workspace_bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_loop_arcs(const int32_t *mask, int height, int width, int bits, const int32_t *loop_edges,
                                  const int32_t *loop_offsets, const int32_t *points, long long n_loops, long long n_points, long long edges,
                                  void *workspace, size_t workspace_bytes, int32_t *arcs, void *hip_stream)
{
    ArcsPlan plan;
    gs_status st = plan_arcs(edges, n_points, n_loops, bits, plan);
    if (st != GS_OK)
        return st;
    if ((st = check_lesion_map("gs_loop_arcs", height, width)) != GS_OK)
        return st;
    GS_REQUIRE(aligned(mask, 4), "gs_loop_arcs: mask is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(loop_edges, 4), "gs_loop_arcs: loop_edges is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(loop_offsets, 4), "gs_loop_arcs: loop_offsets is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(points, 4), "gs_loop_arcs: points is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 8), "gs_loop_arcs: workspace is NULL or not 8-byte aligned");
    GS_REQUIRE(aligned(arcs, 4), "gs_loop_arcs: arcs is NULL or not 4-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_loop_arcs: %lld edges, %lld points, %lld loops and %d bits need %zu bytes of workspace (got %zu)",
               edges, n_points, n_loops, bits, plan.bytes, workspace_bytes);
    if (n_loops == 0)
        return GS_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char *ws = static_cast<char *>(workspace);
    int *seg_len = reinterpret_cast<int *>(ws + plan.seg_len_off), *seg_loop = reinterpret_cast<int *>(ws + plan.seg_loop_off);
    i64 *seg_sum = reinterpret_cast<i64 *>(ws + plan.seg_sum_off);
    int *loop_base = reinterpret_cast<int *>(ws + plan.loop_base_off);
    int *edge_mask = reinterpret_cast<int *>(ws + plan.edge_mask_off), *edge_loop = reinterpret_cast<int *>(ws + plan.edge_loop_off);
    int *carry = reinterpret_cast<int *>(ws + plan.carry_off), *wrap = reinterpret_cast<int *>(ws + plan.wrap_off);
    const int loops = (int)n_loops, corners = (int)n_points, n_edges = (int)edges;          // the plan: all within an int
    const i64 loop_bits = (i64)loops * bits;
    const dim3 block(kThreads), scan(kScanThreads), edge_grid((unsigned)plan.edge_blocks), corner_grid((unsigned)plan.corner_blocks);
    const dim3 loop_grid((unsigned)((loops + kThreads - 1) / kThreads));
    const dim3 arcs_grid((unsigned)((3 * loop_bits + kThreads - 1) / kThreads));             // 3 * n_loops * bits < 2^36: blocks < 2^28

    hipLaunchKernelGGL(arc_fill_kernel, edge_grid, block, 0, s, edge_mask, 0, (i64)n_edges, edge_loop, -1, (i64)n_edges);
    hipLaunchKernelGGL(arc_fill_kernel, arcs_grid, block, 0, s, arcs, 0, 3 * loop_bits, wrap, 0, loop_bits);
    hipLaunchKernelGGL(arc_fill_kernel, loop_grid, block, 0, s, loop_base, -1, (i64)loops, loop_base, -1, (i64)0);
    hipLaunchKernelGGL(arc_segment_kernel, corner_grid, block, 0, s, loop_offsets, points, loops, corners, n_edges, seg_len, seg_loop, seg_sum);
    hipLaunchKernelGGL(arc_scan_kernel, dim3(1), scan, 0, s, seg_sum, plan.corner_blocks);
    hipLaunchKernelGGL(arc_edges_kernel, corner_grid, block, 0, s, mask, height, width, loop_offsets, points, corners, n_edges, seg_len,
                       seg_loop, seg_sum, loop_base, edge_mask, edge_loop);
    hipLaunchKernelGGL(arc_last_kernel, edge_grid, block, 0, s, edge_mask, n_edges, bits, plan.edge_blocks, carry);
    hipLaunchKernelGGL(arc_carry_kernel, dim3((unsigned)bits), scan, 0, s, carry, plan.edge_blocks);
    hipLaunchKernelGGL(arc_runs_kernel, edge_grid, block, 0, s, edge_mask, edge_loop, loop_edges, loop_base, carry, n_edges, loops,
                       bits, plan.edge_blocks, arcs, wrap);
    hipLaunchKernelGGL(arc_finish_kernel, dim3((unsigned)plan.loop_bit_blocks), block, 0, s, wrap, loop_bits, arcs);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
