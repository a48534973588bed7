// Per-glomerulus convex hulls (csrc/hulls_abi.h): for every instance of a label map the ring of its hull's vertices, twice the
// hull's area, the largest squared distance of two vertices and the narrowest caliper, all in integers.
//
// Only the two end pixels of a row of an instance can carry hull vertices, so the hull comes out of the row table without a sort
// and without a stack: lattice line Y has the points L(Y) and R(Y) (hulls_abi.h, "lines"), and a line is a vertex of the left
// (right) chain exactly when the steepest slope from the lines above it is strictly below the flattest slope to the lines below
// it (hull_slope_less of hulls_plan.h).  gs_instance_hulls keeps a head, one slot per valid box, the row table and a flag byte
// per lattice line in the caller's workspace (hulls_plan.h), in seven launches:
//   1 hull_scan_kernel     one workgroup of 1024, as morph_scan_kernel: thread t walks its run of boxes and sums, over the valid
//                          ones, their number, their heights and their tiles; the sums are scanned in LDS; the total of the
//                          heights is rows_needed and decides whether the table fits.  The second walk writes, for every
//                          instance, hull_offsets = the number of valid boxes in front of it (its slot, if its own box is valid)
//                          and the slot: instance, box, first row, first task, right = left = 0.  Thread 0 writes the head and
//                          rows_needed.  Where the table does not fit it writes every offset 0 and points_needed as the bound.
//   2 hull_clear_kernel    stats = -1; the rows of the table that are needed = (INT_MAX, -1).
//   3 hull_fill_kernel     a lane per pixel: a pixel of i inside i's box whose left (right) neighbour is not i, or lies outside
//                          the box, takes the row's atomic min (max).
//   4 hull_flag_kernel     a task is (slot, tile of 256 lattice lines); the task list is the scan of launch 1, decoded from the
//                          task's number.  The grid is persistent, every workgroup takes one contiguous share of the list.  A
//                          lane holds one line of the tile and sweeps all lines of the slot, staged through LDS in tiles: it keeps
//                          the steepest slope from above and the flattest to below, for L and for -R, and compares the two at
//                          the end.  The flag byte of every line of the slot is written (0 for a line that does not exist); the
//                          vertices of a wave are counted by ballot and added to the slot's right / left.
//   5 hull_offsets_kernel  one workgroup of 1024: the slots' right + left are scanned into their bases; the total is
//                          points_needed and decides whether the points fit.  Then hull_offsets[b] = the base of the slot it
//                          named (the total for b == n and behind the last slot), or 0 throughout where the points do not fit.
//   6 hull_place_kernel    a wave per slot walks its flag bytes 64 at a time; ballots give a vertex its rank in its chain: right
//                          vertices go to 1 + rank, left vertices to 0 (rank 0, the start) or k - rank.
//   7 hull_measure_kernel  a wave per slot, a lane per edge e: it sweeps the ring's vertices for w, the largest squared distance
//                          from its start vertex and its shoelace term; the lane keeps its narrowest edge (hull_ratio_less of
//                          hulls_plan.h, the lowest e among equals), the wave reduces by shuffles and lane 0 writes the row.
// With n == 0 launch 1 alone runs.  Where the table or the points do not fit the head says so: the later launches touch no table,
// no slot, no point and no stats row, which launch 2 has set to -1 throughout.
//
// Deviations from the launches first suggested for this entry: L(Y) and R(Y) are not stored -- line_ends forms them from the two
// adjacent rows of the table wherever they are needed, which saves a launch and eight bytes a line; the vertices are counted
// per slot by the vertex pass itself (integer atomic adds) and the scan runs over slots, not over blocks of flags, so launch 6
// needs no block ranks; and launch 7 is a wave per instance at every k: a convex lattice polygon within 32768 x 32768 has a few
// thousand vertices at the most (its edges are distinct primitive vectors), far from where a workgroup would pay.
//
// hull_offsets between the launches.  The plan does not know n, so the workspace has no per-instance array: the instance -> slot
// index of launch 3 is the caller's hull_offsets itself, written by launch 1, read plainly by launch 3, and overwritten by
// launch 5.  An instance with an invalid box names the slot of the next valid box, whose `inst` is not its own: launch 3 tests that.
//
// Why the result is exact: the table's row ends are the smallest and the largest x of the instance's pixels of that row inside
// the box (morphometry.hip's argument); the hull of a set of unit squares is the hull of their corners, and a corner strictly
// between L(Y) and R(Y) on its line, or on a line's end that the slope rule drops, lies on a segment between two kept points or
// inside; every comparison is between integers that fit their type (hulls_plan.h).
//
// Why the bytes do not depend on the run: the slots' plain fields, the head and the offsets are pure functions of the boxes and
// the flags, each written by one thread; the flags, the points and the stats rows have one writer per element; the table is
// written with integer min and max, right and left with integer add, which commute.
//
// Visibility.  Per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores.  Across
// launches visibility comes from the kernel boundary alone: what a launch stores plainly is read plainly only by later launches.
// Inside launch 3 the table, inside launch 4 right and left are touched only through agent-scope atomics, which execute at the
// memory side, and no lane reads them there.  Launch 5 is one workgroup: the bases its threads store are read by other threads
// of the same workgroup behind its barrier.
//
// Rules: those of wave_block.h.  The loops of this file's own --
//   a walk of launch 1 / 5  b rises by one from lo to hi <= n (n_slots)
//   the LDS scans           d doubles up to 1024; every thread takes every barrier
//   grid-stride loops       (launches 2, 6 and 7) the index rises by the grid's threads (waves) until it passes the count; in 6
//                           and 7 the index is the same in every lane of a wave, so ballots and shuffles inside are whole
//   the task share          t rises by one from the share's first task to its last; the share's bounds are the same in every
//                           thread of the workgroup, so the barriers inside are reached by all of them
//   the slot search         hi - v halves; the slot walk v rises by one and stops below n_slots
//   the tile loop           b rises by one to the slot's tiles, the same in every thread; the sweep j rises by one to the lines
//                           of tile b, at most 256
//   the chunk loops         (launches 6 and 7) c rises by 64 to the slot's lines / vertices; the vertex sweep j rises by one to k
// An id is used as an index only after its range test, a slot number only below n_slots, a row only inside its slot's box: rows
// row_off .. row_off + height of a slot lie below rows_needed <= rows_cap, its lines row_off + v .. row_off + v + height below
// rows_needed + n_slots <= 2 * rows_cap.  A ring index is used only below k, and base + k <= points_needed <= points_cap.
#include "gs_internal.h"
#include "hulls_plan.h"
#include "wave_block.h"
#include "hulls_abi.h"

#include <climits>

namespace gs {

namespace {

typedef unsigned long long u64;

constexpr int kThreads = kHullThreads;
static_assert(kThreads == 256 && kHullTile == kThreads, "a tile is one lattice line per thread of four waves");

__device__ inline bool box_valid(int x0, int y0, int x1, int y1, int H, int W)
{
    return x0 >= 0 && y0 >= 0 && x1 <= W && y1 <= H && x0 < x1 && y0 < y1;
}

// L and R of lattice line j (0 <= j <= height) of a slot whose rows begin at row_off: from rows j - 1 and j.  R < 0: the line
// does not exist.
__device__ inline void line_ends(const int *__restrict__ table, long long row_off, int height, int j, int &L, int &R)
{
    int lo = INT_MAX, hi = -1;
    if (j >= 1) {
        const int *row = table + 2 * (row_off + j - 1);
        lo = row[0], hi = row[1];
    }
    if (j < height) {
        const int *row = table + 2 * (row_off + j);
        lo = row[0] < lo ? row[0] : lo;
        hi = row[1] > hi ? row[1] : hi;
    }
    L = lo;
    R = hi >= 0 ? hi + 1 : -1;
}

// 1 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void hull_scan_kernel(const int *__restrict__ boxes, int n, int H, int W, long long rows_cap,
                                                                  HullHead *__restrict__ head, HullSlot *__restrict__ slots,
                                                                  int *__restrict__ hull_offsets, long long *__restrict__ counts)
{
    __shared__ long long s_rows[kScanThreads], s_tasks[kScanThreads];
    __shared__ int s_cnt[kScanThreads];
    const int t = (int)threadIdx.x;
    const long long run = ((long long)n + kScanThreads - 1) / kScanThreads, lo = t * run, hi = lo + run < n ? lo + run : n;
    long long rows = 0, tasks = 0;
    int cnt = 0;
    for (long long b = lo; b < hi; ++b) {
        const int x0 = boxes[4 * b], y0 = boxes[4 * b + 1], x1 = boxes[4 * b + 2], y1 = boxes[4 * b + 3];
        if (box_valid(x0, y0, x1, y1, H, W)) {
            ++cnt;
            rows += y1 - y0;
            tasks += hull_tiles(y1 - y0);
        }
    }
    s_rows[t] = rows;
    s_tasks[t] = tasks;
    s_cnt[t] = cnt;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const long long vr = t >= d ? s_rows[t - d] : 0, vt = t >= d ? s_tasks[t - d] : 0;
        const int vc = t >= d ? s_cnt[t - d] : 0;
        __syncthreads();
        s_rows[t] += vr;
        s_tasks[t] += vt;
        s_cnt[t] += vc;
        __syncthreads();
    }
    const long long total_rows = s_rows[kScanThreads - 1];
    const bool fits = total_rows <= rows_cap;
    long long row_off = s_rows[t] - rows, task_off = s_tasks[t] - tasks;
    int v = s_cnt[t] - cnt;
    for (long long b = lo; b < hi; ++b) {
        const int x0 = boxes[4 * b], y0 = boxes[4 * b + 1], x1 = boxes[4 * b + 2], y1 = boxes[4 * b + 3];
        const bool valid = box_valid(x0, y0, x1, y1, H, W);
        hull_offsets[b] = fits ? v : 0;
        if (valid && fits) {                       // v < the valid boxes <= total_rows <= rows_cap: inside the slots
            HullSlot s;
            s.row_off = row_off;
            s.task_off = task_off;
            s.base = 0;
            s.inst = (int)b + 1;
            s.x0 = x0, s.y0 = y0, s.x1 = x1, s.y1 = y1;
            s.right = s.left = 0;
            s.pad[0] = s.pad[1] = s.pad[2] = 0;
            slots[v] = s;
        }
        if (valid) {
            ++v;
            row_off += y1 - y0;
            task_off += hull_tiles(y1 - y0);
        }
    }
    if (t == 0) {
        head->rows_needed = total_rows;
        head->n_tasks = fits ? s_tasks[kScanThreads - 1] : 0;
        head->n_slots = fits ? s_cnt[kScanThreads - 1] : 0;
        head->fits = fits ? 1 : 0;
        counts[0] = total_rows;
        if (!fits || n == 0) {                     // no later launch writes these two
            counts[1] = 2 * (total_rows + s_cnt[kScanThreads - 1]);
            hull_offsets[n] = 0;
        }
    }
}

// 2 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void hull_clear_kernel(long long *__restrict__ stats, long long words, const HullHead *__restrict__ head,
                                                              int *__restrict__ table)
{
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x, step = (long long)gridDim.x * kThreads;
    for (long long i = gid; i < words; i += step)
        stats[i] = -1;
    const long long rows = head->fits ? head->rows_needed : 0;
    for (long long r = gid; r < rows; r += step) {
        table[2 * r] = INT_MAX;
        table[2 * r + 1] = -1;
    }
}

// 3 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void hull_fill_kernel(const int *__restrict__ L, int n, int H, int W, const HullHead *__restrict__ head,
                                                             const HullSlot *__restrict__ slots, const int *__restrict__ slot_of, int *table)
{
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= (long long)H * W)
        return;
    const int own = L[p];
    const int n_slots = head->n_slots;             // 0 where the table does not fit
    if (own < 1 || own > n)
        return;
    const int v = slot_of[own - 1];                // the valid boxes in front of `own`: its slot exactly where its own box is valid
    if (v < 0 || v >= n_slots)
        return;
    const HullSlot *s = slots + v;
    if (s->inst != own)
        return;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const int x0 = s->x0, y0 = s->y0, x1 = s->x1, y1 = s->y1;         // within the map
    if (x < x0 || x >= x1 || y < y0 || y >= y1)
        return;
    const bool left_end = x == x0 || L[p - 1] != own, right_end = x == x1 - 1 || L[p + 1] != own;     // x > x0 >= 0; x + 1 < x1 <= W
    int *row = table + 2 * (s->row_off + (y - y0));                   // a row of the slot: below rows_needed
    if (left_end)
        __hip_atomic_fetch_min(row, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (right_end)
        __hip_atomic_fetch_max(row + 1, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 4 ------------------------------------------------------------------------------------------------------------------------
// The steepest slope from above (a maximum) or the flattest to below (a minimum) met so far, as a fraction num / den with
// den > 0; den == 0: none yet.
struct HullSlope {
    int num = 0, den = 0;
};

__device__ inline void keep_steepest(HullSlope &s, int num, int den)
{
    if (s.den == 0 || hull_slope_less(s.num, s.den, num, den))
        s.num = num, s.den = den;
}

__device__ inline void keep_flattest(HullSlope &s, int num, int den)
{
    if (s.den == 0 || hull_slope_less(num, den, s.num, s.den))
        s.num = num, s.den = den;
}

// a side without lines counts as satisfied
__device__ inline bool strict_vertex(const HullSlope &above, const HullSlope &below)
{
    return above.den == 0 || below.den == 0 || hull_slope_less(above.num, above.den, below.num, below.den);
}

__global__ __launch_bounds__(kThreads) void hull_flag_kernel(const HullHead *__restrict__ head, HullSlot *slots, const int *__restrict__ table,
                                                             unsigned char *__restrict__ flags)
{
    __shared__ int tile_l[kHullTile], tile_r[kHullTile];
    const long long n_tasks = head->n_tasks;
    const int n_slots = head->n_slots;
    const long long share = (n_tasks + gridDim.x - 1) / gridDim.x;
    const long long t0 = (long long)blockIdx.x * share, t1 = t0 + share < n_tasks ? t0 + share : n_tasks;
    if (t0 >= t1)                                  // the whole workgroup
        return;
    // the last slot whose first task is at most t0: slot 0 starts at task 0
    int v = 0;
    for (int hi = n_slots; hi - v > 1;) {
        const int mid = v + (hi - v) / 2;
        if (slots[mid].task_off <= t0)
            v = mid;
        else
            hi = mid;
    }
    for (long long t = t0; t < t1; ++t) {
        while (v + 1 < n_slots && slots[v + 1].task_off <= t)
            ++v;
        const long long row_off = slots[v].row_off;                   // (field by field: right and left are left to the atomics)
        const int height = slots[v].y1 - slots[v].y0, lines = height + 1;
        const int tiles = (int)hull_tiles(height);
        const long long k = t - slots[v].task_off;                    // 0 <= k < tiles
        const int a = (int)(k < tiles ? k : tiles - 1);
        const int i = a * kHullTile + (int)threadIdx.x;
        const bool mine = i < lines;
        int Li = 0, Ri = -1;
        if (mine)
            line_ends(table, row_off, height, i, Li, Ri);
        HullSlope l_above, l_below, r_above, r_below;                 // of L and of -R
        for (int b = 0; b < tiles; ++b) {
            const int j0 = b * kHullTile, rest = lines - j0, nb = rest < kHullTile ? rest : kHullTile;       // >= 1
            __syncthreads();                       // the tile before is read to the end
            int Lj = INT_MAX, Rj = -1;
            if ((int)threadIdx.x < nb)
                line_ends(table, row_off, height, j0 + (int)threadIdx.x, Lj, Rj);
            tile_l[threadIdx.x] = Lj;
            tile_r[threadIdx.x] = Rj;
            __syncthreads();
            if (Ri >= 0) {
                for (int jj = 0; jj < nb; ++jj) {
                    const int l = tile_l[jj], r = tile_r[jj], j = j0 + jj;               // every lane the same word: a broadcast
                    if (r < 0 || j == i)
                        continue;
                    if (j < i) {
                        keep_steepest(l_above, Li - l, i - j);
                        keep_steepest(r_above, r - Ri, i - j);
                    } else {
                        keep_flattest(l_below, l - Li, j - i);
                        keep_flattest(r_below, Ri - r, j - i);
                    }
                }
            }
        }
        const bool right = Ri >= 0 && strict_vertex(r_above, r_below), left = Ri >= 0 && strict_vertex(l_above, l_below);
        if (mine)
            flags[row_off + v + i] = (unsigned char)((right ? 1 : 0) | (left ? 2 : 0));   // line row_off + v + i: below 2 * rows_cap
        const int n_right = __popcll(__ballot(right)), n_left = __popcll(__ballot(left));
        if ((threadIdx.x & 63) == 0) {
            if (n_right)
                __hip_atomic_fetch_add(&slots[v].right, n_right, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (n_left)
                __hip_atomic_fetch_add(&slots[v].left, n_left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// 5 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void hull_offsets_kernel(HullHead *head, HullSlot *slots, int n, long long points_cap,
                                                                     int *hull_offsets, long long *__restrict__ counts)
{
    __shared__ long long s_k[kScanThreads];
    if (!head->fits)                               // the whole workgroup: launch 1 has written the offsets and the bound
        return;
    const int t = (int)threadIdx.x, n_slots = head->n_slots;
    const long long run = ((long long)n_slots + kScanThreads - 1) / kScanThreads, lo = t * run, hi = lo + run < n_slots ? lo + run : n_slots;
    long long sum = 0;
    for (long long v = lo; v < hi; ++v)
        sum += slots[v].right + slots[v].left;
    s_k[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const long long vk = t >= d ? s_k[t - d] : 0;
        __syncthreads();
        s_k[t] += vk;
        __syncthreads();
    }
    const long long total = s_k[kScanThreads - 1];
    const bool ok = total <= points_cap;           // <= 2^31 - 1
    long long base = s_k[t] - sum;
    for (long long v = lo; v < hi; ++v) {
        slots[v].base = base;
        base += slots[v].right + slots[v].left;
    }
    __syncthreads();                               // the bases, stored by other threads of this workgroup, are read below
    for (long long b = t; b <= n; b += kScanThreads) {
        long long off = 0;
        if (ok) {
            const int v = b < n ? hull_offsets[b] : n_slots;          // launch 1's: the valid boxes in front of b
            off = v >= 0 && v < n_slots ? slots[v].base : total;
        }
        hull_offsets[b] = (int)off;
    }
    if (t == 0) {
        counts[1] = total;
        if (!ok)
            head->fits = 0;                        // read by every thread in front of the scan's barriers
    }
}

// 6 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void hull_place_kernel(const HullHead *__restrict__ head, const HullSlot *__restrict__ slots,
                                                              const int *__restrict__ table, const unsigned char *__restrict__ flags,
                                                              int *__restrict__ points)
{
    if (!head->fits)
        return;
    const int lane = threadIdx.x & 63, n_slots = head->n_slots;
    const long long wave = ((long long)blockIdx.x * kThreads + threadIdx.x) >> 6, waves = (long long)gridDim.x * (kThreads / 64);
    const u64 below = (1ull << lane) - 1;
    for (long long v = wave; v < n_slots; v += waves) {               // the same v in every lane of the wave
        const HullSlot *s = slots + v;
        const long long row_off = s->row_off, base = s->base;
        const int height = s->y1 - s->y0, lines = height + 1, y0 = s->y0, k = s->right + s->left;
        int seen_r = 0, seen_l = 0;
        for (int c = 0; c < lines; c += 64) {
            const int i = c + lane;
            const int f = i < lines ? flags[row_off + v + i] : 0;
            const u64 m_r = __ballot(f & 1), m_l = __ballot(f & 2);
            if (f) {
                int Li, Ri;
                line_ends(table, row_off, height, i, Li, Ri);
                if (f & 1) {
                    const int at = 1 + seen_r + __popcll(m_r & below);
                    if (at < k) {
                        points[2 * (base + at)] = Ri;
                        points[2 * (base + at) + 1] = y0 + i;
                    }
                }
                if (f & 2) {
                    const int rank = seen_l + __popcll(m_l & below), at = rank ? k - rank : 0;
                    if (at >= 0 && at < k) {
                        points[2 * (base + at)] = Li;
                        points[2 * (base + at) + 1] = y0 + i;
                    }
                }
            }
            seen_r += __popcll(m_r);
            seen_l += __popcll(m_l);
        }
    }
}

// 7 ------------------------------------------------------------------------------------------------------------------------
// a before b: the narrower caliper, the lower edge among equals; e < 0: none
__device__ inline bool narrower(u64 wa, u64 la, int ea, u64 wb, u64 lb, int eb)
{
    if (ea < 0 || eb < 0)
        return eb < 0 && ea >= 0;
    if (hull_ratio_less(wa, la, wb, lb))
        return true;
    return !hull_ratio_less(wb, lb, wa, la) && ea < eb;
}

__global__ __launch_bounds__(kThreads) void hull_measure_kernel(const HullHead *__restrict__ head, const HullSlot *__restrict__ slots, int n,
                                                                const int *__restrict__ points, long long *__restrict__ stats)
{
    if (!head->fits)
        return;
    const int lane = threadIdx.x & 63, n_slots = head->n_slots;
    const long long wave = ((long long)blockIdx.x * kThreads + threadIdx.x) >> 6, waves = (long long)gridDim.x * (kThreads / 64);
    for (long long v = wave; v < n_slots; v += waves) {               // the same v in every lane of the wave
        const HullSlot *s = slots + v;
        const int k = s->right + s->left, inst = s->inst;
        const int *P = points + 2 * s->base;       // the ring: k points
        u64 best_w = 0, best_l = 0, far = 0;
        int best_e = -1;
        long long area2 = 0;
        for (int c = 0; c < k; c += 64) {
            const int e = c + lane;
            if (e < k) {
                const int e1 = e + 1 < k ? e + 1 : 0;
                const long long ax = P[2 * e], ay = P[2 * e + 1], bx = P[2 * e1], by = P[2 * e1 + 1];
                const long long ex = bx - ax, ey = by - ay;
                area2 += ax * by - bx * ay;
                long long w = 0;
                for (int j = 0; j < k; ++j) {
                    const long long vx = P[2 * j] - ax, vy = P[2 * j + 1] - ay;
                    long long cr = ex * vy - ey * vx;                 // |cr| <= 2^31
                    cr = cr < 0 ? -cr : cr;
                    w = cr > w ? cr : w;
                    const u64 d = (u64)(vx * vx + vy * vy);
                    far = d > far ? d : far;
                }
                const u64 len2 = (u64)(ex * ex + ey * ey);
                if (narrower((u64)w, len2, e, best_w, best_l, best_e))
                    best_w = (u64)w, best_l = len2, best_e = e;
            }
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const u64 ow = __shfl_xor(best_w, off), ol = __shfl_xor(best_l, off), of = __shfl_xor(far, off);
            const int oe = __shfl_xor(best_e, off);
            area2 += __shfl_xor(area2, off);
            far = of > far ? of : far;
            if (narrower(ow, ol, oe, best_w, best_l, best_e))
                best_w = ow, best_l = ol, best_e = oe;
        }
        if (lane == 0 && inst >= 1 && inst <= n) {
            long long *row = stats + 6 * (size_t)(inst - 1);
            row[0] = k;
            row[1] = area2;
            row[2] = (long long)far;
            row[3] = (long long)best_w;
            row[4] = (long long)best_l;
            row[5] = k ? best_e : 0;
        }
    }
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" gs_status gs_hulls_plan(int height, int width, long long rows_cap, size_t *workspace_bytes)
{
    GS_REQUIRE(workspace_bytes, "gs_hulls_plan: null argument");
    HullsPlan plan;
    const gs_status st = plan_hulls(height, width, rows_cap, plan);
    *workspace_bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_instance_hulls(const int32_t *labels, const int32_t *boxes, int n, int height, int width, void *workspace,
                                       size_t workspace_bytes, long long rows_cap, int32_t *hull_offsets, int32_t *points,
                                       long long points_cap, long long *stats, long long *counts, void *hip_stream)
{
    HullsPlan plan;
    gs_status st = plan_hulls(height, width, rows_cap, plan);
    if (st != GS_OK || (st = check_hull_points_cap(points_cap)) != GS_OK)
        return st;
    GS_REQUIRE(n >= 0, "gs_instance_hulls: n must not be negative (got %d)", n);
    GS_REQUIRE(aligned(labels, 4), "gs_instance_hulls: labels is NULL or not 4-byte aligned");
    GS_REQUIRE(n == 0 || aligned(boxes, 4), "gs_instance_hulls: boxes is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 8), "gs_instance_hulls: workspace is NULL or not 8-byte aligned");
    GS_REQUIRE(aligned(hull_offsets, 4), "gs_instance_hulls: hull_offsets is NULL or not 4-byte aligned");
    GS_REQUIRE(n == 0 || points_cap == 0 || aligned(points, 4), "gs_instance_hulls: points is NULL or not 4-byte aligned");
    GS_REQUIRE(n == 0 || aligned(stats, 8), "gs_instance_hulls: stats is NULL or not 8-byte aligned");
    GS_REQUIRE(aligned(counts, 8), "gs_instance_hulls: counts is NULL or not 8-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_instance_hulls: rows_cap %lld needs %zu bytes of workspace (got %zu)", rows_cap, plan.bytes,
               workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char *ws = static_cast<char *>(workspace);
    HullHead *head = reinterpret_cast<HullHead *>(ws + plan.head_off);
    HullSlot *slots = reinterpret_cast<HullSlot *>(ws + plan.slot_off);
    int *table = reinterpret_cast<int *>(ws + plan.rows_off);
    unsigned char *flags = reinterpret_cast<unsigned char *>(ws + plan.flags_off);

    hipLaunchKernelGGL(hull_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, boxes, n, height, width, plan.rows_cap, head, slots, hull_offsets,
                       counts);
    if (n > 0) {
        const long long words = 6ll * n, most = words > plan.rows_cap ? words : plan.rows_cap;
        const long long clear_blocks = (most - 1) / kThreads + 1;
        const unsigned stride = (unsigned)plan.stride_blocks;
        hipLaunchKernelGGL(hull_clear_kernel, dim3((unsigned)(clear_blocks < kHullMaxGrid ? clear_blocks : kHullMaxGrid)), dim3(kThreads), 0, s,
                           stats, words, head, table);
        hipLaunchKernelGGL(hull_fill_kernel, dim3((unsigned)plan.pixel_blocks), dim3(kThreads), 0, s, labels, n, height, width, head, slots,
                           hull_offsets, table);
        hipLaunchKernelGGL(hull_flag_kernel, dim3(stride), dim3(kThreads), 0, s, head, slots, table, flags);
        hipLaunchKernelGGL(hull_offsets_kernel, dim3(1), dim3(kScanThreads), 0, s, head, slots, n, points_cap, hull_offsets, counts);
        hipLaunchKernelGGL(hull_place_kernel, dim3(stride), dim3(kThreads), 0, s, head, slots, table, flags, points);
        hipLaunchKernelGGL(hull_measure_kernel, dim3(stride), dim3(kThreads), 0, s, head, slots, n, points, stats);
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
}
