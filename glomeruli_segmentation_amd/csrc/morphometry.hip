// Per-glomerulus morphometry (include/glomseg_morphometry.h): for every instance of a label map ten exact integer sums -- pixels,
// first and second moments, Gray's bit-quad counts -- and the squared maximum Feret diameter.
//
// gs_instance_morphometry keeps a head, one slot per valid box and a row table in the caller's workspace (morphometry_plan.h), in
// five launches:
//   1 morph_scan_kernel    one workgroup of 1024: thread t walks its run of boxes and sums, over the valid ones, their number,
//                          their heights and their Feret tasks; the 1024 sums are scanned in LDS (wave_block.h's Hillis-Steele,
//                          on three sums at once: that one scans an int array in place, and this entry has no per-instance
//                          array to scan); the total of the heights is rows_needed and decides whether the table fits.  The
//                          second walk writes, for every instance, feret2 = its slot (valid box, table fits) or -1, and the slot:
//                          instance, box, first row, first task, best = 0.  Thread 0 writes the head and rows_needed.
//   2 morph_clear_kernel   stats = 0; the rows of the table that are needed = (INT_MAX, -1).
//   3 morph_map_kernel     one lane per bit-quad window, whose lower-right pixel (x, y) is the lane's own pixel; a workgroup takes
//                          256 columns and a lane walks kMorphRows windows down its column, so the upper two pixels of a window
//                          are the lower two of the one before: three loads a window (left, own, right neighbour).  Of the at
//                          most four distinct instances of a window, what belongs to the first instance the lane has met stays
//                          in its registers; for each other one the lanes of the wave that hold it are grouped
//                          (for_each_wave_group), the ten sums are reduced in the group -- the five counts by ballot, the five
//                          coordinate sums by shuffles -- and the group's first lane adds what is not zero to stats.  After the
//                          last row the kept sums go the same way, grouped by kept instance: inside a large instance that is ten
//                          atomics per wave and sixteen rows.  A pixel inside its instance's box whose left (right)
//                          neighbour is another instance or lies outside the box takes the row's min (max) in the table.
//   4 morph_feret_kernel   the farthest pair of a point set lies among its convex-hull vertices, and a pixel with pixels of its
//                          instance on both sides in its row is none: the candidates are the two ends of every row of the
//                          table, 2 * height per instance, in tiles of 256.  A task is (slot, tile a, tile b >= a); the task
//                          list is the scan of launch 1 (task_off per slot), built on the device, and a task's slot and tiles
//                          are decoded from its number.  The grid is persistent, its size is the plan's, every workgroup takes
//                          one contiguous share of the list.  Both tiles are staged in LDS; a lane holds one candidate of a and
//                          sweeps b; a wave max, then one atomic max on the slot's best.
//   5 morph_finish_kernel  feret2[inst - 1] = best, per slot.
// With n == 0 launch 1 alone runs (rows_needed = 0).  Where the table does not fit the head says so: launches 3..5 touch no
// table, no slot and no feret2, which launch 1 has set to -1 throughout.
//
// feret2 between the launches.  The plan does not know n, so the workspace has no per-instance array: the instance -> slot index
// of launch 3 is the caller's feret2 itself, written by launch 1, read plainly by launch 3, and overwritten for every valid box by
// launch 5.  Launch 4 never touches it.  An invalid box keeps launch 1's -1.
//
// Why the result is exact: stats is sums of integers below 2^61; the table's row ends are exactly the smallest and the largest x
// of the instance's pixels of that row inside the box -- the smallest such pixel has no pixel of the instance inside the box to
// its left, so it passes the test, and min / max over a superset that contains the extreme is the extreme; every pair of
// candidates of an instance meets in exactly the tasks (a, b) and, for a == b, in both orders.
//
// Why the bytes do not depend on the run: feret2's slot numbers, the slots and the head are pure functions of the boxes, each
// written by one thread.  stats, the table and best are written with integer add, min and max only, which commute: the bytes do
// not depend on the order in which waves arrive, nor on how a wave's lanes happen to be grouped.
//
// Visibility.  Per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores.  Across
// launches visibility comes from the kernel boundary alone: what a launch stores plainly is read plainly only by later launches.
// Inside launch 3 stats and the table, inside launch 4 best are touched only through agent-scope atomics, which execute at the
// memory side: no lane reads stats at all, the table is read first in launch 4 and best in launch 5.
//
// Rules: those of wave_block.h, whose grouping loop ends launch 3.  The loops of this file's own --
//   a walk of launch 1    b rises by one from lo to hi <= n
//   the LDS scan          d doubles up to 1024; every thread takes every barrier
//   grid-stride loops     (launches 2 and 5) the index rises by the grid's threads until it passes the count
//   the column walk       y rises by one over the workgroup's kMorphRows rows, the same in every lane
//   the task share        t rises by one from the share's first task to its last; the share's bounds are the same in every thread
//                         of the workgroup, so the barriers inside are reached by all of them
//   the slot search       hi - v halves; the slot walk v rises by one and stops below n_slots
//   the tile decode       a rises by one while k >= tiles - a: at most `tiles` <= 256 rounds
//   the sweep             j rises by one to the candidates of tile b, at most 256
// An id is used as an index only after its range test, a slot number only below n_slots, a row only inside its slot's box: rows
// row_off .. row_off + height of a slot lie below rows_needed <= rows_cap.  The box of launch 3 is read from `boxes` at an id in
// range and compared, never indexed through.
#include "gs_internal.h"
#include "morphometry_plan.h"
#include "wave_block.h"
#include "../../include/glomseg_morphometry.h"

#include <climits>

namespace gs {

namespace {

typedef unsigned long long u64;

constexpr int kThreads = kMorphThreads;
static_assert(kThreads == 256 && kMorphTile == kThreads, "a tile is one candidate per thread of four waves");

__device__ inline bool box_valid(int x0, int y0, int x1, int y1, int H, int W)
{
    return x0 >= 0 && y0 >= 0 && x1 <= W && y1 <= H && x0 < x1 && y0 < y1;
}

// 1 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void morph_scan_kernel(const int *__restrict__ boxes, int n, int H, int W, long long rows_cap,
                                                                   MorphHead *__restrict__ head, MorphSlot *__restrict__ slots,
                                                                   int *__restrict__ feret2, long long *__restrict__ rows_needed)
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
            tasks += morph_tasks(y1 - y0);
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
        feret2[b] = valid && fits ? v : -1;
        if (valid && fits) {                       // v < the valid boxes <= total_rows <= rows_cap: inside the slots
            MorphSlot s;
            s.row_off = row_off;
            s.task_off = task_off;
            s.inst = (int)b + 1;
            s.x0 = x0, s.y0 = y0, s.x1 = x1, s.y1 = y1;
            s.best = 0;
            s.pad[0] = s.pad[1] = 0;
            slots[v] = s;
        }
        if (valid) {
            ++v;
            row_off += y1 - y0;
            task_off += morph_tasks(y1 - y0);
        }
    }
    if (t == 0) {
        head->rows_needed = total_rows;
        head->n_tasks = fits ? s_tasks[kScanThreads - 1] : 0;
        head->n_slots = fits ? s_cnt[kScanThreads - 1] : 0;
        head->fits = fits ? 1 : 0;
        rows_needed[0] = total_rows;
    }
}

// 2 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void morph_clear_kernel(u64 *__restrict__ stats, long long words, const MorphHead *__restrict__ head,
                                                               int *__restrict__ table)
{
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x, step = (long long)gridDim.x * kThreads;
    for (long long i = gid; i < words; i += step)
        stats[i] = 0;
    const long long rows = head->fits ? head->rows_needed : 0;
    for (long long r = gid; r < rows; r += step) {
        table[2 * r] = INT_MAX;
        table[2 * r + 1] = -1;
    }
}

// 3 ------------------------------------------------------------------------------------------------------------------------
// The sums of one instance that a lane has gathered, and their way into stats: reduced over the lanes of the group, added by its
// first lane.  Counts and first moments of a wave fit 32 bits (64 lanes x kMorphRows windows, coordinates below 2^15).
struct MorphSums {
    unsigned cnt[5] = {0, 0, 0, 0, 0};             // A, Q1, Q2, QD, Q3
    unsigned sx = 0, sy = 0;
    u64 sxx = 0, syy = 0, sxy = 0;
};

__device__ inline void add_to_stats(u64 *stats, int key, bool first, u64 area, u64 sx, u64 sy, u64 sxx, u64 syy, u64 sxy, u64 n1, u64 n2,
                                    u64 nd, u64 n3)
{
    if (first) {
        u64 *row = stats + (size_t)(key - 1) * 10;                     // 1 <= key <= n
        const u64 v[10] = {area, sx, sy, sxx, syy, sxy, n1, n2, nd, n3};
#pragma unroll
        for (int j = 0; j < 10; ++j)
            if (v[j])
                __hip_atomic_fetch_add(row + j, v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kThreads) void morph_map_kernel(const int *__restrict__ L, const int *__restrict__ boxes, int n, int H, int W,
                                                             const MorphHead *__restrict__ head, const MorphSlot *__restrict__ slots,
                                                             const int *__restrict__ slot_of, int *table, u64 *stats)
{
    const int lane = threadIdx.x & 63;
    const int tiles_x = W / kThreads + 1;          // ceil((W + 1) / 256)
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int x = tx * kThreads + (int)threadIdx.x;
    const int y_begin = ty * kMorphRows, y_end = y_begin + kMorphRows < H + 1 ? y_begin + kMorphRows : H + 1;      // the workgroup's
    const bool col = x <= W, hl = col && x > 0, hr = x < W;
    const int fits = head->fits, n_slots = head->n_slots;
    // the row above the first window: the labels at (x-1, y-1) and (x, y-1), background beyond the map and beyond n
    int up0 = 0, up1 = 0;
    if (y_begin > 0) {
        const size_t row = (size_t)(y_begin - 1) * W;
        if (hl) {
            const int v = L[row + x - 1];
            up0 = v >= 1 && v <= n ? v : 0;
        }
        if (hr) {
            const int v = L[row + x];
            up1 = v >= 1 && v <= n ? v : 0;
        }
    }
    int kept = 0;                                  // the instance whose sums stay in this lane's registers until the end
    MorphSums acc;
    for (int y = y_begin; y < y_end; ++y) {        // the same rows in every lane of the workgroup
        int c0 = 0, c1 = 0, right = 0;
        if (y < H) {
            const size_t row = (size_t)y * W;
            if (hl) {
                const int v = L[row + x - 1];
                c0 = v >= 1 && v <= n ? v : 0;
            }
            if (hr) {
                const int v = L[row + x];
                c1 = v >= 1 && v <= n ? v : 0;
                right = x + 1 < W ? L[row + x + 1] : 0;               // compared with the own id only, which is in range
            }
        }
        const int id[4] = {up0, up1, c0, c1};      // (x-1, y-1), (x, y-1), (x-1, y), (x, y): the last one is the lane's own pixel
        const int own = c1;
        up0 = c0;
        up1 = c1;

        // the row table: before the grouping, so that its loads are in flight during it
        if (own && fits) {
            const int *box = boxes + 4 * (size_t)(own - 1);           // 1 <= own <= n
            const int x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
            const bool inside = x >= x0 && x < x1 && y >= y0 && y < y1;
            const bool left_end = c0 != own || x == x0, right_end = right != own || x == x1 - 1;
            if (inside && (left_end || right_end)) {
                const int v = slot_of[own - 1];    // >= 0 exactly for a valid box, and `inside` of an invalid one may still hold
                if (v >= 0 && v < n_slots) {
                    const MorphSlot *s = slots + v;
                    if (s->inst == own && x0 == s->x0 && y0 == s->y0 && x1 == s->x1 && y1 == s->y1) {
                        int *row = table + 2 * (s->row_off + (y - y0));                  // a row of the slot: below rows_needed
                        if (left_end)
                            __hip_atomic_fetch_min(row, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (right_end)
                            __hip_atomic_fetch_max(row + 1, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
        }

        if (!kept)                                 // the first instance the lane meets: its own pixel's if there is one
            kept = own ? own : id[0] ? id[0] : id[1] ? id[1] : id[2];
        // every lane of the wave gets here.  Position k of the window is taken in round k if no earlier position holds its
        // instance; what belongs to the kept instance stays in the lane, the rest is grouped and added at once.
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int key = id[k];
            bool fresh = key != 0;
            int m = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (id[j] == key)
                    m |= 1 << j;
                if (j < k && id[j] == key)
                    fresh = false;
            }
            const int c = __popc(m);
            const bool q1 = c == 1, q3 = c == 3, qd = m == 9 || m == 6, q2 = c == 2 && !qd;        // 9: (x-1,y-1) + (x,y); 6: the other diagonal
            const bool mine_px = fresh && key == own;                  // the own pixel goes with the round that takes its instance
            if (fresh && key == kept) {
                acc.cnt[0] += mine_px, acc.cnt[1] += q1, acc.cnt[2] += q2, acc.cnt[3] += qd, acc.cnt[4] += q3;
                if (mine_px) {
                    acc.sx += (unsigned)x, acc.sy += (unsigned)y;
                    acc.sxx += (u64)x * x, acc.syy += (u64)y * y, acc.sxy += (u64)x * y;
                }
            }
            for_each_wave_group(fresh && key != kept, key, [&](int first, u64 grp, bool mine) {
                const u64 area = (u64)__popcll(__ballot(mine && mine_px));
                const u64 n1 = (u64)__popcll(__ballot(mine && q1)), n2 = (u64)__popcll(__ballot(mine && q2));
                const u64 nd = (u64)__popcll(__ballot(mine && qd)), n3 = (u64)__popcll(__ballot(mine && q3));
                unsigned sx = 0, sy = 0;           // at most 64 * 32767
                u64 sxx = 0, syy = 0, sxy = 0;
                if (area) {                        // wave-uniform
                    const bool px = mine && mine_px;
                    sx = px ? (unsigned)x : 0;
                    sy = px ? (unsigned)y : 0;
                    sxx = (u64)sx * sx, syy = (u64)sy * sy, sxy = (u64)sx * sy;
#pragma unroll
                    for (int off = 32; off; off >>= 1) {
                        sx += __shfl_xor(sx, off);
                        sy += __shfl_xor(sy, off);
                        sxx += __shfl_xor(sxx, off);
                        syy += __shfl_xor(syy, off);
                        sxy += __shfl_xor(sxy, off);
                    }
                }
                add_to_stats(stats, key, lane == first, area, sx, sy, sxx, syy, sxy, n1, n2, nd, n3);
            });
        }
    }
    // the kept sums: every lane of the wave gets here too
    for_each_wave_group(kept != 0, kept, [&](int first, u64 grp, bool mine) {
        MorphSums s = mine ? acc : MorphSums();
#pragma unroll
        for (int off = 32; off; off >>= 1) {
#pragma unroll
            for (int j = 0; j < 5; ++j)
                s.cnt[j] += __shfl_xor(s.cnt[j], off);
            s.sx += __shfl_xor(s.sx, off);
            s.sy += __shfl_xor(s.sy, off);
            s.sxx += __shfl_xor(s.sxx, off);
            s.syy += __shfl_xor(s.syy, off);
            s.sxy += __shfl_xor(s.sxy, off);
        }
        add_to_stats(stats, kept, lane == first, s.cnt[0], s.sx, s.sy, s.sxx, s.syy, s.sxy, s.cnt[1], s.cnt[2], s.cnt[3], s.cnt[4]);
    });
}

// 4 ------------------------------------------------------------------------------------------------------------------------
// Candidate c of a slot of `height` rows from row_off on, whose box begins at y0: the left (c even) or right (c odd) end of row
// c / 2, packed x | y << 16, or -1 where the row holds no pixel of the instance or c lies beyond the box.
__device__ inline int candidate(const int *__restrict__ table, long long row_off, int y0, int height, long long c)
{
    const long long r = c >> 1;
    if (r >= height)
        return -1;
    const int *row = table + 2 * (row_off + r);
    const int lo = row[0], hi = row[1];
    if (hi < 0)
        return -1;
    return ((c & 1) ? hi : lo) | ((y0 + (int)r) << 16);               // x, y <= 32767
}

__global__ __launch_bounds__(kThreads) void morph_feret_kernel(const MorphHead *__restrict__ head, MorphSlot *slots,
                                                               const int *__restrict__ table)
{
    __shared__ int tile_a[kMorphTile], tile_b[kMorphTile];
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
        const long long row_off = slots[v].row_off;                   // (field by field: best is left to the atomics)
        const int y0 = slots[v].y0, height = slots[v].y1 - y0;
        const int tiles = (int)morph_tiles(height);
        int k = (int)(t - slots[v].task_off), a = 0;                  // 0 <= k < tiles * (tiles + 1) / 2
        while (a < tiles - 1 && k >= tiles - a) {
            k -= tiles - a;
            ++a;
        }
        const int b = a + k < tiles ? a + k : tiles - 1;
        const long long left = 2ll * height - (long long)b * kMorphTile;     // the candidates of tile b and beyond: >= 1
        const int nb = (int)(left < kMorphTile ? left : kMorphTile);
        __syncthreads();                           // the tiles of the task before are read to the end
        tile_a[threadIdx.x] = candidate(table, row_off, y0, height, (long long)a * kMorphTile + threadIdx.x);
        tile_b[threadIdx.x] = candidate(table, row_off, y0, height, (long long)b * kMorphTile + threadIdx.x);
        __syncthreads();
        const int p = tile_a[threadIdx.x];
        int best = 0;
        if (p >= 0) {
            const int px = p & 0xFFFF, py = p >> 16;
            for (int j = 0; j < nb; ++j) {
                const int q = tile_b[j];           // every lane the same word: a broadcast
                const int dx = (q & 0xFFFF) - px, dy = (q >> 16) - py;
                const int d = dx * dx + dy * dy;   // <= 2 * 32767^2
                best = q >= 0 && d > best ? d : best;
            }
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const int o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
        if ((threadIdx.x & 63) == 0 && best > 0)
            __hip_atomic_fetch_max(&slots[v].best, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// 5 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void morph_finish_kernel(const MorphHead *__restrict__ head, const MorphSlot *__restrict__ slots, int n,
                                                                int *__restrict__ feret2)
{
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x, step = (long long)gridDim.x * kThreads;
    const int n_slots = head->n_slots;
    for (long long v = gid; v < n_slots; v += step) {
        const int inst = slots[v].inst;            // launch 1's: 1..n
        if (inst >= 1 && inst <= n)
            feret2[inst - 1] = slots[v].best;
    }
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" gs_status gs_morphometry_plan(int height, int width, long long rows_cap, size_t *workspace_bytes)
{
    GS_REQUIRE(workspace_bytes, "gs_morphometry_plan: null argument");
    MorphometryPlan plan;
    const gs_status st = plan_morphometry(height, width, rows_cap, plan);
    *workspace_bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_instance_morphometry(const int32_t *labels, const int32_t *boxes, int n, int height, int width, void *workspace,
                                             size_t workspace_bytes, long long rows_cap, unsigned long long *stats, int32_t *feret2,
                                             long long *rows_needed, void *hip_stream)
{
    MorphometryPlan plan;
    const gs_status st = plan_morphometry(height, width, rows_cap, plan);
    if (st != GS_OK)
        return st;
    GS_REQUIRE(n >= 0, "gs_instance_morphometry: n must not be negative (got %d)", n);
    GS_REQUIRE(aligned(labels, 4), "gs_instance_morphometry: labels is NULL or not 4-byte aligned");
    GS_REQUIRE(n == 0 || aligned(boxes, 4), "gs_instance_morphometry: boxes is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 8), "gs_instance_morphometry: workspace is NULL or not 8-byte aligned");
    GS_REQUIRE(n == 0 || aligned(stats, 8), "gs_instance_morphometry: stats is NULL or not 8-byte aligned");
    GS_REQUIRE(n == 0 || aligned(feret2, 4), "gs_instance_morphometry: feret2 is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(rows_needed, 8), "gs_instance_morphometry: rows_needed is NULL or not 8-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_instance_morphometry: rows_cap %lld needs %zu bytes of workspace (got %zu)", rows_cap,
               plan.bytes, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char *ws = static_cast<char *>(workspace);
    MorphHead *head = reinterpret_cast<MorphHead *>(ws + plan.head_off);
    MorphSlot *slots = reinterpret_cast<MorphSlot *>(ws + plan.slot_off);
    int *table = reinterpret_cast<int *>(ws + plan.rows_off);

    hipLaunchKernelGGL(morph_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, boxes, n, height, width, plan.rows_cap, head, slots, feret2,
                       rows_needed);
    if (n > 0) {
        const long long words = 10ll * n, most = words > plan.rows_cap ? words : plan.rows_cap;
        const long long clear_blocks = (most - 1) / kThreads + 1;
        hipLaunchKernelGGL(morph_clear_kernel, dim3((unsigned)(clear_blocks < kMorphMaxGrid ? clear_blocks : kMorphMaxGrid)), dim3(kThreads), 0,
                           s, stats, words, head, table);
        hipLaunchKernelGGL(morph_map_kernel, dim3((unsigned)plan.window_blocks), dim3(kThreads), 0, s, labels, boxes, n, height, width, head,
                           slots, feret2, table, stats);
        hipLaunchKernelGGL(morph_feret_kernel, dim3((unsigned)plan.stride_blocks), dim3(kThreads), 0, s, head, slots, table);
        hipLaunchKernelGGL(morph_finish_kernel, dim3((unsigned)plan.stride_blocks), dim3(kThreads), 0, s, head, slots, n, feret2);
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
}
