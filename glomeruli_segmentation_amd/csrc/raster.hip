// Polygons back to a map (csrc/raster_abi.h, gs_polygon_raster): features, each a set of rings of fixed-point vertices, painted
// into an int32 owner map by the even-odd rule at pixel centres.  The inverse of gs_instance_outlines: the loops traced from a
// label map give that label map back.  The definitions (coordinates, crossings, inside, owner, words) are the header's;
// everything is integer.
//
// gs_polygon_raster keeps a head, 28 bytes per feature and a word per 32 toggle columns of every row of every feature's box in
// the caller's workspace (raster_plan.h), in 8 launches, none of which needs a sort:
//   1 ras_init_kernel    one lane per feature: the empty box.  One lane per pixel: owner = 0.
//   2 ras_box_kernel     one lane per point: its ring by binary search in ring_offsets, its feature from ring_feature, its toggle
//                        column and row by raster_first_pixel -- the ceil and clamp of the rule, and monotone, so every later t
//                        lies between the columns of its edge's ends and every crossed row between their rows.  The lanes of a
//                        wave are grouped by feature (for_each_wave_group), reduced by shuffles, at most one atomic min / max
//                        per group on each of the feature's four box words: none where a relaxed load shows it cannot change.
//   3 ras_size_kernel    one lane per feature: the words of its box (raster_abi.h, "words"), the words of the features in front
//                        of it in its workgroup (a shuffle scan per wave, the waves' sums in LDS) and the workgroup's sum.
//   4 ras_scan_kernel    one workgroup of 1024: the block sums become the words in front of each block (wave_block.h's scan with
//                        64-bit sums: the boxes of 2^31 features can hold more than 2^31 words); the total is words_needed and
//                        decides whether the result fits.  Writes the head, counts[0] and counts[1] = 0, or -1 where it does not.
//   5 ras_clear_kernel   one lane per scratch word below words_needed: zero.  One lane per feature: its word base.
//   6 ras_cross_kernel   one lane per point, that is per edge (to the next point of its ring): it walks the rows it crosses and
//                        issues one 32-bit atomic exclusive-or per crossing; an upright edge (X0 == X1, every edge of a traced
//                        outline) takes its column once, by the same arithmetic.  The crossings are summed per wave by shuffles
//                        and added to counts[1] with one 64-bit atomic.
//   7 ras_fill_kernel    one lane per scratch word: its feature by binary search in the word bases, then its row and its place
//                        in the row.  The carry is the parity of the popcounts of the words in front of it in the row, the prefix
//                        exclusive-or inside the word takes five shift steps, and every set bit inside the map is one
//                        atomic max of feature + 1 on owner: the wave takes its words two at a time, a lane per bit.  Reads the
//                        scratch, writes only owner.
//   8 ras_class_kernel   only where class_map is given: one lane per pixel, feature_class[owner - 1] or 0.
// Launches 2 and 6 are issued only where there are points and rings.  Launches 5..7 are sized by words_cap and n_features: a
// lane beyond words_needed, and every lane where the result does not fit, does nothing.  The entry reads no device value: the
// grids follow from the sizes given on the host.
//
// Why the result is exact: a toggle at (row j, column t) flips the parity of every pixel (x, j) with x >= t, so after launch 6
// bit t of row j holds the parity of the feature's crossings at t, and the inclusive prefix exclusive-or along the row is the
// header's "inside".  A closed ring crosses a row an even number of times, so the parity is 0 behind the box.
//
// Why the bytes do not depend on the run: the boxes are minima and maxima, the scratch is zeroed and then only toggled, owner
// is zeroed and then only raised, counts[1] is zeroed and then only added to, with integers.  Everything else is written by one
// thread as a pure function of what earlier launches left.
//
// Visibility: across launches the kernel boundary alone; a launch never reads what it writes, with one exception argued at
// lower() / raise(): launch 2 looks at a box word, with a relaxed agent-scope load, only to leave out an atomic that could not
// change it.  The boxes in launch 2, the scratch and counts[1] in launch 6 and owner in launch 7 are otherwise touched only
// through agent-scope atomics whose results are unused.
//
// Rules: those of wave_block.h.  The loops of this file's own --
//   the binary searches       32 rounds, a constant; the interval [lo, hi] only shrinks and halves while lo < hi
//   the wave and block scans  off doubles up to 64, d up to 1024; b rises by one over the thread's run of blocks
//   the shuffle reductions    off halves from 32
//   the rows of an edge       j rises by one from the edge's first row to its last, both within [0, height]
//   the carry of a word       k rises by one over the words in front of it in its row: fewer than the words of a row
//   the words of a wave       i rises by one from 0 to 32: two words a round
//
// Memory safety, whatever ring_offsets holds: a ring index comes out of the search within [0, n_rings), whatever the values
// compared; ring_offsets is read at ring and ring + 1 only.  An edge is walked only where ring start <= point < ring end <=
// n_points, so the next point is one of [0, n_points).  A feature index is tested against n_features before it indexes a box.
// A scratch word is touched only where its row and bit lie inside the feature's box and its index is below words_needed <=
// words_cap (launch 6), or is the lane's own index below words_needed (launch 7); a pixel only inside the map.  Offsets that
// break the rule of the header can therefore change what is painted, never where memory is touched.
#include "gs_internal.h"
#include "raster_abi.h"
#include "raster_plan.h"
#include "wave_block.h"

namespace gs {

namespace {

typedef unsigned long long u64;

constexpr int kThreads = kRasterThreads;
static_assert(kThreads == 256 && kThreads == kFlagThreads, "four waves a workgroup");

// the largest index in [0, n) whose value is at most v (0 where none is), for values that do not decrease; n >= 1
__device__ inline int last_at_most(const int *__restrict__ a, int n, int v)
{
    int lo = 0, hi = n - 1;
    for (int k = 0; k < 32; ++k)
        if (lo < hi) {
            const int mid = lo + (hi - lo + 1) / 2;
            if (a[mid] <= v)
                lo = mid;
            else
                hi = mid - 1;
        }
    return lo;
}

// vertex i in units of 1/(2S) pixel, clamped on load
__device__ inline void load_vertex(const int *__restrict__ points, int i, long long &X, long long &Y)
{
    X = 2ll * raster_clamp_coord(points[2 * (size_t)i]);
    Y = 2ll * raster_clamp_coord(points[2 * (size_t)i + 1]);
}

// *word = min(*word, v) / max(*word, v), the atomic issued only where it can still change the word.  In launch 2 a word only
// falls (rises), so whatever value the relaxed load returns, however stale, bounds the final one: a skipped atomic would have
// changed nothing, and the final word is the same minimum (maximum) of the same values.  Without the test every wave of a
// feature of millions of points queues on its one box (measured: 10.9 of 14.9 ms on the noise map of tools/raster_rate.py).
__device__ inline void lower(int *word, int v)
{
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v)
        atomicMin(word, v);
}
__device__ inline void raise(int *word, int v)
{
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v)
        atomicMax(word, v);
}

// 1 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ras_init_kernel(RasterBox *__restrict__ box, int n_features, int *__restrict__ owner, int n_pixels)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n_features) {
        RasterBox b;
        b.col_min = b.row_min = INT_MAX;
        b.col_max = b.row_max = INT_MIN;
        box[i] = b;
    }
    if (i < n_pixels)
        owner[i] = 0;
}

// 2 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ras_box_kernel(const int *__restrict__ points, int n_points, const int *__restrict__ ring_offsets,
                                                           const int *__restrict__ ring_feature, int n_rings, int n_features, int S, int H,
                                                           int W, RasterBox *box)
{
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    bool todo = false;
    int f = 0, c = 0, r = 0;
    if (i < n_points) {
        f = ring_feature[last_at_most(ring_offsets, n_rings, (int)i)];
        if (f >= 0 && f < n_features) {
            long long X, Y;
            load_vertex(points, (int)i, X, Y);
            c = raster_first_pixel(X, S, W);
            r = raster_first_pixel(Y, S, H);
            todo = true;
        }
    }
    // every lane of the wave gets here
    for_each_wave_group(todo, f, [&](int first, u64 group, bool mine) {
        int c0 = mine ? c : INT_MAX, c1 = mine ? c : INT_MIN, r0 = mine ? r : INT_MAX, r1 = mine ? r : INT_MIN;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            c0 = min(c0, __shfl_xor(c0, off));
            c1 = max(c1, __shfl_xor(c1, off));
            r0 = min(r0, __shfl_xor(r0, off));
            r1 = max(r1, __shfl_xor(r1, off));
        }
        if (lane == first) {
            lower(&box[f].col_min, c0);
            raise(&box[f].col_max, c1);
            lower(&box[f].row_min, r0);
            raise(&box[f].row_max, r1);
        }
    });
}

// 3 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ras_size_kernel(const RasterBox *__restrict__ box, int n_features,
                                                            long long *__restrict__ feature_front, long long *__restrict__ block_words)
{
    __shared__ long long wave_sum[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long f = (long long)blockIdx.x * kThreads + threadIdx.x;
    long long words = 0;
    if (f < n_features) {
        const RasterBox b = box[f];
        words = raster_box_rows(b) * raster_box_row_words(b);
    }
    long long inc = words;
    for (int off = 1; off < 64; off <<= 1) {
        const long long o = __shfl_up(inc, off);
        if (lane >= off)
            inc += o;
    }
    if (lane == 63)
        wave_sum[wave] = inc;
    __syncthreads();                               // the workgroup's one barrier, reached by all
    long long before = inc - words, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const long long s = wave_sum[w];
        before += w < wave ? s : 0;
        total += s;
    }
    if (f < n_features)
        feature_front[f] = before;
    if (threadIdx.x == 0)
        block_words[blockIdx.x] = total;
}

// 4 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void ras_scan_kernel(long long *__restrict__ block_words, int n_blocks, int words_cap,
                                                                RasterHead *__restrict__ head, long long *__restrict__ counts)
{
    __shared__ long long s[kScanThreads];
    const int t = (int)threadIdx.x, run = (n_blocks + kScanThreads - 1) / kScanThreads;
    const long long lo = (long long)t * run, hi = lo + run < n_blocks ? lo + run : n_blocks;
    long long sum = 0;
    for (long long b = lo; b < hi; ++b)
        sum += block_words[b];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const long long v = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    const long long total = s[kScanThreads - 1];   // below 2^63: raster_plan.h
    long long base = s[t] - sum;
    for (long long b = lo; b < hi; ++b) {
        const long long c = block_words[b];
        block_words[b] = base;
        base += c;
    }
    if (t == 0) {
        const bool fits = total <= words_cap;
        head->words_needed = total;
        head->fits = fits ? 1 : 0;
        head->pad = 0;
        counts[0] = total;
        counts[1] = fits ? 0 : -1;
    }
}

// 5 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ras_clear_kernel(const RasterHead *__restrict__ head, const long long *__restrict__ feature_front,
                                                             const long long *__restrict__ block_words, int n_features,
                                                             int *__restrict__ feature_base, unsigned *__restrict__ scratch)
{
    if (!head->fits)
        return;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < head->words_needed)
        scratch[i] = 0;
    if (i < n_features)
        feature_base[i] = (int)(block_words[blockIdx.x] + feature_front[i]);       // at most words_needed <= words_cap: an int
}

// 6 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ras_cross_kernel(const int *__restrict__ points, int n_points, const int *__restrict__ ring_offsets,
                                                             const int *__restrict__ ring_feature, int n_rings, int n_features, int S, int H,
                                                             int W, const RasterHead *__restrict__ head, const RasterBox *__restrict__ box,
                                                             const int *__restrict__ feature_base, unsigned *scratch, long long *counts)
{
    if (!head->fits)                               // the whole grid
        return;
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    long long applied = 0;
    if (i < n_points) {
        const int ring = last_at_most(ring_offsets, n_rings, (int)i);
        const int start = ring_offsets[ring], end = ring_offsets[ring + 1], f = ring_feature[ring];
        if (start >= 0 && start <= i && i < end && end <= n_points && f >= 0 && f < n_features) {
            const int next = i + 1 < end ? (int)i + 1 : start;
            long long X0, Y0, X1, Y1;
            load_vertex(points, (int)i, X0, Y0);
            load_vertex(points, next, X1, Y1);
            if (Y0 > Y1) {
                const long long x = X0, y = Y0;
                X0 = X1, Y0 = Y1, X1 = x, Y1 = y;
            }
            const RasterBox b = box[f];
            const long long rows = raster_box_rows(b), row_words = raster_box_row_words(b), needed = head->words_needed;
            const long long den = Y1 - Y0, dx = X1 - X0, base = feature_base[f];
            const int j0 = raster_first_pixel(Y0, S, H), j1 = raster_first_pixel(Y1, S, H);     // none where Y0 == Y1
            const int upright = raster_first_pixel(X0, S, W);
            for (int j = j0; j < j1; ++j) {
                int t = upright;
                if (dx != 0) {
                    const long long num = X0 * den + ((2ll * j + 1) * S - Y0) * dx;              // below 2^61: raster_abi.h
                    const long long q = raster_ceil_div(num - S * den, 2ll * S * den);
                    t = q < 0 ? 0 : q > W ? W : (int)q;
                }
                const long long row = (long long)j - b.row_min, bit = (long long)t - b.col_min;
                const long long word = base + row * row_words + (bit >> 5);
                if (row >= 0 && row < rows && bit >= 0 && (bit >> 5) < row_words && word < needed) {
                    atomicXor(scratch + word, 1u << (bit & 31));
                    ++applied;
                }
            }
        }
    }
    // every lane of the wave gets here
#pragma unroll
    for (int off = 32; off; off >>= 1)
        applied += __shfl_xor(applied, off);
    if (lane == 0 && applied)
        __hip_atomic_fetch_add(reinterpret_cast<u64 *>(counts + 1), (u64)applied, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 7 ------------------------------------------------------------------------------------------------------------------------
// A lane first finds the inside bits of its own word; then the wave paints its 64 words two at a time, a lane per bit, so that
// one atomic instruction covers two runs of 32 neighbouring pixels and not 64 pixels of 64 different rows or words (measured
// on the 287-disc map of tools/raster_rate.py: 190 us with a lane painting its own word bit by bit).
__global__ __launch_bounds__(kThreads) void ras_fill_kernel(const RasterHead *__restrict__ head, const RasterBox *__restrict__ box,
                                                            const int *__restrict__ feature_base, int n_features,
                                                            const unsigned *__restrict__ scratch, int H, int W, int *owner)
{
    if (!head->fits || n_features < 1)             // the whole grid
        return;
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * kThreads + threadIdx.x;
    unsigned inside = 0;                           // the bits of this lane's word that are pixels inside its feature
    int pixel = 0, mark = 0;                       // the pixel of bit 0, and feature + 1
    if (w < head->words_needed) {
        const int f = last_at_most(feature_base, n_features, (int)w);
        const RasterBox b = box[f];
        const long long rows = raster_box_rows(b), row_words = raster_box_row_words(b), local = w - feature_base[f];
        if (local >= 0 && local < rows * row_words) {
            const long long row = local / row_words, k = local - row * row_words;
            unsigned carry = 0;
            for (long long front = w - k; front < w; ++front)
                carry ^= __popc(scratch[front]);
            unsigned v = scratch[w];
            v ^= v << 1;
            v ^= v << 2;
            v ^= v << 4;
            v ^= v << 8;
            v ^= v << 16;
            if (carry & 1)
                v = ~v;
            const long long y = b.row_min + row, x0 = b.col_min + 32 * k;
            long long bits = (long long)b.col_max + 1 - x0;           // the box's bits in this word and behind it
            if (bits > W - x0)
                bits = W - x0;                                         // ... that are pixels of the map
            if (y >= 0 && y < H && x0 >= 0 && bits > 0) {
                inside = bits < 32 ? v & ((1u << bits) - 1) : v;
                pixel = (int)(y * W + x0);                             // pixel + bit < height * width for every bit kept
                mark = f + 1;
            }
        }
    }
    // every lane of the wave gets here; round i paints the words of lanes 2 i and 2 i + 1
    const int half = lane >> 5, bit = lane & 31;
    for (int i = 0; i < 32; ++i) {
        const unsigned m = __shfl(inside, 2 * i + half);
        const int p = __shfl(pixel, 2 * i + half), k = __shfl(mark, 2 * i + half);
        if (m >> bit & 1)
            atomicMax(owner + p + bit, k);
    }
}

// 8 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ras_class_kernel(const int *__restrict__ owner, int n_pixels, const unsigned char *__restrict__ feature_class,
                                                             int n_features, unsigned char *__restrict__ class_map)
{
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_pixels)
        return;
    const int o = owner[p];
    class_map[p] = o >= 1 && o <= n_features ? feature_class[o - 1] : 0;
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" gs_status gs_polygon_raster_plan(int height, int width, long long n_points, long long n_rings, long long n_features,
                                            long long words_cap, size_t *workspace_bytes)
{
    GS_REQUIRE(workspace_bytes, "gs_polygon_raster_plan: null argument");
    RasterPlan plan;
    const gs_status st = plan_raster(height, width, n_points, n_rings, n_features, words_cap, plan);
    *workspace_bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_polygon_raster(const int32_t *points, long long n_points, const int32_t *ring_offsets, const int32_t *ring_feature,
                                       long long n_rings, const uint8_t *feature_class, long long n_features, int frac_bits, int height,
                                       int width, void *workspace, size_t workspace_bytes, long long words_cap, int32_t *owner,
                                       uint8_t *class_map, long long *counts, void *hip_stream)
{
    RasterPlan plan;
    gs_status st = plan_raster(height, width, n_points, n_rings, n_features, words_cap, plan);
    if (st != GS_OK)
        return st;
    if ((st = check_raster_frac_bits("gs_polygon_raster", frac_bits)) != GS_OK)
        return st;
    GS_REQUIRE(n_points == 0 || aligned(points, 4), "gs_polygon_raster: points is NULL or not 4-byte aligned");
    GS_REQUIRE(n_rings == 0 || aligned(ring_offsets, 4), "gs_polygon_raster: ring_offsets is NULL or not 4-byte aligned");
    GS_REQUIRE(n_rings == 0 || aligned(ring_feature, 4), "gs_polygon_raster: ring_feature is NULL or not 4-byte aligned");
    GS_REQUIRE(!class_map || feature_class, "gs_polygon_raster: class_map is given without feature_class");
    GS_REQUIRE(aligned(workspace, 16), "gs_polygon_raster: workspace is NULL or not 16-byte aligned");
    GS_REQUIRE(aligned(owner, 4), "gs_polygon_raster: owner is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(counts, 8), "gs_polygon_raster: counts is NULL or not 8-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_polygon_raster: %lld features and words_cap %lld need %zu bytes of workspace (got %zu)",
               n_features, words_cap, plan.bytes, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char *ws = static_cast<char *>(workspace);
    RasterHead *head = reinterpret_cast<RasterHead *>(ws + plan.head_off);
    RasterBox *box = reinterpret_cast<RasterBox *>(ws + plan.box_off);
    long long *feature_front = reinterpret_cast<long long *>(ws + plan.feature_front_off);
    long long *block_words = reinterpret_cast<long long *>(ws + plan.block_words_off);
    int *feature_base = reinterpret_cast<int *>(ws + plan.feature_base_off);
    unsigned *scratch = reinterpret_cast<unsigned *>(ws + plan.scratch_off);
    const int S = 1 << frac_bits;
    const bool edges = plan.n_points > 0 && plan.n_rings > 0;
    const dim3 block(kThreads), pixel_grid((unsigned)plan.pixel_blocks), point_grid((unsigned)plan.point_blocks);
    const dim3 feature_grid((unsigned)plan.feature_blocks), word_grid((unsigned)plan.word_blocks);
    const dim3 init_grid((unsigned)(plan.pixel_blocks > plan.feature_blocks ? plan.pixel_blocks : plan.feature_blocks));
    const dim3 clear_grid((unsigned)(plan.word_blocks > plan.feature_blocks ? plan.word_blocks : plan.feature_blocks));

    hipLaunchKernelGGL(ras_init_kernel, init_grid, block, 0, s, box, plan.n_features, owner, plan.n_pixels);
    if (edges)
        hipLaunchKernelGGL(ras_box_kernel, point_grid, block, 0, s, points, plan.n_points, ring_offsets, ring_feature, plan.n_rings,
                           plan.n_features, S, height, width, box);
    hipLaunchKernelGGL(ras_size_kernel, feature_grid, block, 0, s, box, plan.n_features, feature_front, block_words);
    hipLaunchKernelGGL(ras_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, block_words, plan.feature_blocks, plan.words_cap, head, counts);
    hipLaunchKernelGGL(ras_clear_kernel, clear_grid, block, 0, s, head, feature_front, block_words, plan.n_features, feature_base, scratch);
    if (edges)
        hipLaunchKernelGGL(ras_cross_kernel, point_grid, block, 0, s, points, plan.n_points, ring_offsets, ring_feature, plan.n_rings,
                           plan.n_features, S, height, width, head, box, feature_base, scratch, counts);
    hipLaunchKernelGGL(ras_fill_kernel, word_grid, block, 0, s, head, box, feature_base, plan.n_features, scratch, height, width, owner);
    if (class_map)
        hipLaunchKernelGGL(ras_class_kernel, pixel_grid, block, 0, s, owner, plan.n_pixels, feature_class, plan.n_features, class_map);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
